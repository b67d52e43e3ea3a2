// vgpu_kernels.hip -- gfx950 kernels of the motion-validation rake.
//
// Per robot (Panda today; sphere_fk lives in vgpu_fk.hip):
//   fkcc           one lane per configuration (rake group G = 1 == a configuration broadcast
//                  to all 8 reference lanes): per-configuration validity mask
//                  (fk.hh:1335-6276 interleaved_sphere_fk);
//   validate       validate_motion over a batch of edges (planning/validate.hh:23-75) in two
//                  phases with the reference's early-exit semantics:
//                    head  one 8-lane group per edge evaluates the first rake block
//                          (t = 1/8 .. 8/8, validate.hh:31-44) and computes n_e;
//                    scan  edges that survive with n_e > 1 get n_e - 1 work items;
//                    tail  one 8-lane group per (edge, back-step k) evaluates block k,
//                          reached by the reference's k sequential subtractions
//                          (validate.hh:50-56), and clears the edge's flag on a hit.
//                  On collision-heavy scenes most invalid edges die in the head block
//                  (59.5 % of the bench edges, 0.06 % later), so the tail runs only for the
//                  survivors, and adjacent groups of the tail are neighbouring blocks of one
//                  edge (correlated branches).  The edge result equals the reference's
//                  sequential loop: it is the AND of its blocks.
// All of this is VALU code: FK is 7 chained quaternion products + sparse 3x3 transforms,
// nothing is a dense contraction worth MFMA (DESIGN.md "Why no MFMA").
#include <hipcub/hipcub.hpp>

#include "vgpu_lean.hh"
#include "vgpu_panda.hh"
#include "vgpu_staged.hh"

namespace vgpu {

template <bool EXT>
__global__ __launch_bounds__(kBlock, VGPU_WAVES_PER_EU) void panda_fkcc_kernel(const float* __restrict__ q, size_t n, EnvView env,
                                                            float bx, float by, float bz,
                                                            uint8_t* __restrict__ valid)
{
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float* qi = q + 7 * i;
    valid[i] = panda_fkcc<Grp1, EXT>(qi[0], qi[1], qi[2], qi[3], qi[4], qi[5], qi[6], env, bx, by, bz) ? 1 : 0;
}

// ---- sampling: Halton<7> draw -> scale_configuration -> fkcc (prm.hh:236-251) ----
__global__ __launch_bounds__(kBlock) void panda_sample_kernel(uint64_t first, size_t n, float* __restrict__ q)
{
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float v[7];
    panda_sample(first + i, v);
#pragma unroll
    for (int d = 0; d < 7; ++d) q[7 * i + d] = v[d];
}

template <bool EXT>
__global__ __launch_bounds__(kBlock, VGPU_WAVES_PER_EU) void panda_sample_fkcc_kernel(
    uint64_t first, size_t n, EnvView env, float bx, float by, float bz, float* __restrict__ q,
    uint8_t* __restrict__ valid)
{
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float v[7];
    panda_sample(first + i, v);
    if (q) {
#pragma unroll
        for (int d = 0; d < 7; ++d) q[7 * i + d] = v[d];
    }
    valid[i] = panda_fkcc<Grp1, EXT>(v[0], v[1], v[2], v[3], v[4], v[5], v[6], env, bx, by, bz) ? 1 : 0;
}

template <bool EXT>
__global__ __launch_bounds__(kBlock, VGPU_WAVES_PER_EU) void panda_validate_head_kernel(
    const float* __restrict__ starts, const float* __restrict__ goals, size_t n_edges, EnvView env, float bx,
    float by, float bz, uint8_t* __restrict__ ok, int32_t* __restrict__ n_blocks, uint32_t* __restrict__ cnt)
{
    const size_t tid = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const size_t e = tid >> 3;  // one 8-lane rake group per edge
    const int lane = (int)(tid & 7);
    if (e >= n_edges) return;   // group-uniform
    const float* s = starts + 7 * e;
    const Rake rk = rake_setup(s, goals + 7 * e);
    const float pct = (float)(lane + 1) / 8.0f;  // validate.hh:11-21
    float b[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) b[j] = __builtin_fmaf(rk.v[j], pct, s[j]);  // validate.hh:37 (contracted)
    const bool valid = panda_fkcc<Grp8, EXT>(b[0], b[1], b[2], b[3], b[4], b[5], b[6], env, bx, by, bz);
    if (lane == 0) {
        ok[e] = valid ? 1 : 0;
        if (n_blocks) n_blocks[e] = rk.n;
        cnt[e] = (valid && rk.n > 1) ? (uint32_t)(rk.n - 1) : 0u;
    }
}

__global__ __launch_bounds__(kBlock) void gather_rows_kernel(const float* __restrict__ q, const uint32_t* __restrict__ idx,
                                                             const uint32_t* __restrict__ count, int dim,
                                                             float* __restrict__ out)
{
    const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const size_t j = t / (size_t)dim;
    if (j >= *count) return;
    const int d = (int)(t - j * (size_t)dim);
    out[t] = q[(size_t)idx[j] * dim + d];
}

__global__ __launch_bounds__(kBlock) void scatter_items_kernel(const uint32_t* __restrict__ cnt,
                                                               const uint32_t* __restrict__ off, size_t n_edges,
                                                               uint32_t* __restrict__ item_edge)
{
    const size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n_edges) return;
    const uint32_t c = cnt[e], o = off[e];
    for (uint32_t i = 0; i < c; ++i) item_edge[o + i] = (uint32_t)e;
}

template <bool EXT>
__global__ __launch_bounds__(kBlock, VGPU_WAVES_PER_EU) void panda_validate_tail_kernel(
    const float* __restrict__ starts, const float* __restrict__ goals, const uint32_t* __restrict__ item_edge,
    const uint32_t* __restrict__ off, size_t n_items, EnvView env, float bx, float by, float bz,
    uint8_t* __restrict__ ok)
{
    const size_t tid = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const size_t it = tid >> 3;  // one 8-lane rake group per (edge, back-step)
    const int lane = (int)(tid & 7);
    if (it >= n_items) return;   // group-uniform
    const uint32_t e = item_edge[it];
    const int k = (int)(it - off[e]) + 1;  // back-step index 1 .. n_e - 1
    const float* s = starts + 7 * (size_t)e;
    const Rake rk = rake_setup(s, goals + 7 * (size_t)e);
    const float pct = (float)(lane + 1) / 8.0f;
    const float div = (float)(8 * (size_t)rk.n);
    float b[7], back[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        b[j] = __builtin_fmaf(rk.v[j], pct, s[j]);
        back[j] = rk.v[j] / div;  // validate.hh:50
    }
    for (int i = 0; i < k; ++i) {  // the reference's sequential subtraction chain, bit for bit
#pragma unroll
        for (int j = 0; j < 7; ++j) b[j] = b[j] - back[j];
    }
    const bool valid = panda_fkcc<Grp8, EXT>(b[0], b[1], b[2], b[3], b[4], b[5], b[6], env, bx, by, bz);
    if (lane == 0 && !valid) ok[e] = 0;  // every writer stores 0: the race is benign
}

// 64-bit total of the per-edge back-step counts after a MONOLITHIC head kernel (the staged pipelines' tail_counts
// kernels sum while they count, vgpu_lean.hh item_total_block): the item scan is 32-bit, so a batch whose blocks
// exceed 2^32 must be rejected before its offsets are trusted.
__global__ __launch_bounds__(kBlock) void item_total_kernel(uint32_t* __restrict__ cnt, size_t n, ItemTotalArgs t)
{
    unsigned long long s = 0;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) s += cnt[i];
    item_total_block<kBlock>(s, cnt, n, t);
}

// The scan of a staged pass's per-(check, block) counts (vgpu_staged.hh count_kernel: counts[c * nb + block]):
// one block per check scans its nb counts into offs, RELATIVE to the check's first block -- queue_kernel uses
// only offs[c * nb + block] - offs[c * nb] and the plan only the per-check totals, so no scan across checks,
// no sentinel and no scan workspace.  Tiles of kScanTile counts with a carried prefix, any nb.
// The block whose ticket comes last (the ticket word is zero between launches: that block resets it)
//   - stores the per-check totals into the pinned host array host_fired (when given: the pass's read-back is
//     then a synchronisation, no copy command),
//   - writes bnd[0 .. checks]: their running sum, the segment boundaries plan_kernel reads (stride 1),
//   - lays out the round's plan when the round's check set is known at launch (plan != NULL): what
//     plan_kernel<R, EXT> computes, from the same class table (cls.of[c] = ChildClassesE<R, EXT>::of(c)).
// Not a template: a kernel templated on the robot alone is one symbol across a robot's part translation units
// (vgpu_staged.hip kClasses).
constexpr int kScanTile = 1024;
__global__ __launch_bounds__(kScanTile) void staged_scan_kernel(const uint32_t* __restrict__ counts,
                                                                uint32_t* __restrict__ offs, uint32_t nb,
                                                                uint32_t checks, uint32_t* __restrict__ fired,
                                                                uint32_t* __restrict__ bnd,
                                                                uint32_t* __restrict__ ticket,
                                                                uint32_t* __restrict__ host_fired,
                                                                StagedPlan* __restrict__ plan, StagedClassTable cls,
                                                                uint64_t set, uint32_t W, uint32_t n_groups)
{
    constexpr int kWaves = kScanTile / 64;
    __shared__ uint32_t wsum[2][kWaves];
    __shared__ uint32_t tot[kPlanMaxChecks], pad[kPlanMaxChecks];
    __shared__ uint32_t is_last;
    const uint32_t c = blockIdx.x;
    const uint32_t* __restrict__ in = counts + (size_t)c * nb;
    uint32_t* __restrict__ out = offs + (size_t)c * nb;
    const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
    uint32_t carry = 0;  // block-uniform: the counts of the tiles before this one
    uint32_t next = threadIdx.x < nb ? in[threadIdx.x] : 0u;
    for (uint32_t base = 0, buf = 0; base < nb; base += kScanTile, buf ^= 1u) {
        const uint32_t i = base + threadIdx.x;  // nb < 2^23 (n_groups < 2^31): no wrap
        const uint32_t x = next;
        next = (i + kScanTile < nb) ? in[i + kScanTile] : 0u;  // the next tile's load overlaps this tile's scan
        uint32_t s = x;  // inclusive scan within the wave
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t t = __shfl_up(s, d);
            if (lane >= d) s += t;
        }
        if (lane == 63) wsum[buf][w] = s;
        __syncthreads();  // one barrier per tile: the next tile writes the other buffer
        uint32_t pre = 0, all = 0;
        for (int k = 0; k < kWaves; ++k) {
            const uint32_t v = wsum[buf][k];
            pre += (k < w) ? v : 0u;
            all += v;
        }
        if (i < nb) out[i] = carry + pre + s - x;
        carry += all;
    }
    if (threadIdx.x == 0) {
        // the total leaves this thread (write-through store, drained) before its ticket is taken; the last ticket
        // holder reads the totals past its L1 (agent-scope loads)
        __hip_atomic_store(fired + c, carry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        is_last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == checks - 1u;
    }
    __syncthreads();
    if (!is_last) return;
    if (threadIdx.x < kPlanMaxChecks) {
        const bool have = threadIdx.x < checks;
        const uint32_t f = have ? __hip_atomic_load(fired + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        const bool on = have && ((set >> threadIdx.x) & 1u);
        tot[threadIdx.x] = f;
        pad[threadIdx.x] = on ? (f + W - 1) / W * W : 0u;  // the check's segment, padded to whole waves
        if (have && host_fired) host_fired[threadIdx.x] = f;
    }
    __syncthreads();
    if (threadIdx.x > kPlanMaxChecks) return;  // lane checks (<= 64) writes the last boundary
    if (threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // one lane per check: its boundary (checks in order) and its segment start (class-major, then in order);
    // lanes 0 .. kPlanMaxClasses - 1 also sum their class's range
    const uint32_t k = threadIdx.x;
    const uint32_t my_cls = k < checks ? cls.of[k] : 0xFFu;
    uint32_t before = 0, start = 0, lo = 0, hi = 0;
    for (uint32_t j = 0; j < checks; ++j) {
        const uint32_t cj = cls.of[j], pj = pad[j];
        before += (j < k) ? tot[j] : 0u;
        start += (cj < my_cls || (cj == my_cls && j < k)) ? pj : 0u;
        lo += (cj < k) ? pj : 0u;
        hi += (cj <= k) ? pj : 0u;
    }
    if (k <= checks) bnd[k] = before;
    if (!plan) return;
    if (k < checks) {  // what plan_kernel<R, EXT> lays out
        const bool on = (set >> k) & 1u;
        plan->start[k] = start;
        plan->fill[k] = start + (on ? tot[k] : 0u);
        plan->end[k] = start + pad[k];
    }
    if (k < (uint32_t)kPlanMaxClasses) {  // classes the robot does not have stay empty
        plan->lo[k] = lo;
        plan->hi[k] = hi;
    }
    if (k == 0) {
        uint32_t total = 0;
        for (uint32_t j = 0; j < checks; ++j) total += pad[j];
        plan->total = total;
        plan->n_groups = n_groups;
    }
}

}  // namespace vgpu

static bool has_ext(const EnvView* env) { return env->n_hf > 0 || env->n_pc > 0; }

extern "C" {

hipError_t vgpu_launch_panda_fkcc(const float* q, size_t n, const EnvView* env, float bx, float by, float bz,
                                  uint8_t* valid, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const unsigned grid = (unsigned)((n + vgpu::kBlock - 1) / vgpu::kBlock);
    if (has_ext(env))
        hipLaunchKernelGGL(vgpu::panda_fkcc_kernel<true>, dim3(grid), dim3(vgpu::kBlock), 0, st, q, n, *env, bx, by,
                           bz, valid);
    else
        hipLaunchKernelGGL(vgpu::panda_fkcc_kernel<false>, dim3(grid), dim3(vgpu::kBlock), 0, st, q, n, *env, bx, by,
                           bz, valid);
    return hipGetLastError();
}

hipError_t vgpu_launch_panda_sample(uint64_t first, size_t n, float* q, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const unsigned grid = (unsigned)((n + vgpu::kBlock - 1) / vgpu::kBlock);
    hipLaunchKernelGGL(vgpu::panda_sample_kernel, dim3(grid), dim3(vgpu::kBlock), 0, st, first, n, q);
    return hipGetLastError();
}

hipError_t vgpu_launch_panda_sample_fkcc(uint64_t first, size_t n, const EnvView* env, float bx, float by, float bz,
                                         float* q, uint8_t* valid, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const unsigned grid = (unsigned)((n + vgpu::kBlock - 1) / vgpu::kBlock);
    if (has_ext(env))
        hipLaunchKernelGGL(vgpu::panda_sample_fkcc_kernel<true>, dim3(grid), dim3(vgpu::kBlock), 0, st, first, n,
                           *env, bx, by, bz, q, valid);
    else
        hipLaunchKernelGGL(vgpu::panda_sample_fkcc_kernel<false>, dim3(grid), dim3(vgpu::kBlock), 0, st, first, n,
                           *env, bx, by, bz, q, valid);
    return hipGetLastError();
}

// Compaction of valid samples (the PRM vertex stage): out_q[j] = q[idx[j]], idx ascending.
size_t vgpu_compact_bytes(size_t n)
{
    size_t tmp = 0;
    (void)hipcub::DeviceSelect::Flagged(nullptr, tmp, hipcub::CountingInputIterator<uint32_t>(0),
                                        (const uint8_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (int)n);
    return tmp;
}

hipError_t vgpu_launch_gather_rows(const float* q, const uint32_t* idx, const uint32_t* count, size_t max_rows,
                                   int dim, float* out, hipStream_t st)
{
    if (max_rows == 0) return hipSuccess;
    const size_t threads = max_rows * (size_t)dim;
    const unsigned grid = (unsigned)((threads + vgpu::kBlock - 1) / vgpu::kBlock);
    hipLaunchKernelGGL(vgpu::gather_rows_kernel, dim3(grid), dim3(vgpu::kBlock), 0, st, q, idx, count, dim, out);
    return hipGetLastError();
}

hipError_t vgpu_launch_compact(const uint8_t* valid, size_t n, uint32_t* idx_out, uint32_t* count, void* tmp,
                               size_t tmp_bytes, hipStream_t st)
{
    return hipcub::DeviceSelect::Flagged(tmp, tmp_bytes, hipcub::CountingInputIterator<uint32_t>(0), valid, idx_out,
                                         count, (int)n, st);
}

// Workspace for the two-phase validate: cnt[n_edges + 1], off[n_edges + 1], scan temp.
size_t vgpu_validate_scan_bytes(size_t n_edges)
{
    size_t tmp = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                           (int)(n_edges + 1));
    return tmp;
}

hipError_t vgpu_launch_scan(const uint32_t* cnt, uint32_t* off, size_t n_edges, void* scan_tmp, size_t scan_bytes,
                            hipStream_t st)
{
    return hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, cnt, off, (int)(n_edges + 1), st);
}

hipError_t vgpu_launch_panda_validate_head(const float* starts, const float* goals, size_t n_edges,
                                           const EnvView* env, float bx, float by, float bz, uint8_t* ok,
                                           int32_t* n_blocks, uint32_t* cnt, hipStream_t st)
{
    const size_t threads = n_edges * 8;
    const unsigned grid = (unsigned)((threads + vgpu::kBlock - 1) / vgpu::kBlock);
    if (has_ext(env))
        hipLaunchKernelGGL(vgpu::panda_validate_head_kernel<true>, dim3(grid), dim3(vgpu::kBlock), 0, st, starts,
                           goals, n_edges, *env, bx, by, bz, ok, n_blocks, cnt);
    else
        hipLaunchKernelGGL(vgpu::panda_validate_head_kernel<false>, dim3(grid), dim3(vgpu::kBlock), 0, st, starts,
                           goals, n_edges, *env, bx, by, bz, ok, n_blocks, cnt);
    return hipGetLastError();
}

hipError_t vgpu_launch_item_total(uint32_t* cnt, size_t n, const ItemTotalArgs* t, hipStream_t st)
{
    const size_t want = (n + vgpu::kBlock - 1) / vgpu::kBlock;
    const unsigned grid = (unsigned)(want < 256 ? (want ? want : 1) : 256);
    hipLaunchKernelGGL(vgpu::item_total_kernel, dim3(grid), dim3(vgpu::kBlock), 0, st, cnt, n, *t);
    return hipGetLastError();
}

// plan = NULL: the totals and boundaries only (the round's check set is chosen from them on the host)
hipError_t vgpu_launch_staged_scan(const uint32_t* counts, uint32_t* offs, uint32_t nb, int checks, uint32_t* fired,
                                   uint32_t* bnd, uint32_t* ticket, uint32_t* host_fired, void* plan,
                                   const StagedClassTable* cls, uint64_t set, uint32_t W, uint32_t n_groups,
                                   hipStream_t st)
{
    if (checks < 1 || checks > vgpu::kPlanMaxChecks || nb == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vgpu::staged_scan_kernel, dim3((unsigned)checks), dim3(vgpu::kScanTile), 0, st, counts, offs,
                       nb, (uint32_t)checks, fired, bnd, ticket, host_fired, (vgpu::StagedPlan*)plan, *cls, set, W,
                       n_groups);
    return hipGetLastError();
}

hipError_t vgpu_launch_scatter_items(const uint32_t* cnt, const uint32_t* off, size_t n_edges, uint32_t* item_edge,
                                     hipStream_t st)
{
    if (n_edges == 0) return hipSuccess;
    const unsigned grid = (unsigned)((n_edges + vgpu::kBlock - 1) / vgpu::kBlock);
    hipLaunchKernelGGL(vgpu::scatter_items_kernel, dim3(grid), dim3(vgpu::kBlock), 0, st, cnt, off, n_edges,
                       item_edge);
    return hipGetLastError();
}

hipError_t vgpu_launch_panda_validate_tail(const float* starts, const float* goals, size_t n_edges,
                                           size_t n_items, const EnvView* env, float bx, float by, float bz,
                                           uint8_t* ok, const uint32_t* cnt, const uint32_t* off,
                                           uint32_t* item_edge, hipStream_t st)
{
    if (n_items == 0) return hipSuccess;
    unsigned grid = (unsigned)((n_edges + vgpu::kBlock - 1) / vgpu::kBlock);
    hipLaunchKernelGGL(vgpu::scatter_items_kernel, dim3(grid), dim3(vgpu::kBlock), 0, st, cnt, off, n_edges,
                       item_edge);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    const size_t threads = n_items * 8;
    grid = (unsigned)((threads + vgpu::kBlock - 1) / vgpu::kBlock);
    if (has_ext(env))
        hipLaunchKernelGGL(vgpu::panda_validate_tail_kernel<true>, dim3(grid), dim3(vgpu::kBlock), 0, st, starts,
                           goals, item_edge, off, n_items, *env, bx, by, bz, ok);
    else
        hipLaunchKernelGGL(vgpu::panda_validate_tail_kernel<false>, dim3(grid), dim3(vgpu::kBlock), 0, st, starts,
                           goals, item_edge, off, n_items, *env, bx, by, bz, ok);
    return hipGetLastError();
}

}  // extern "C"
