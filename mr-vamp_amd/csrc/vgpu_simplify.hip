// vgpu_simplify.hip -- batched path simplification (planning/simplify.hh:192-260) in lockstep on the device.
//
// n_paths paths in one environment each follow the sequential algorithm of vcpu_simplify.cpp; what they share
// is the round: every path still working names the motions it needs validated next, one vgpu_validate_motions
// call checks the compact list of all of them, and every path consumes its own results.
//   straight   one edge front -> back (simplify.hh:222-230);
//   shortcut   the row of waypoint i: edges (path[i], path[j]) for j = len-1 ... i+2, farthest first; the
//              sequential walk takes the first valid one in that order, i.e. the valid edge with the smallest
//              position in the row, whatever the others are (simplify.hh:127-138);
//   B-spline   after Path::subdivide the even indices 2 ... len-3 are updated from their odd neighbours only,
//              which no update writes, so all of a step's midpoints and their two edges are independent
//              (simplify.hh:31-44).
// The control flow between those rounds (operation order, iteration counter, `any`, the step loop, the
// capacity stop) is per-path state on the device, advanced by the resolve kernel; a path that is done emits
// no edges.  One wave (64 lanes) per path everywhere: rows and candidate lists are strided over the lanes
// and decided with 64-bit ballots.
// Arithmetic is the CPU's, bit for bit: interpolate = a + (b - a) * t unfused (-ffp-contract=off), distance =
// l2_norm in the AVX lane order with __builtin_sqrtf (vgpu_rake.hh:16-41).
#include <hip/hip_runtime.h>

#include "../../include/vamp_gpu.h"
#include "vgpu_simplify.hh"

namespace vgpu {

constexpr int kWave = 64;
constexpr int kScanBlock = 1024;

// FloatVector<dim>::l2_norm of b - a: squares in the hsum lane order, two registers as fma(lo, lo, hi * hi)
__device__ __forceinline__ float distance_d(const float* __restrict__ a, const float* __restrict__ b, uint32_t dim)
{
    float sq[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float lo = (uint32_t)j < dim ? b[j] - a[j] : 0.0f;
        if (dim <= 8) {
            sq[j] = lo * lo;
        } else {
            const float hi = (uint32_t)(j + 8) < dim ? b[j + 8] - a[j + 8] : 0.0f;
            sq[j] = __builtin_fmaf(lo, lo, hi * hi);
        }
    }
    const float x = (sq[0] + sq[4]) + (sq[2] + sq[6]);
    const float y = (sq[1] + sq[5]) + (sq[3] + sq[7]);
    return __builtin_sqrtf(x + y);
}

// smooth_bspline's midpoint of waypoint idx (simplify.hh:33-35), component j
__device__ __forceinline__ float midpoint_j(const float* __restrict__ w, uint32_t dim, uint32_t j, float m)
{
    const float p = w[j], prev = (w - dim)[j], next = (w + dim)[j];
    const float t1 = p + (prev - p) * m;
    const float t2 = p + (next - p) * m;
    return t1 + (t2 - t1) * 0.5f;
}

// path[idx].distance(midpoint) (simplify.hh:37)
__device__ __forceinline__ float midpoint_change(const float* __restrict__ w, uint32_t dim, float m)
{
    float sq[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float lo = (uint32_t)j < dim ? midpoint_j(w, dim, j, m) - w[j] : 0.0f;
        if (dim <= 8) {
            sq[j] = lo * lo;
        } else {
            const float hi = (uint32_t)(j + 8) < dim ? midpoint_j(w, dim, j + 8, m) - w[j + 8] : 0.0f;
            sq[j] = __builtin_fmaf(lo, lo, hi * hi);
        }
    }
    const float x = (sq[0] + sq[4]) + (sq[2] + sq[6]);
    const float y = (sq[1] + sq[5]) + (sq[3] + sq[7]);
    return __builtin_sqrtf(x + y);
}

__device__ __forceinline__ float* path_of(const SimplifyArgs& a, uint32_t buf, uint32_t p)
{
    return a.buf[buf] + (size_t)p * a.cap * a.dim;
}

// The path's control flow from the end of an operation (or the failed straight-line test) to the next round
// that needs edges (simplify.hh:239-256).  `finished`: the running operation returned s[SP_CHANGED].
__device__ __forceinline__ void advance(const SimplifyArgs& a, uint32_t* s, uint32_t len, bool finished)
{
    if (finished) {
        s[SP_ANY] |= s[SP_CHANGED];
        s[SP_OP] += 1;
    } else {  // entering the iteration loop
        s[SP_ANY] = 1;
        s[SP_OP] = a.n_ops;
    }
    for (;;) {
        while (s[SP_OP] < a.n_ops) {
            const bool shortcut = a.ops[s[SP_OP]] == VGPU_SIMPLIFY_SHORTCUT;
            s[SP_CHANGED] = 0;
            if (len >= 3 && shortcut) {  // simplify.hh:121-127
                s[SP_PHASE] = SPH_SHORTCUT;
                s[SP_I] = 0;
                return;
            }
            if (len >= 3 && !shortcut && a.max_steps > 0) {  // simplify.hh:20-26
                s[SP_PHASE] = SPH_BSPLINE;
                s[SP_STEP] = 0;
                return;
            }
            s[SP_OP] += 1;  // the operation returns false at once
        }
        if (!s[SP_ANY] || s[SP_ITER] >= a.max_iterations) {  // simplify.hh:241,251-254
            s[SP_PHASE] = SPH_DONE;
            return;
        }
        s[SP_ITER] += 1;
        s[SP_ANY] = 0;
        s[SP_OP] = 0;
    }
}

__global__ void __launch_bounds__(256) simplify_init_kernel(SimplifyArgs a)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n_paths) return;
    uint32_t* s = a.st + (size_t)p * kSimplifyWords;
    const uint32_t len = a.len[p];
    for (uint32_t k = 0; k < kSimplifyWords; ++k) s[k] = 0;
    s[SP_STATUS] = len > a.cap ? VGPU_SIMPLIFY_CAPACITY : VGPU_SIMPLIFY_DONE;
    s[SP_PHASE] = (len > 2 && len <= a.cap) ? SPH_STRAIGHT : SPH_DONE;
}

// One wave per path: the number of edges the path needs this round.  A B-spline step subdivides into the other
// buffer first (Path::subdivide, plan.hh:34-49), unless that would exceed the limit, and lists the even indices
// whose midpoint moves them by more than min_change.
__global__ void __launch_bounds__(kWave) simplify_prepare_kernel(SimplifyArgs a)
{
    const uint32_t p = blockIdx.x, lane = threadIdx.x, dim = a.dim;
    uint32_t* s = a.st + (size_t)p * kSimplifyWords;
    const uint32_t phase = s[SP_PHASE], len = a.len[p], buf = s[SP_BUF];
    uint32_t cnt = 0;
    if (phase == SPH_STRAIGHT) {
        cnt = 1;
    } else if (phase == SPH_SHORTCUT) {
        cnt = len - s[SP_I] - 2;
    } else if (phase == SPH_BSPLINE) {
        const uint32_t n2 = 2 * len - 1;
        if (n2 > a.limit) {
            if (lane == 0) {
                s[SP_STATUS] = VGPU_SIMPLIFY_CAPACITY;
                s[SP_PHASE] = SPH_DONE;
                a.cnt[p] = 0;
            }
            return;
        }
        const float* src = path_of(a, buf, p);
        float* dst = path_of(a, buf ^ 1, p);
        for (uint32_t x = lane; x < n2 * dim; x += kWave) {
            const uint32_t w = x / dim, j = x - w * dim, k = w >> 1;
            const float c = src[k * dim + j];
            dst[x] = (w & 1) ? c + (src[(k + 1) * dim + j] - c) * 0.5f : c;
        }
        __syncthreads();  // the candidates read what other lanes wrote
        uint32_t* cand = a.cand + (size_t)p * a.cap;
        const uint32_t n_even = len - 2;  // indices 2, 4 ... 2 len - 4 (simplify.hh:31)
        uint32_t base = 0;
        for (uint32_t t0 = 0; t0 < n_even; t0 += kWave) {
            const uint32_t t = t0 + lane, idx = 2 + 2 * t;
            const bool moved = t < n_even && midpoint_change(dst + (size_t)idx * dim, dim, a.midpoint) > a.min_change;
            const unsigned long long mask = __ballot(moved);
            if (moved) cand[base + __popcll(mask & ((1ull << lane) - 1))] = idx;
            base += __popcll(mask);
        }
        cnt = 2 * base;
        if (lane == 0) {
            s[SP_BUF] = buf ^ 1;
            a.len[p] = n2;
        }
    }
    if (lane == 0) a.cnt[p] = cnt;
}

// Exclusive scan of cnt[0 .. n_paths) into off[0 .. n_paths], one block; the total and the number of paths
// still working go to the pinned words the driver reads after the round's synchronisation.
__global__ void __launch_bounds__(kScanBlock) simplify_scan_kernel(SimplifyArgs a)
{
    __shared__ uint32_t wave_sum[kScanBlock / kWave];
    __shared__ uint32_t wave_act[kScanBlock / kWave];
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    uint32_t carry = 0, active = 0;
    for (uint32_t base = 0; base < a.n_paths; base += kScanBlock) {
        const uint32_t i = base + tid;
        const uint32_t v = i < a.n_paths ? a.cnt[i] : 0;
        const bool act = i < a.n_paths && a.st[(size_t)i * kSimplifyWords + SP_PHASE] != SPH_DONE;
        uint32_t incl = v;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, kWave);
            if ((int)lane >= d) incl += up;
        }
        const uint32_t n_act = (uint32_t)__popcll(__ballot(act));
        if (lane == kWave - 1) wave_sum[wave] = incl;
        if (lane == 0) wave_act[wave] = n_act;
        __syncthreads();
        uint32_t before = 0, chunk = 0;
        for (uint32_t w = 0; w < kScanBlock / kWave; ++w) {
            if (w < wave) before += wave_sum[w];
            chunk += wave_sum[w];
            active += wave_act[w];
        }
        if (i < a.n_paths) a.off[i] = carry + before + incl - v;
        carry += chunk;
        __syncthreads();
    }
    if (tid == 0) {
        a.off[a.n_paths] = carry;
        a.host[0] = carry;
        a.host[1] = active;
    }
}

// One wave per path: its edges into the round's compact list at off[p].
__global__ void __launch_bounds__(kWave) simplify_emit_kernel(SimplifyArgs a)
{
    const uint32_t p = blockIdx.x, lane = threadIdx.x, dim = a.dim;
    const uint32_t* s = a.st + (size_t)p * kSimplifyWords;
    const uint32_t phase = s[SP_PHASE], len = a.len[p], cnt = a.cnt[p];
    if (phase == SPH_DONE || cnt == 0) return;
    const float* w = path_of(a, s[SP_BUF], p);
    float* es = a.starts + (size_t)a.off[p] * dim;
    float* eg = a.goals + (size_t)a.off[p] * dim;
    if (phase == SPH_STRAIGHT) {
        if (lane < dim) {
            es[lane] = w[lane];
            eg[lane] = w[(size_t)(len - 1) * dim + lane];
        }
    } else if (phase == SPH_SHORTCUT) {
        const uint32_t i = s[SP_I];
        for (uint32_t x = lane; x < cnt * dim; x += kWave) {  // candidate k is j = len - 1 - k
            const uint32_t k = x / dim, j = x - k * dim;
            es[x] = w[(size_t)i * dim + j];
            eg[x] = w[(size_t)(len - 1 - k) * dim + j];
        }
    } else {
        const uint32_t* cand = a.cand + (size_t)p * a.cap;
        for (uint32_t k = lane; k < cnt / 2; k += kWave) {  // (path[idx-1], midpoint), (midpoint, path[idx+1])
            const float* c = w + (size_t)cand[k] * dim;
            float* s0 = es + (size_t)2 * k * dim;
            float* g0 = eg + (size_t)2 * k * dim;
            for (uint32_t j = 0; j < dim; ++j) {
                const float mid = midpoint_j(c, dim, j, a.midpoint);
                s0[j] = (c - dim)[j];
                g0[j] = mid;
                s0[dim + j] = mid;
                g0[dim + j] = (c + dim)[j];
            }
        }
    }
}

// One wave per path: consume the round's results and advance the path's control state.
__global__ void __launch_bounds__(kWave) simplify_resolve_kernel(SimplifyArgs a)
{
    const uint32_t p = blockIdx.x, lane = threadIdx.x, dim = a.dim;
    uint32_t* sg = a.st + (size_t)p * kSimplifyWords;
    uint32_t s[kSimplifyWords];
#pragma unroll
    for (int k = 0; k < (int)kSimplifyWords; ++k) s[k] = sg[k];
    const uint32_t phase = s[SP_PHASE], cnt = a.cnt[p];
    if (phase == SPH_DONE) return;
    uint32_t len = a.len[p];
    float* w = path_of(a, s[SP_BUF], p);
    const uint8_t* ok = a.ok + a.off[p];
    if (phase == SPH_STRAIGHT) {
        if (ok[0]) {  // [front, back]
            if (lane < dim) w[dim + lane] = w[(size_t)(len - 1) * dim + lane];
            len = 2;
            s[SP_PHASE] = SPH_DONE;
        } else {
            advance(a, s, len, false);
        }
    } else if (phase == SPH_SHORTCUT) {
        uint32_t found = cnt;  // first valid candidate of the row = largest valid j
        for (uint32_t k0 = 0; k0 < cnt; k0 += kWave) {
            const uint32_t k = k0 + lane;
            const unsigned long long mask = __ballot(k < cnt && ok[k] != 0);
            if (mask) {
                found = k0 + (uint32_t)__ffsll((long long)mask) - 1;
                break;
            }
        }
        const uint32_t i = s[SP_I];
        if (found < cnt) {  // erase (i, j): close the gap in place, front to back (dst < src)
            const uint32_t j = len - 1 - found, n = (len - j) * dim;
            const float* src = w + (size_t)j * dim;
            float* dst = w + (size_t)(i + 1) * dim;
            for (uint32_t x0 = 0; x0 < n; x0 += kWave) {
                const uint32_t x = x0 + lane;
                const float v = x < n ? src[x] : 0.0f;
                __syncthreads();
                if (x < n) dst[x] = v;
                __syncthreads();
            }
            len = i + 1 + (len - j);
            s[SP_CHANGED] = 1;
        }
        s[SP_I] = i + 1;
        if (!(i + 1 + 2 < len)) advance(a, s, len, true);  // simplify.hh:127 re-reads path.size()
    } else {
        const uint32_t* cand = a.cand + (size_t)p * a.cap;
        const float* eg = a.goals + (size_t)a.off[p] * dim;
        bool mine = false;
        for (uint32_t k = lane; k < cnt / 2; k += kWave) {
            if (ok[2 * k] && ok[2 * k + 1]) {  // simplify.hh:38-42
                float* c = w + (size_t)cand[k] * dim;
                for (uint32_t j = 0; j < dim; ++j) c[j] = eg[(size_t)2 * k * dim + j];
                mine = true;
            }
        }
        const bool updated = __ballot(mine) != 0;
        if (updated) s[SP_CHANGED] = 1;
        s[SP_STEP] += 1;
        if (!updated || s[SP_STEP] >= a.max_steps) advance(a, s, len, true);  // simplify.hh:26,46-49
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < (int)kSimplifyWords; ++k) sg[k] = s[k];
        a.len[p] = len;
    }
}

// One wave per path: the result back into the caller's buffer, iterations, status and Path::cost
// (plan.hh:13-32: segment lengths added in order).
__global__ void __launch_bounds__(kWave) simplify_finish_kernel(SimplifyArgs a, uint32_t* iterations, uint8_t* status,
                                                                float* cost)
{
    __shared__ float seg[kWave];
    const uint32_t p = blockIdx.x, lane = threadIdx.x, dim = a.dim;
    const uint32_t* s = a.st + (size_t)p * kSimplifyWords;
    const uint32_t len = a.len[p];
    float* w = path_of(a, 0, p);
    if (s[SP_BUF] == 1) {
        const float* src = path_of(a, 1, p);
        for (uint32_t x = lane; x < len * dim; x += kWave) w[x] = src[x];
        __syncthreads();
    }
    if (lane == 0) {
        if (iterations) iterations[p] = s[SP_ITER];
        if (status) status[p] = (uint8_t)s[SP_STATUS];
    }
    if (!cost) return;
    float total = len >= 2 && len <= a.cap ? 0.0f : __builtin_inff();
    if (len >= 2 && len <= a.cap) {
        for (uint32_t i0 = 0; i0 + 1 < len; i0 += kWave) {
            const uint32_t i = i0 + lane;
            if (i + 1 < len) seg[lane] = distance_d(w + (size_t)i * dim, w + (size_t)(i + 1) * dim, dim);
            __syncthreads();
            if (lane == 0) {
                const uint32_t n = len - 1 - i0 < (uint32_t)kWave ? len - 1 - i0 : (uint32_t)kWave;
                for (uint32_t k = 0; k < n; ++k) total += seg[k];
            }
            __syncthreads();
        }
    }
    if (lane == 0) cost[p] = total;
}

}  // namespace vgpu

extern "C" hipError_t vgpu_launch_simplify_init(const vgpu::SimplifyArgs* a, hipStream_t st)
{
    hipLaunchKernelGGL(vgpu::simplify_init_kernel, dim3((a->n_paths + 255) / 256), dim3(256), 0, st, *a);
    return hipGetLastError();
}

extern "C" hipError_t vgpu_launch_simplify_prepare(const vgpu::SimplifyArgs* a, hipStream_t st)
{
    hipLaunchKernelGGL(vgpu::simplify_prepare_kernel, dim3(a->n_paths), dim3(vgpu::kWave), 0, st, *a);
    hipLaunchKernelGGL(vgpu::simplify_scan_kernel, dim3(1), dim3(vgpu::kScanBlock), 0, st, *a);
    return hipGetLastError();
}

extern "C" hipError_t vgpu_launch_simplify_emit(const vgpu::SimplifyArgs* a, hipStream_t st)
{
    hipLaunchKernelGGL(vgpu::simplify_emit_kernel, dim3(a->n_paths), dim3(vgpu::kWave), 0, st, *a);
    return hipGetLastError();
}

extern "C" hipError_t vgpu_launch_simplify_resolve(const vgpu::SimplifyArgs* a, hipStream_t st)
{
    hipLaunchKernelGGL(vgpu::simplify_resolve_kernel, dim3(a->n_paths), dim3(vgpu::kWave), 0, st, *a);
    return hipGetLastError();
}

extern "C" hipError_t vgpu_launch_simplify_finish(const vgpu::SimplifyArgs* a, uint32_t* iterations, uint8_t* status,
                                                  float* cost, hipStream_t st)
{
    hipLaunchKernelGGL(vgpu::simplify_finish_kernel, dim3(a->n_paths), dim3(vgpu::kWave), 0, st, *a, iterations, status,
                       cost);
    return hipGetLastError();
}
