// vgpu_rrtc.hip -- batched RRT-Connect (planning/rrtc.hh:33-248): one wave per planning problem.
//
// P problems each follow vcpu_rrtc.cpp statement for statement, all in one environment (rrtc_kernel) or each in the
// environment it names (rrtc_scenes_kernel: a device table of views and an index per problem; the search itself,
// rrtc_search, is the same function).  Nothing couples them, so a problem is one wave64 that runs its whole
// search inside the kernel -- sampling, nearest neighbours, the inline collision check, tree growth and path
// extraction -- and the host only relaunches until no problem is left working (a launch advances a problem by at
// most `slice` iterations, so every launch is short).
//   state      wave-uniform values in registers; the trees in the problem's arena (nodes in insertion order
//              with parent, dynamic-domain radius and tree membership), the control words of vgpu_rrtc.hh
//              between launches;
//   sampling   panda_sample(rng_index) (vgpu_panda.hh), one coordinate per lane, read back by the whole wave;
//   nearest    the 64 lanes stride over the arena's nodes, l2_norm in the hsum order, then a wave reduction on
//              (distance, index): the smallest distance, among equals the earliest-inserted node -- what the
//              CPU's scan with `d < dist` keeps;
//   validate   validate_vector(start, v, distance) on the wave: the 8 rake groups take 8 blocks per pass
//              (block k = fma(v, (lane + 1) / 8, start) then k subtractions of v / (8 n), the arithmetic of
//              panda_validate_tail_kernel), n from the caller's distance.  A segment with n < 8 leaves groups
//              free: in the connect phase they take the next segments (start = prior + inc iterated), and the
//              first failing segment in order ends the connect.  Validity is the AND of a segment's blocks, so
//              the blocks evaluated beyond the CPU's sequential early exit cannot change it.
// There is ONE panda_fkcc call site per kernel: the loop below is a state machine around it (M_*), because the
// generated function is thousands of instructions and is inlined.
// Arithmetic is the CPU's, bit for bit (-ffp-contract=off, IEEE division and sqrt).
#include <hip/hip_runtime.h>

#include "vgpu_panda.hh"
#include "vgpu_rrtc.hh"

namespace vgpu {

constexpr int kWave = 64;
constexpr float kFltMax = 3.402823466e+38f;  // std::numeric_limits<float>::max()
// a segment of more blocks than this counts as invalid (only a non-finite or absurd configuration gets here;
// the CPU would evaluate up to 2^31 blocks): it bounds a launch
constexpr int kMaxBlocks = 1 << 16;

enum : int { M_ITER = 0, M_INIT = 1, M_EXT = 2, M_CON = 3 };

// FloatVector<7>::l2_norm in the AVX hsum lane order (vector/avx.hh:441-452); lane 7 is padding 0
__device__ __forceinline__ float l2_norm7(const float v[7])
{
    const float a = (v[0] * v[0] + v[4] * v[4]) + (v[2] * v[2] + v[6] * v[6]);
    const float c = (v[1] * v[1] + v[5] * v[5]) + (v[3] * v[3] + 0.0f);
    return __builtin_sqrtf(a + c);
}

// validate.hh:41 from the caller's distance
__device__ __forceinline__ int blocks_of(float distance)
{
    float nf = __builtin_ceilf(distance / 8.0f * 32.0f);
    if (!(nf > 1.0f)) nf = 1.0f;
    return nf < 2147483520.0f ? (int)nf : 2147483520;
}

__device__ __forceinline__ float uniform_f(float v)
{
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

// panda_sample(k) (vgpu_panda.hh) with one coordinate per lane: lane d < 7 computes coordinate d with the same
// operations, and the wave reads the seven values back by lane -- the draw costs its longest radical inverse
// (base 3) instead of the sum of all seven
__device__ __forceinline__ void wave_sample(uint64_t k, int lane, float q[7])
{
    uint32_t idx, cyc;
    halton_index(k, idx, cyc);
    const uint32_t d = (uint32_t)lane < 7u ? (uint32_t)lane : 0u;
    const float x = __builtin_fmaf(halton_coord(idx, kHaltonPrimes[(d + cyc) % 7u]), panda_s_m[d], panda_s_a[d]);
#pragma unroll
    for (int j = 0; j < 7; ++j) q[j] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), j));
}

struct Arena {
    float* nodes;
    uint32_t* parent;
    float* radius;
    uint8_t* tree;
};

__device__ __forceinline__ void load7(const float* __restrict__ p, float v[7])
{
#pragma unroll
    for (int j = 0; j < 7; ++j) v[j] = p[j];
}

// rrtc.hh:48-53 push: node i = n_nodes (the caller has checked i < node_cap)
__device__ __forceinline__ void push_node(const Arena& t, uint32_t i, const float q[7], uint32_t parent, uint32_t which,
                                          int lane)
{
    if (lane == 0) {  // q is wave-uniform: one lane holds all of it
#pragma unroll
        for (int j = 0; j < 7; ++j) t.nodes[(size_t)i * 7 + j] = q[j];
        t.parent[i] = parent;
        t.radius[i] = kFltMax;
        t.tree[i] = (uint8_t)which;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // the other lanes read these nodes next
}

// nearest node of tree `which` to q: index (wave-uniform) and distance
__device__ __forceinline__ uint32_t nearest(const Arena& t, uint32_t n_nodes, uint32_t which, const float q[7], int lane,
                                            float& dist)
{
    float bd = 0.0f;
    uint32_t bi = 0xffffffffu;
    for (uint32_t i = (uint32_t)lane; i < n_nodes; i += kWave) {
        if (t.tree[i] != which) continue;
        const float* c = t.nodes + (size_t)i * 7;
        float d[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) d[j] = q[j] - c[j];
        const float dd = l2_norm7(d);
        if (bi == 0xffffffffu || dd < bd) {
            bd = dd;
            bi = i;
        }
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const float od = __shfl_xor(bd, off);
        const uint32_t oi = (uint32_t)__shfl_xor((int)bi, off);
        const bool take = oi != 0xffffffffu && (bi == 0xffffffffu || od < bd || (od == bd && oi < bi));
        bd = take ? od : bd;
        bi = take ? oi : bi;
    }
    dist = uniform_f(bd);
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)bi);
}

// one slice of problem p's search in `env` (wave-uniform): the body of both entry kernels below, which differ only
// in where the view comes from.  phase != RPH_DONE (the kernels return before they read a view).
template <bool EXT>
__device__ __forceinline__ void rrtc_search(const RrtcArgs& a, const EnvView& env, unsigned long long* __restrict__ totals,
                                            uint32_t p, uint32_t* ctl, uint32_t phase)
{
    const int lane = (int)threadIdx.x, g = lane >> 3, gl = lane & 7;

    Arena t;
    t.nodes = a.nodes + (size_t)p * a.node_cap * 7;
    t.parent = a.parent + (size_t)p * a.node_cap;
    t.radius = a.radius + (size_t)p * a.node_cap;
    t.tree = a.tree + (size_t)p * a.node_cap;
    const float* __restrict__ start = a.starts + (size_t)p * 7;
    const float* __restrict__ goals = a.goals + (size_t)p * a.n_goals * 7;

    // the problem's state: all wave-uniform
    uint64_t rng = a.rng[p];
    if (rng == 0) {  // halton.hh: draws are 1-based; the host fails the call on totals[3]
        if (lane == 0) {
            ctl[RC_PHASE] = RPH_DONE;
            atomicAdd(totals + 3, 1ull);
        }
        return;
    }
    uint32_t n_nodes = 0, size0 = 0, size1 = 0, ta = 0;
    uint64_t iter = 0;
    int mode = M_INIT;
    if (phase == RPH_SEARCH) {
        n_nodes = ctl[RC_NODES];
        size0 = ctl[RC_SIZE0];
        size1 = ctl[RC_SIZE1];
        ta = ctl[RC_A];
        iter = (uint64_t)ctl[RC_ITER_LO] | ((uint64_t)ctl[RC_ITER_HI] << 32);
        mode = M_ITER;
    }

    // the validation in flight: nseg segments of n blocks each, segment i from base + i * v (iterated), pass
    // jpass of a segment with more than 8 blocks
    float base[7], v[7];
    int n = 1, jpass = 0;
    uint32_t nseg = 1;
    uint32_t gi = 0;           // M_INIT: the goal being tried
    uint32_t nn = 0, on = 0;   // M_EXT: the extended node; M_CON: the node of the other tree
    float nr = 0.0f;           // M_EXT: radii[nn]
    uint32_t done_iters = 0;   // iterations started in this launch

    // result fields of a problem that ends
    bool finished = false;
    int32_t solved = 0;
    uint32_t status = VGPU_RRTC_DONE, out_len = 0;
    float cost = 0.0f;

    if (mode == M_INIT) {  // rrtc.hh:61-73: validate_motion(start, goals[0])
        load7(start, base);
#pragma unroll
        for (int j = 0; j < 7; ++j) v[j] = goals[j] - base[j];
        n = blocks_of(l2_norm7(v));
    }

    for (;;) {
        if (mode == M_ITER) {
            bool leave = false;
            for (;;) {  // rrtc.hh:95: iterations that reject their sample validate nothing
                if (done_iters == a.slice) {
                    leave = true;
                    break;
                }
                const uint64_t it = iter++;
                if (!(it < a.max_iterations)) {
                    finished = leave = true;
                    break;
                }
                if (!(n_nodes < a.max_nodes)) {
                    finished = leave = true;
                    if (a.cap_limited) status = VGPU_RRTC_CAPACITY;
                    break;
                }
                ++done_iters;
                const float asize = (float)(ta ? size1 : size0), bsize = (float)(ta ? size0 : size1);
                const float ratio = __builtin_fabsf(asize - bsize) / asize;
                if (!a.balance || ratio < a.tree_ratio) ta ^= 1u;  // rrtc.hh:101-105
                float temp[7];
                wave_sample(rng++, lane, temp);
                float nd;
                nn = nearest(t, n_nodes, ta, temp, lane, nd);
                nr = t.radius[nn];
                if (a.dynamic_domain && nr < nd) continue;  // rrtc.hh:125-128
                load7(t.nodes + (size_t)nn * 7, base);
                const bool reach = nd < a.range;
                const float sc = a.range / nd;
#pragma unroll
                for (int j = 0; j < 7; ++j) {
                    const float d = temp[j] - base[j];
                    v[j] = reach ? d : d * sc;  // rrtc.hh:132-136
                }
                n = blocks_of(reach ? nd : a.range);
                nseg = 1;
                jpass = 0;
                mode = M_EXT;
                break;
            }
            if (leave) break;
        }

        // ---- one pass: 8 rake blocks ----
        const int pps = (n + 7) >> 3;  // passes per segment
        int seg = 0, blk;
        bool active;
        if (pps == 1) {  // whole segments side by side
            seg = g / n;
            blk = g - seg * n;
            active = seg < 8 / n && (uint32_t)seg < nseg;
        } else {
            blk = 8 * jpass + g;
            active = blk < n;
        }
        active = active && n <= kMaxBlocks;
        bool valid = true;
        if (active) {  // group-uniform
            float s[7], b[7];
#pragma unroll
            for (int j = 0; j < 7; ++j) s[j] = base[j];
            for (int i = 0; i < seg; ++i) {  // prior + inc, iterated (rrtc.hh:180-186)
#pragma unroll
                for (int j = 0; j < 7; ++j) s[j] = s[j] + v[j];
            }
            const float pct = (float)(gl + 1) / 8.0f;  // validate.hh:11-21
#pragma unroll
            for (int j = 0; j < 7; ++j) b[j] = __builtin_fmaf(v[j], pct, s[j]);  // validate.hh:37 (contracted)
            if (blk > 0) {
                const float div = (float)(8 * (size_t)n);
                float back[7];
#pragma unroll
                for (int j = 0; j < 7; ++j) back[j] = v[j] / div;  // validate.hh:50
                for (int i = 0; i < blk; ++i) {
#pragma unroll
                    for (int j = 0; j < 7; ++j) b[j] = b[j] - back[j];
                }
            }
            valid = panda_fkcc<Grp8, EXT>(b[0], b[1], b[2], b[3], b[4], b[5], b[6], env, a.bx, a.by, a.bz);
        }
        const uint64_t bad = __builtin_amdgcn_ballot_w64(active && !valid);

        // whole segments of this pass that are valid, in order, and whether one failed
        uint32_t good;
        bool failed;
        if (n > kMaxBlocks) {
            good = 0;
            failed = true;
        } else if (pps == 1) {
            const uint32_t per = (uint32_t)(8 / n), segs = per < nseg ? per : nseg;
            const uint32_t first_bad = bad ? (uint32_t)((__builtin_ctzll(bad) >> 3) / n) : segs;
            good = first_bad < segs ? first_bad : segs;
            failed = good < segs;
        } else if (bad) {  // the wave-uniform early exit between passes
            good = 0;
            failed = true;
            jpass = 0;
        } else if (++jpass < pps) {
            continue;  // the segment's next 8 blocks
        } else {
            good = 1;
            failed = false;
            jpass = 0;
        }

        if (mode == M_INIT) {
            if (!failed) {  // a direct connection needs no search
                finished = true;
                solved = 1;
                out_len = 2;
                size0 = size1 = 1;
                if (a.path_cap >= 2) {
                    float* out = a.paths + (size_t)p * a.path_cap * 7;
                    if (lane < 7) {
                        out[lane] = start[lane];
                        out[7 + lane] = goals[(size_t)gi * 7 + lane];
                    }
                } else {
                    status = VGPU_RRTC_PATH_CAPACITY;
                }
                break;
            }
            if (++gi < a.n_goals) {
#pragma unroll
                for (int j = 0; j < 7; ++j) v[j] = goals[(size_t)gi * 7 + j] - base[j];
                n = blocks_of(l2_norm7(v));
                continue;
            }
            // rrtc.hh:76-91: the trees' roots
            push_node(t, 0, base, 0, 0, lane);
            for (uint32_t k = 0; k < a.n_goals; ++k) {
                float q[7];
                load7(goals + (size_t)k * 7, q);
                push_node(t, 1 + k, q, 1 + k, 1, lane);
            }
            n_nodes = 1 + a.n_goals;
            size0 = 1;
            size1 = a.n_goals;
            ta = a.start_tree_first ? 1u : 0u;
            mode = M_ITER;
            continue;
        }

        if (mode == M_EXT) {
            if (failed) {  // rrtc.hh:229-239
                if (a.dynamic_domain && lane == 0) {
                    const float shrunk = nr * (1.0f - a.alpha);
                    t.radius[nn] = nr == kFltMax ? a.radius0 : (shrunk < a.min_radius ? a.min_radius : shrunk);
                }
                mode = M_ITER;
                continue;
            }
            float newc[7];
#pragma unroll
            for (int j = 0; j < 7; ++j) newc[j] = base[j] + v[j];
            push_node(t, n_nodes, newc, nn, ta, lane);
            ++n_nodes;
            if (ta) ++size1; else ++size0;
            if (a.dynamic_domain && nr != kFltMax && lane == 0) t.radius[nn] = nr * (1.0f + a.alpha);  // rrtc.hh:156-159
            float od;  // extend to the other tree (rrtc.hh:161-191)
            on = nearest(t, n_nodes, ta ^ 1u, newc, lane, od);
            float oc[7];
            load7(t.nodes + (size_t)on * 7, oc);
            const float nf = __builtin_ceilf(od / a.range);  // (float)n_ext
            const float inc_len = od / nf;
            const float inv = 1.0f / nf;
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                base[j] = newc[j];
                v[j] = (oc[j] - newc[j]) * inv;
            }
            n = blocks_of(inc_len);
            nseg = nf >= 1.0f ? (nf < 2147483648.0f ? (uint32_t)nf : 0x80000000u) : 0u;
            jpass = 0;
            mode = M_CON;
            if (nseg != 0) continue;
            good = 0;  // n_ext == 0: connected without a segment
            failed = false;
        }

        // M_CON: the valid segments become nodes while there is room (rrtc.hh:186-191)
        const uint32_t room = a.max_nodes > n_nodes ? a.max_nodes - n_nodes : 0u;
        const uint32_t pushable = good < room ? good : room;
        for (uint32_t k = 0; k < pushable; ++k) {
#pragma unroll
            for (int j = 0; j < 7; ++j) base[j] = base[j] + v[j];
            push_node(t, n_nodes, base, n_nodes - 1, ta, lane);
            ++n_nodes;
            if (ta) ++size1; else ++size0;
        }
        nseg -= pushable;
        if (nseg != 0) {
            if (failed || pushable < good || n_nodes >= a.max_nodes) mode = M_ITER;
            continue;
        }

        // connected: both half-paths (rrtc.hh:193-226).  The walks are bounded by the node count.
        const uint32_t last = n_nodes - 1;
        uint32_t len_a = 1, len_b = 0;
        for (uint32_t cur = last; t.parent[cur] != cur && len_a <= n_nodes; cur = t.parent[cur]) ++len_a;
        for (uint32_t cur = on; t.parent[cur] != cur && len_b <= n_nodes; cur = t.parent[cur]) ++len_b;
        out_len = len_a + len_b;
        const bool write = out_len <= a.path_cap;
        if (!write) status = VGPU_RRTC_PATH_CAPACITY;
        float* out = a.paths + (size_t)p * a.path_cap * 7;
        const bool flip = ta != 0u;  // tree_a is the goal tree: the whole path is reversed
        float prev[7], c[7];
        load7(t.nodes + (size_t)last * 7, prev);
        uint32_t pos = len_a - 1;
        if (write && lane < 7) out[(size_t)(flip ? out_len - 1 - pos : pos) * 7 + lane] = t.nodes[(size_t)last * 7 + lane];
        for (uint32_t cur = last, k = 1; k < len_a; ++k) {
            const uint32_t q = t.parent[cur];
            load7(t.nodes + (size_t)q * 7, c);
            float d[7];
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                d[j] = c[j] - prev[j];
                prev[j] = c[j];
            }
            cost += l2_norm7(d);
            --pos;
            if (write && lane < 7) out[(size_t)(flip ? out_len - 1 - pos : pos) * 7 + lane] = t.nodes[(size_t)q * 7 + lane];
            cur = q;
        }
        load7(t.nodes + (size_t)last * 7, prev);
        pos = len_a;
        for (uint32_t cur = on, k = 0; k < len_b; ++k, ++pos) {
            const uint32_t q = t.parent[cur];
            load7(t.nodes + (size_t)q * 7, c);
            float d[7];
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                d[j] = c[j] - prev[j];
                prev[j] = c[j];
            }
            cost += l2_norm7(d);
            if (write && lane < 7) out[(size_t)(flip ? out_len - 1 - pos : pos) * 7 + lane] = t.nodes[(size_t)q * 7 + lane];
            cur = q;
        }
        finished = true;
        solved = 1;
        break;
    }

    if (lane != 0) return;
    a.rng[p] = rng;
    if (!finished) {
        ctl[RC_PHASE] = RPH_SEARCH;
        ctl[RC_NODES] = n_nodes;
        ctl[RC_SIZE0] = size0;
        ctl[RC_SIZE1] = size1;
        ctl[RC_A] = ta;
        ctl[RC_ITER_LO] = (uint32_t)iter;
        ctl[RC_ITER_HI] = (uint32_t)(iter >> 32);
        atomicAdd(totals + 0, 1ull);
        return;
    }
    ctl[RC_PHASE] = RPH_DONE;
    vgpu_plan_result r{};
    r.solved = solved;
    r.iterations = iter;
    r.nanoseconds = 0;
    r.size[0] = size0;
    r.size[1] = size1;
    r.cost = cost;
    r.path_len = out_len;
    a.results[p] = r;
    a.path_len[p] = out_len;
    if (a.status) a.status[p] = (uint8_t)status;
    atomicAdd(totals + 1, (unsigned long long)iter);
    atomicMax(totals + 2, (unsigned long long)iter);
}

// one environment for every problem: the view is a kernel argument
template <bool EXT>
__global__ __launch_bounds__(kWave) void rrtc_kernel(RrtcArgs a, EnvView env, unsigned long long* __restrict__ totals)
{
    const uint32_t p = blockIdx.x;
    uint32_t* ctl = a.ctl + (size_t)p * kRrtcWords;
    const uint32_t phase = ctl[RC_PHASE];
    if (phase == RPH_DONE) return;  // wave-uniform
    rrtc_search<EXT>(a, env, totals, p, ctl, phase);
}

// one environment per problem: wave p searches in views[env_index[p]].  The index is read through readfirstlane and
// the table lies in the constant address space, so the view's fields arrive by scalar loads into SGPRs, as the
// kernel argument's do.  An index outside the table ends the problem unrun and counts in totals[4] (the host fails
// the call), the pattern of rng == 0 on totals[3]: no view is read for it.
template <bool EXT>
__global__ __launch_bounds__(kWave) void rrtc_scenes_kernel(RrtcArgs a, const VGPU_CONST EnvView* __restrict__ views,
                                                            const uint32_t* __restrict__ env_index, uint32_t n_envs,
                                                            unsigned long long* __restrict__ totals)
{
    const uint32_t p = blockIdx.x;
    uint32_t* ctl = a.ctl + (size_t)p * kRrtcWords;
    const uint32_t phase = ctl[RC_PHASE];
    if (phase == RPH_DONE) return;  // wave-uniform
    const uint32_t e = (uint32_t)__builtin_amdgcn_readfirstlane((int)env_index[p]);
    if (e >= n_envs) {
        if (threadIdx.x == 0) {
            ctl[RC_PHASE] = RPH_DONE;
            atomicAdd(totals + 4, 1ull);
        }
        return;
    }
    static_assert(sizeof(EnvView) % 4 == 0 && alignof(EnvView) >= 4, "the view is copied word by word");
    union {
        EnvView v;
        uint32_t w[sizeof(EnvView) / 4];
    } env;
    const VGPU_CONST uint32_t* src = (const VGPU_CONST uint32_t*)(views + e);
#pragma unroll
    for (size_t i = 0; i < sizeof(EnvView) / 4; ++i) env.w[i] = src[i];
    rrtc_search<EXT>(a, env.v, totals, p, ctl, phase);
}

// the launch's counters to the pinned words the host reads after its synchronisation
__global__ void rrtc_report_kernel(unsigned long long* __restrict__ totals, unsigned long long* __restrict__ host)
{
    host[0] = totals[0];
    host[1] = totals[1];
    host[2] = totals[2];
    host[3] = totals[3];
    host[4] = totals[4];
    totals[0] = 0;
}

}  // namespace vgpu

extern "C" hipError_t vgpu_launch_rrtc(const vgpu::RrtcArgs* a, const EnvView* env, unsigned long long* totals,
                                       unsigned long long* host_totals, hipStream_t st)
{
    if (env->n_hf > 0 || env->n_pc > 0)
        hipLaunchKernelGGL(vgpu::rrtc_kernel<true>, dim3(a->P), dim3(vgpu::kWave), 0, st, *a, *env, totals);
    else
        hipLaunchKernelGGL(vgpu::rrtc_kernel<false>, dim3(a->P), dim3(vgpu::kWave), 0, st, *a, *env, totals);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(vgpu::rrtc_report_kernel, dim3(1), dim3(1), 0, st, totals, host_totals);
    return hipGetLastError();
}

extern "C" hipError_t vgpu_launch_rrtc_scenes(const vgpu::RrtcArgs* a, const EnvView* views, const uint32_t* env_index,
                                              uint32_t n_envs, int ext, unsigned long long* totals,
                                              unsigned long long* host_totals, hipStream_t st)
{
    const VGPU_CONST EnvView* v = (const VGPU_CONST EnvView*)views;
    if (ext)
        hipLaunchKernelGGL(vgpu::rrtc_scenes_kernel<true>, dim3(a->P), dim3(vgpu::kWave), 0, st, *a, v, env_index, n_envs,
                           totals);
    else
        hipLaunchKernelGGL(vgpu::rrtc_scenes_kernel<false>, dim3(a->P), dim3(vgpu::kWave), 0, st, *a, v, env_index, n_envs,
                           totals);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(vgpu::rrtc_report_kernel, dim3(1), dim3(1), 0, st, totals, host_totals);
    return hipGetLastError();
}
