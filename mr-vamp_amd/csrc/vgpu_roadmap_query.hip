// vgpu_roadmap_query.hip -- queries over a built roadmap (CSR adjacency in HBM): PRM::solve's search half
// (planning/prm.hh:168-187, utils.hh:75-142) for S (source, prefix limit) pairs in lockstep.
//
// One frontier engine, two semirings:
//   sssp        val = bits of g (float >= 0: the bit patterns order as the values, so a 32-bit atomicMin is
//               exact), candidate = fl32(g[u] + w(u, t));
//   bottleneck  val = the smallest possible largest vertex index of a path, candidate = max(b[u], t).
// A round is ONE launch over the items (search, vertex) whose value fell in the round before: one wave per
// item, lanes striding its adjacency slots, atomicMin into the neighbours.  A neighbour whose value falls is
// appended to the next frontier once: stamp[item] holds the last round the item was appended for, and the lane
// whose atomicMax raises it appends.  The host reads the next frontier's size after every round (no grid-wide
// barrier, no wait between blocks) and stops at 0; a value can fall only along a path with more edges than
// rounds done, so rounds <= n, and the host gives up with an error past n + 1.
//
// The fixed point is unique (float addition is monotone), so g does not depend on the order of the atomics.
// Parents do NOT come out of the relaxation: an attempt made from a predecessor's transient g would survive in
// any packed (g, parent) word.  They come from the final g alone: a level-synchronous BFS from the source over
// the TIGHT edges (bits(fl32(g[u] + w)) == bits(g[t]), g[t] finite) gives hops, and every frontier vertex u of
// level d with a tight edge into a vertex t of level d + 1 offers itself by atomicMin(parent[t], u) -- the
// set of offers is fixed by g and hops, so the minimum is too.  Zero-length edges and absorbed additions
// (fl(g + w) == g) make plateaus where "a predecessor achieving g" could cycle; BFS levels cannot.
#include <algorithm>

#include "../../include/vamp_gpu.h"
#include "vgpu_roadmap_query.hh"

namespace vgpu {
namespace rq {

constexpr uint32_t kInfBits = 0x7f800000u;
constexpr unsigned kBlock = 256, kWavesPerBlock = kBlock / 64, kMaxBlocks = 4096;

__global__ __launch_bounds__(256) void fill_kernel(uint32_t* __restrict__ p, uint32_t value, size_t count)
{
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += (size_t)gridDim.x * kBlock)
        p[i] = value;
}

// bad[0] |= 1 on a structural error (offsets not monotone from 0 within E slots, a slot index >= n), |= 2 on a
// negative or NaN weight
__global__ __launch_bounds__(256) void check_kernel(uint32_t n, const unsigned long long* __restrict__ off,
                                                    const uint32_t* __restrict__ adj, const float* __restrict__ w,
                                                    unsigned long long E, uint32_t* __restrict__ bad)
{
    const size_t stride = (size_t)gridDim.x * kBlock, first = (size_t)blockIdx.x * kBlock + threadIdx.x;
    for (size_t v = first; v < n; v += stride)
        if (off[v] > off[v + 1] || off[v + 1] > E || (v == 0 && off[0] != 0)) atomicOr(bad, 1u);
    for (size_t e = first; e < E; e += stride) {
        if (adj[e] >= n) atomicOr(bad, 1u);
        if (w && !(w[e] >= 0.0f)) atomicOr(bad, 2u);
    }
}

// search s: its source gets the semiring's one (g = 0 / b = source) and is the first frontier item;
// bad[0] |= 4 for a source >= n or above its limit (nothing is written for it)
template <bool SSSP>
__global__ __launch_bounds__(256) void seed_kernel(uint32_t n, const uint32_t* __restrict__ sources,
                                                   const uint32_t* __restrict__ limits, uint32_t S,
                                                   uint32_t* __restrict__ val, uint32_t* __restrict__ stamp,
                                                   uint32_t* __restrict__ frontier, uint32_t* __restrict__ bad)
{
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= S) return;
    const uint32_t src = sources[s];
    if (src >= n || (limits && src > limits[s])) {
        atomicOr(bad, 4u);
        frontier[s] = s * n;  // in bounds; the call fails before any round runs
        return;
    }
    const uint32_t idx = s * n + src;
    val[idx] = SSSP ? 0u : src;
    stamp[idx] = 1u;
    frontier[s] = idx;
}

// the lanes with `take` set append `item` to out[]: one atomicAdd per wave
__device__ __forceinline__ void wave_append(bool take, uint32_t item, uint32_t* __restrict__ out,
                                            uint32_t* __restrict__ out_count)
{
    const unsigned long long mask = __ballot(take);
    if (mask == 0) return;
    const uint32_t lane = threadIdx.x & 63u;
    const int leader = __ffsll((long long)mask) - 1;
    uint32_t base = 0;
    if ((int)lane == leader) base = atomicAdd(out_count, (uint32_t)__popcll(mask));
    base = __shfl(base, leader, 64);
    if (take) out[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = item;
}

// One relaxation round (round >= 1): items cur[0 .. count) were stamped `round`.  A value read here may already
// be below the one the item was appended for; whoever lowered it appended the item for round + 1 as well.
template <bool SSSP>
__global__ __launch_bounds__(256) void relax_kernel(uint32_t n, const unsigned long long* __restrict__ off,
                                                    const uint32_t* __restrict__ adj, const float* __restrict__ w,
                                                    const uint32_t* __restrict__ limits, uint32_t* val,
                                                    uint32_t* stamp, const uint32_t* __restrict__ cur, uint32_t count,
                                                    uint32_t* __restrict__ next, uint32_t* __restrict__ next_count,
                                                    uint32_t round, unsigned long long* __restrict__ slots)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * kBlock + threadIdx.x) >> 6, waves = (gridDim.x * kBlock) >> 6;
    unsigned long long relaxed = 0;
    for (uint32_t it = wave; it < count; it += waves) {
        const uint32_t idx = cur[it];
        const uint32_t s = idx / n, v = idx - s * n;
        const uint32_t lim = limits ? limits[s] : 0xffffffffu;
        const uint32_t mine = val[idx];
        const unsigned long long lo = off[v], hi = off[v + 1];
        uint32_t* row = val + (size_t)s * n;
        uint32_t* srow = stamp + (size_t)s * n;
        relaxed += hi - lo;
        for (unsigned long long base = lo; base < hi; base += 64) {  // uniform trip count: the ballots below
            const unsigned long long e = base + lane;
            bool fell = false;
            uint32_t t = 0;
            if (e < hi) {
                t = adj[e];
                if (t <= lim) {
                    // +inf weights and overflowing sums give +inf's bits, which are below no value
                    const uint32_t cand = SSSP ? __float_as_uint(__uint_as_float(mine) + w[e]) : (mine > t ? mine : t);
                    // the plain read may be stale, but never below the truth: it only saves atomics
                    if (cand < row[t] && atomicMin(&row[t], cand) > cand) fell = atomicMax(&srow[t], round + 1u) <= round;
                }
            }
            wave_append(fell, s * n + t, next, next_count);
        }
    }
    if (lane == 0 && relaxed) atomicAdd(slots, relaxed);
}

// One level of the BFS over tight edges: items cur[0 .. count) have hops == d.
__global__ __launch_bounds__(256) void tight_kernel(uint32_t n, const unsigned long long* __restrict__ off,
                                                    const uint32_t* __restrict__ adj, const float* __restrict__ w,
                                                    const uint32_t* __restrict__ limits, const uint32_t* __restrict__ g,
                                                    uint32_t* hops, uint32_t* parent, const uint32_t* __restrict__ cur,
                                                    uint32_t count, uint32_t* __restrict__ next,
                                                    uint32_t* __restrict__ next_count, uint32_t d)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * kBlock + threadIdx.x) >> 6, waves = (gridDim.x * kBlock) >> 6;
    for (uint32_t it = wave; it < count; it += waves) {
        const uint32_t idx = cur[it];
        const uint32_t s = idx / n, u = idx - s * n;
        const uint32_t lim = limits ? limits[s] : 0xffffffffu;
        const float gu = __uint_as_float(g[idx]);
        const unsigned long long lo = off[u], hi = off[u + 1];
        const uint32_t* grow = g + (size_t)s * n;
        uint32_t* hrow = hops + (size_t)s * n;
        uint32_t* prow = parent + (size_t)s * n;
        for (unsigned long long base = lo; base < hi; base += 64) {
            const unsigned long long e = base + lane;
            bool first = false;
            uint32_t t = 0;
            if (e < hi) {
                t = adj[e];
                if (t <= lim) {
                    const uint32_t cand = __float_as_uint(gu + w[e]);
                    // hops only falls, from UINT32_MAX to its level: a stale read is never below the truth
                    if (cand < kInfBits && cand == grow[t] && hrow[t] > d) {
                        const uint32_t h = atomicMin(&hrow[t], d + 1u);
                        if (h > d) {  // t is on level d + 1: u is one of its candidates
                            atomicMin(&prow[t], u);
                            first = h == 0xffffffffu;
                        }
                    }
                }
            }
            wave_append(first, s * n + t, next, next_count);
        }
    }
}

// hops[s][src] = 0, parent[s][src] = src; the BFS frontier restarts from the sources
__global__ __launch_bounds__(256) void tight_seed_kernel(uint32_t n, const uint32_t* __restrict__ sources, uint32_t S,
                                                         uint32_t* __restrict__ hops, uint32_t* __restrict__ parent,
                                                         uint32_t* __restrict__ frontier)
{
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= S) return;
    const uint32_t src = sources[s], idx = s * n + src;  // checked by seed_kernel
    hops[idx] = 0u;
    parent[idx] = src;
    frontier[s] = idx;
}

// one lane per search: count the walk target -> source (at most min(cap, n) vertices), then write it reversed
__global__ __launch_bounds__(256) void extract_kernel(const uint32_t* __restrict__ parent, uint32_t n,
                                                      const uint32_t* __restrict__ targets, uint32_t S, uint32_t cap,
                                                      uint32_t* __restrict__ idx, uint32_t* __restrict__ len)
{
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= S) return;
    const uint32_t* p = parent + (size_t)s * n;
    const uint32_t target = targets[s];
    if (target >= n || p[target] == 0xffffffffu) {
        len[s] = 0u;
        return;
    }
    const uint32_t most = cap < n ? cap : n;
    uint32_t L = 1, v = target;
    while (true) {
        const uint32_t up = p[v];
        if (up == v) break;
        if (up >= n || L >= most) {  // a broken chain, or more vertices than fit
            len[s] = 0xffffffffu;
            return;
        }
        v = up;
        ++L;
    }
    if (L > cap) {  // cap == 0
        len[s] = 0xffffffffu;
        return;
    }
    uint32_t* out = idx + (size_t)s * cap;
    v = target;
    for (uint32_t k = L; k-- > 0;) {
        out[k] = v;
        v = p[v];
    }
    len[s] = L;
}

static unsigned blocks_for_items(uint32_t count)
{
    return std::min<unsigned>(kMaxBlocks, (count + kWavesPerBlock - 1) / kWavesPerBlock);
}

static unsigned blocks_for(size_t count)
{
    return (unsigned)std::min<size_t>(kMaxBlocks, std::max<size_t>(1, (count + kBlock - 1) / kBlock));
}

static size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }

#define RQ_HIP(expr)                                        \
    do {                                                    \
        hipError_t e_ = (expr);                             \
        if (e_ != hipSuccess) return QueryStatus{VGPU_ERR_HIP, e_, #expr}; \
    } while (0)

struct Work {
    uint32_t *stamp, *front[2], *count, *bad;
    unsigned long long* slots;
};

static QueryStatus prepare(QueryState& q, size_t items, Work* k, hipStream_t st)
{
    const size_t ib = al256(items * 4), need = 3 * ib + 256;
    if (need > q.dev_bytes) {
        if (q.dev) {
            RQ_HIP(hipStreamSynchronize(st));
            RQ_HIP(hipFree(q.dev));
            q.dev = nullptr;
            q.dev_bytes = 0;
        }
        RQ_HIP(hipMalloc(&q.dev, need));
        q.dev_bytes = need;
    }
    if (!q.host) RQ_HIP(hipHostMalloc((void**)&q.host, 4 * sizeof(uint32_t), hipHostMallocDefault));
    char* p = (char*)q.dev;
    k->stamp = (uint32_t*)p;
    k->front[0] = (uint32_t*)(p + ib);
    k->front[1] = (uint32_t*)(p + 2 * ib);
    k->slots = (unsigned long long*)(p + 3 * ib);
    k->count = (uint32_t*)(p + 3 * ib + 8);
    k->bad = (uint32_t*)(p + 3 * ib + 12);
    return QueryStatus{};
}

// the frontier loop of one semiring; val [S][n] is the output buffer itself
template <bool SSSP>
static QueryStatus run(QueryState& q, uint32_t n, const unsigned long long* off, const uint32_t* adj, const float* w,
                       const uint32_t* sources, const uint32_t* limits, uint32_t S, uint32_t* val, uint32_t* hops,
                       uint32_t* parent, hipStream_t st)
{
    for (auto& x : q.stats) x = 0;
    const size_t items = (size_t)S * n;
    Work k;
    QueryStatus rc = prepare(q, items, &k, st);
    if (rc.code) return rc;
    // the slot count, then the checks: no round runs over a graph that would send it out of bounds
    unsigned long long E = 0;
    RQ_HIP(hipMemcpyAsync(&E, off + n, sizeof(E), hipMemcpyDeviceToHost, st));
    RQ_HIP(hipStreamSynchronize(st));
    q.stats[3] += 1;
    if (E >= (1ull << 32)) return QueryStatus{VGPU_ERR_INVALID_ARG, hipSuccess, "offsets[n] must be below 2^32"};
    RQ_HIP(hipMemsetAsync(k.slots, 0, 16, st));  // slots, count, bad
    hipLaunchKernelGGL(check_kernel, dim3(blocks_for(std::max<size_t>(n, E))), dim3(kBlock), 0, st, n, off, adj, w, E,
                       k.bad);
    hipLaunchKernelGGL(fill_kernel, dim3(blocks_for(items)), dim3(kBlock), 0, st, val, SSSP ? kInfBits : 0xffffffffu,
                       items);
    RQ_HIP(hipMemsetAsync(k.stamp, 0, items * 4, st));
    hipLaunchKernelGGL(seed_kernel<SSSP>, dim3((S + kBlock - 1) / kBlock), dim3(kBlock), 0, st, n, sources, limits, S,
                       val, k.stamp, k.front[0], k.bad);
    RQ_HIP(hipGetLastError());
    RQ_HIP(hipMemcpyAsync(q.host, k.bad, 4, hipMemcpyDeviceToHost, st));
    RQ_HIP(hipStreamSynchronize(st));
    q.stats[3] += 1;
    const uint32_t bad = q.host[0];
    if (bad & 1u) return QueryStatus{VGPU_ERR_INVALID_ARG, hipSuccess, "graph: offsets not monotone or a slot index >= n"};
    if (bad & 2u) return QueryStatus{VGPU_ERR_INVALID_ARG, hipSuccess, "a negative or NaN edge weight"};
    if (bad & 4u) return QueryStatus{VGPU_ERR_INVALID_ARG, hipSuccess, "a source >= n or above its limit"};

    uint32_t count = S;
    int cur = 0;
    for (uint32_t round = 1; count; ++round) {
        if (round > n + 1u) return QueryStatus{VGPU_ERR_INTERNAL, hipSuccess, "relaxation did not converge in n + 1 rounds"};
        RQ_HIP(hipMemsetAsync(k.count, 0, 4, st));
        hipLaunchKernelGGL(relax_kernel<SSSP>, dim3(blocks_for_items(count)), dim3(kBlock), 0, st, n, off, adj, w, limits,
                           val, k.stamp, k.front[cur], count, k.front[cur ^ 1], k.count, round, k.slots);
        RQ_HIP(hipGetLastError());
        RQ_HIP(hipMemcpyAsync(q.host, k.count, 4, hipMemcpyDeviceToHost, st));
        RQ_HIP(hipStreamSynchronize(st));
        q.stats[0] += 1;
        q.stats[2] += count;
        q.stats[3] += 1;
        count = q.host[0];
        if (count > items) return QueryStatus{VGPU_ERR_INTERNAL, hipSuccess, "a frontier exceeds its workspace"};
        cur ^= 1;
    }
    unsigned long long slots = 0;
    RQ_HIP(hipMemcpyAsync(&slots, k.slots, sizeof(slots), hipMemcpyDeviceToHost, st));
    RQ_HIP(hipStreamSynchronize(st));
    q.stats[1] = slots;
    q.stats[3] += 1;
    if (!SSSP || !hops) return QueryStatus{};

    hipLaunchKernelGGL(fill_kernel, dim3(blocks_for(items)), dim3(kBlock), 0, st, hops, 0xffffffffu, items);
    hipLaunchKernelGGL(fill_kernel, dim3(blocks_for(items)), dim3(kBlock), 0, st, parent, 0xffffffffu, items);
    hipLaunchKernelGGL(tight_seed_kernel, dim3((S + kBlock - 1) / kBlock), dim3(kBlock), 0, st, n, sources, S, hops,
                       parent, k.front[0]);
    RQ_HIP(hipGetLastError());
    count = S;
    cur = 0;
    for (uint32_t d = 0; count; ++d) {
        if (d > n) return QueryStatus{VGPU_ERR_INTERNAL, hipSuccess, "tight-edge BFS deeper than n levels"};
        RQ_HIP(hipMemsetAsync(k.count, 0, 4, st));
        hipLaunchKernelGGL(tight_kernel, dim3(blocks_for_items(count)), dim3(kBlock), 0, st, n, off, adj, w, limits, val,
                           hops, parent, k.front[cur], count, k.front[cur ^ 1], k.count, d);
        RQ_HIP(hipGetLastError());
        RQ_HIP(hipMemcpyAsync(q.host, k.count, 4, hipMemcpyDeviceToHost, st));
        RQ_HIP(hipStreamSynchronize(st));
        q.stats[3] += 1;
        count = q.host[0];
        if (count > items) return QueryStatus{VGPU_ERR_INTERNAL, hipSuccess, "a frontier exceeds its workspace"};
        cur ^= 1;
    }
    return QueryStatus{};
}

}  // namespace rq

QueryStatus query_sssp(QueryState& q, uint32_t n, const unsigned long long* offsets, const uint32_t* adj,
                       const float* w, const uint32_t* sources, const uint32_t* limits, uint32_t S, float* g,
                       uint32_t* hops, uint32_t* parent, hipStream_t st)
{
    return rq::run<true>(q, n, offsets, adj, w, sources, limits, S, (uint32_t*)g, hops, parent, st);
}

QueryStatus query_bottleneck(QueryState& q, uint32_t n, const unsigned long long* offsets, const uint32_t* adj,
                             const uint32_t* sources, uint32_t S, uint32_t* b, hipStream_t st)
{
    return rq::run<false>(q, n, offsets, adj, nullptr, sources, nullptr, S, b, nullptr, nullptr, st);
}

QueryStatus query_extract(const uint32_t* parent, uint32_t n, const uint32_t* targets, uint32_t S, uint32_t cap,
                          uint32_t* idx, uint32_t* len, hipStream_t st)
{
    using namespace rq;
    hipLaunchKernelGGL(extract_kernel, dim3((S + kBlock - 1) / kBlock), dim3(kBlock), 0, st, parent, n, targets, S, cap,
                       idx, len);
    RQ_HIP(hipGetLastError());
    RQ_HIP(hipStreamSynchronize(st));
    return QueryStatus{};
}

void query_free(QueryState& q)
{
    if (q.dev) (void)hipFree(q.dev);
    if (q.host) (void)hipHostFree(q.host);
    q.dev = nullptr;
    q.host = nullptr;
    q.dev_bytes = 0;
}

}  // namespace vgpu
