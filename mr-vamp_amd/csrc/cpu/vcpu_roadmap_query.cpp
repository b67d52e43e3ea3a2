// vcpu_roadmap_query.cpp -- the roadmap queries of vgpu_roadmap_query.hip on the host CPU: the bench's CPU
// baseline and the second implementation the GPU results are pinned to (include/vamp_gpu.h, "roadmap queries").
//   sssp        a binary-heap Dijkstra in float arithmetic per search (g = the least fixed point of
//               g[v] = min_u fl32(g[u] + w(u, v)): float addition is monotone, so a vertex popped with the
//               smallest tentative g is final), then a BFS over the tight edges for hops, then the parent rule
//               (smallest tight predecessor one BFS level up).
//   bottleneck  vertices enter in index order into a union-find whose sets keep their members in a circular list;
//               a set that joins the source's set at vertex k gets b = k.  The adjacency is taken as symmetric
//               (a roadmap's is).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <queue>
#include <utility>
#include <vector>

#include "../../../include/vamp_gpu.h"
#include "../vgpu_abi.hh"

namespace vcpu {

static inline uint32_t fbits(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

// offsets monotone from 0, slot indices < n, and (w given) weights >= 0 or +inf, none NaN
int roadmap_graph_check(size_t n, const uint64_t* offsets, const uint32_t* adj, const float* w)
{
    if (n >= ((size_t)1 << 31)) return VGPU_ERR_INVALID_ARG;
    if (n == 0) return VGPU_OK;
    if (!offsets || offsets[0] != 0) return VGPU_ERR_INVALID_ARG;
    for (size_t v = 0; v < n; ++v)
        if (offsets[v + 1] < offsets[v]) return VGPU_ERR_INVALID_ARG;
    const uint64_t e = offsets[n];
    if (e >= ((uint64_t)1 << 32) || (e && !adj)) return VGPU_ERR_INVALID_ARG;
    for (uint64_t k = 0; k < e; ++k) {
        if (adj[k] >= n) return VGPU_ERR_INVALID_ARG;
        if (w && !(w[k] >= 0.0f)) return VGPU_ERR_INVALID_ARG;  // negative or NaN
    }
    return VGPU_OK;
}

static void sssp_one(size_t n, const uint64_t* off, const uint32_t* adj, const float* w, uint32_t src, uint32_t lim,
                     float* g, uint32_t* hops, uint32_t* parent)
{
    const float inf = INFINITY;
    for (size_t v = 0; v < n; ++v) g[v] = inf;
    g[src] = 0.0f;
    using Item = std::pair<float, uint32_t>;
    std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
    heap.emplace(0.0f, src);
    while (!heap.empty()) {
        const Item it = heap.top();
        heap.pop();
        const uint32_t u = it.second;
        if (it.first != g[u]) continue;  // a stale entry
        for (uint64_t e = off[u]; e < off[u + 1]; ++e) {
            const uint32_t t = adj[e];
            if (t > lim) continue;
            const float cand = g[u] + w[e];
            if (cand < g[t]) {
                g[t] = cand;
                heap.emplace(cand, t);
            }
        }
    }
    if (!hops) return;
    for (size_t v = 0; v < n; ++v) hops[v] = parent[v] = UINT32_MAX;
    hops[src] = 0;
    parent[src] = src;
    std::vector<uint32_t> cur{src}, next;
    for (uint32_t d = 0; !cur.empty(); ++d) {
        next.clear();
        for (uint32_t u : cur)
            for (uint64_t e = off[u]; e < off[u + 1]; ++e) {
                const uint32_t t = adj[e];
                if (t > lim) continue;
                const float cand = g[u] + w[e];
                if (!(cand < inf) || fbits(cand) != fbits(g[t]) || hops[t] < d + 1) continue;
                if (hops[t] == UINT32_MAX) {
                    hops[t] = d + 1;
                    next.push_back(t);
                }
                if (u < parent[t]) parent[t] = u;
            }
        cur.swap(next);
    }
}

static uint32_t find(std::vector<uint32_t>& up, uint32_t a)
{
    while (up[a] != a) {
        up[a] = up[up[a]];
        a = up[a];
    }
    return a;
}

static void bottleneck_one(size_t n, const uint64_t* off, const uint32_t* adj, uint32_t src, uint32_t* b)
{
    for (size_t v = 0; v < n; ++v) b[v] = UINT32_MAX;
    std::vector<uint32_t> up(n), ring(n);  // ring: the next member of the vertex's set
    for (uint32_t k = 0; k < n; ++k) {
        up[k] = ring[k] = k;
        if (k == src) b[k] = k;
        for (uint64_t e = off[k]; e < off[k + 1]; ++e) {
            const uint32_t j = adj[e];
            if (j >= k) continue;  // the later endpoint joins the edge
            uint32_t a = find(up, k), c = find(up, j);
            if (a == c) continue;
            if (k >= src) {  // a set meeting the source's set is reached at k
                const uint32_t rs = find(up, src);
                const uint32_t other = a == rs ? c : (c == rs ? a : UINT32_MAX);
                if (other != UINT32_MAX) {
                    uint32_t m = other;
                    do {
                        b[m] = k;
                        m = ring[m];
                    } while (m != other);
                }
            }
            up[c] = a;
            std::swap(ring[a], ring[c]);
        }
    }
}

}  // namespace vcpu

extern "C" int vgpu_cpu_roadmap_sssp(size_t n, const uint64_t* offsets, const uint32_t* adj, const float* w,
                                     const uint32_t* sources, const uint32_t* limits, size_t S, float* g,
                                     uint32_t* hops, uint32_t* parent)
try {
    if ((hops == nullptr) != (parent == nullptr)) return VGPU_ERR_INVALID_ARG;
    if (S == 0) return VGPU_OK;
    if (!sources || !g || n == 0) return VGPU_ERR_INVALID_ARG;
    if (!w && offsets && offsets[n]) return VGPU_ERR_INVALID_ARG;
    int rc = vcpu::roadmap_graph_check(n, offsets, adj, w);
    if (rc) return rc;
    if (S * n >= ((uint64_t)1 << 32)) return VGPU_ERR_INVALID_ARG;
    for (size_t s = 0; s < S; ++s)
        if (sources[s] >= n || (limits && sources[s] > limits[s])) return VGPU_ERR_INVALID_ARG;
    for (size_t s = 0; s < S; ++s)
        vcpu::sssp_one(n, offsets, adj, w, sources[s], limits ? limits[s] : UINT32_MAX, g + s * n,
                       hops ? hops + s * n : nullptr, parent ? parent + s * n : nullptr);
    return VGPU_OK;
} VGPU_ABI_CATCH

extern "C" int vgpu_cpu_roadmap_bottleneck(size_t n, const uint64_t* offsets, const uint32_t* adj,
                                           const uint32_t* sources, size_t S, uint32_t* b)
try {
    if (S == 0) return VGPU_OK;
    if (!sources || !b || n == 0) return VGPU_ERR_INVALID_ARG;
    int rc = vcpu::roadmap_graph_check(n, offsets, adj, nullptr);
    if (rc) return rc;
    if (S * n >= ((uint64_t)1 << 32)) return VGPU_ERR_INVALID_ARG;
    for (size_t s = 0; s < S; ++s)
        if (sources[s] >= n) return VGPU_ERR_INVALID_ARG;
    for (size_t s = 0; s < S; ++s) vcpu::bottleneck_one(n, offsets, adj, sources[s], b + s * n);
    return VGPU_OK;
} VGPU_ABI_CATCH
