"""Plain-Python restatement of the roadmap queries (include/vamp_gpu.h, "roadmap queries") and of the
reference's PRM::solve loop with its astar (planning/prm.hh:43-196, planning/utils.hh:75-142), plus the synthetic
CSR graphs the CPU and GPU tests share.  Nothing here calls the library under test.

  sssp          Dijkstra with np.float32 adds (g = least fixed point of g[v] = min_u fl32(g[u] + w(u, v))), the
                BFS over tight edges (hops) and the parent rule (smallest tight predecessor one level up, found
                per vertex over its in-edges, not by the order of a traversal).
  bottleneck    union-find over the vertices in index order: b[v] = the vertex at whose insertion v first
                shares the source's component.
  prm_solve     the reference's solve loop over the oracle's build_roadmap_edges (whose dist supplies the
                weights): neighbour appends in query order, component merging, astar at the first connection.
"""
import heapq

import numpy as np

F = np.float32
U32_MAX = 0xffffffff
INF = F(np.inf)


def bits(x):
    return np.asarray(x, F).view(np.uint32)


# ---- graphs ---------------------------------------------------------------------------------------------------
def csr(n, edges, directed=False):
    """CSR of a list of (u, v, w): each edge gives slot u -> v and, unless directed, slot v -> u with the same
    weight (a self-loop gives one slot); slots keep the order of the list.  Returns (offsets uint64 [n+1],
    adj uint32, w float32)."""
    lists = [[] for _ in range(n)]
    for u, v, wt in edges:
        lists[u].append((v, wt))
        if not directed and u != v:
            lists[v].append((u, wt))
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(l) for l in lists])
    adj = np.array([v for l in lists for v, _ in l], np.uint32)
    w = np.array([wt for l in lists for _, wt in l], F)
    return off, adj, w


def path_graph(n=2000, seed=5):
    """0 - 1 - ... - n-1 with random weights: as many rounds as vertices"""
    rng = np.random.default_rng(seed)
    wt = rng.random(n - 1, dtype=F) + F(0.01)
    return csr(n, [(i, i + 1, wt[i]) for i in range(n - 1)])


def hub_graph(degree=5000, chain=2, seed=6):
    """vertex 0 with `degree` spokes, each continuing as a chain of `chain` more vertices: one vertex far
    wider than a wave"""
    rng = np.random.default_rng(seed)
    edges, nxt = [], 1
    for _ in range(degree):
        prev = 0
        for _ in range(chain + 1):
            edges.append((prev, nxt, F(rng.random(dtype=F) + F(0.05))))
            prev, nxt = nxt, nxt + 1
    return csr(nxt, edges)


def plateau_graph():
    """0 -1.5- 1, a zero-weight triangle 1 2 3, 4 a duplicate of 3 (zero edge) that is also a duplicate of 5:
    every vertex of the plateau has g = 1.5 and only BFS levels order them"""
    return csr(7, [(0, 1, F(1.5)), (1, 2, F(0)), (2, 3, F(0)), (3, 1, F(0)), (3, 4, F(0)), (4, 5, F(0)), (5, 6, F(2))])


def absorption_graph():
    """a 2^24 edge, then 0.5 edges that float addition absorbs (fl(2^24 + 0.5) == 2^24), then a 2.0 edge that it
    does not, and a cycle among the absorbed vertices"""
    big = F(2.0 ** 24)
    return csr(7, [(0, 1, big), (1, 2, F(0.5)), (2, 3, F(0.5)), (3, 4, F(0.5)), (4, 2, F(0.5)), (3, 5, F(2)),
                   (1, 5, F(2.5)), (5, 6, F(1))])


def equal_cost_graph():
    """0 -> 1: direct 2.0, 1 + 1 through 2, 0.5 x 4 through 3 4 5 (the direct edge wins: fewest waypoints);
    0 -> 8 by two 2-hop routes through 7 and through 6 (the smaller predecessor, 6, wins)"""
    h = F(0.5)
    return csr(9, [(0, 3, h), (3, 4, h), (4, 5, h), (5, 1, h), (0, 2, F(1)), (2, 1, F(1)), (0, 1, F(2)),
                   (0, 7, F(1)), (7, 8, F(2)), (0, 6, F(2)), (6, 8, F(1))])


def disconnected_graph():
    """two components and an isolated vertex 6"""
    return csr(7, [(0, 1, F(1)), (1, 2, F(2)), (3, 4, F(1)), (4, 5, F(1))])


def loops_graph():
    """self-loops, a repeated slot with two different weights, and a +inf edge that must be ignored (4 is reached
    the long way, 5 only through the +inf edge: unreachable)"""
    return csr(6, [(0, 0, F(0)), (0, 1, F(3)), (0, 1, F(1)), (1, 1, F(0.5)), (1, 2, F(1)), (2, 2, F(1)),
                   (0, 4, INF), (2, 3, F(1)), (3, 4, F(1)), (4, 5, INF)])


def limit_graph():
    """0 - 5 - 1 is the short route (2.0), 0 - 2 - 3 - 1 the long one (6.0): a limit below 5 cuts the short one"""
    return csr(6, [(0, 5, F(1)), (5, 1, F(1)), (0, 2, F(2)), (2, 3, F(2)), (3, 1, F(2)), (4, 0, F(9))])


def random_graph(n=20000, partners=8, seed=7):
    """every vertex draws `partners` random partners (an undirected edge each), weights from {1, 2, 3} with
    probabilities 0.5, 0.3, 0.2: small integers make equal-cost routes, so most vertices have several tight
    predecessors (with 4 partners per vertex, or uniform weights, only about a third of them do)"""
    rng = np.random.default_rng(seed)
    u = np.repeat(np.arange(n), partners)
    v = rng.integers(0, n, len(u))
    wt = rng.choice(np.array([1, 2, 3], F), len(u), p=(0.5, 0.3, 0.2))
    return csr(n, list(zip(u.tolist(), v.tolist(), wt)))


SMALL = {"plateau": plateau_graph, "absorption": absorption_graph, "equal_cost": equal_cost_graph,
         "disconnected": disconnected_graph, "loops": loops_graph, "limit": limit_graph}


# ---- the queries ------------------------------------------------------------------------------------------------
def sssp(off, adj, w, src, limit=None):
    """(g float32 [n], hops uint32 [n], parent uint32 [n]) of one search"""
    n = len(off) - 1
    lim = n if limit is None else int(limit)
    off = [int(o) for o in off]
    adj = [int(a) for a in adj]
    w = np.asarray(w, F)
    g = np.full(n, INF, F)
    g[src] = F(0)
    heap = [(0.0, src)]
    while heap:
        gu, u = heapq.heappop(heap)
        if F(gu) != g[u]:
            continue
        for e in range(off[u], off[u + 1]):
            t = adj[e]
            if t > lim:
                continue
            cand = F(g[u] + w[e])
            if cand < g[t]:
                g[t] = cand
                heapq.heappush(heap, (float(cand), t))
    gb = g.view(np.uint32)
    tight_in = [[] for _ in range(n)]  # tight_in[v] = the u with a tight edge u -> v
    for u in range(n):
        if not g[u] < INF:
            continue
        for e in range(off[u], off[u + 1]):
            t = adj[e]
            if t > lim:
                continue
            cand = F(g[u] + w[e])
            if cand < INF and cand.view(np.uint32) == gb[t]:
                tight_in[t].append(u)
    tight_out = [[] for _ in range(n)]
    for v in range(n):
        for u in tight_in[v]:
            tight_out[u].append(v)
    hops = np.full(n, U32_MAX, np.uint32)
    hops[src] = 0
    level, d = [src], 0
    while level:
        nxt = []
        for u in level:
            for v in tight_out[u]:
                if hops[v] == U32_MAX:
                    hops[v] = d + 1
                    nxt.append(v)
        level, d = nxt, d + 1
    parent = np.full(n, U32_MAX, np.uint32)
    parent[src] = src
    for v in range(n):
        if v != src and hops[v] != U32_MAX:
            parent[v] = min(u for u in tight_in[v] if hops[u] != U32_MAX and int(hops[u]) == int(hops[v]) - 1)
    return g, hops, parent


def tight_predecessors(off, adj, w, g, limit=None):
    """per vertex, how many distinct u have a tight edge into it (vectorised; g from any implementation)"""
    n = len(off) - 1
    deg = np.diff(np.asarray(off).astype(np.int64))
    u = np.repeat(np.arange(n), deg)
    t = np.asarray(adj).astype(np.int64)[:len(u)]
    cand = (np.asarray(g, F)[u] + np.asarray(w, F)[:len(u)]).astype(F)
    ok = (cand < INF) & (cand.view(np.uint32) == np.asarray(g, F)[t].view(np.uint32)) & (t != u)
    if limit is not None:
        ok &= (t <= limit) & (u <= limit)
    pairs = np.unique(np.stack([t[ok], u[ok]], 1), axis=0)
    return np.bincount(pairs[:, 0], minlength=n)


def bottleneck(off, adj, src):
    """b uint32 [n]: union-find in index order with member lists (symmetric adjacency)"""
    n = len(off) - 1
    off = [int(o) for o in off]
    adj = [int(a) for a in adj]
    b = np.full(n, U32_MAX, np.uint32)
    root = list(range(n))
    members = [[v] for v in range(n)]

    def find(a):
        while root[a] != a:
            root[a] = root[root[a]]
            a = root[a]
        return a
    for k in range(n):
        if k == src:
            b[k] = k
        for e in range(off[k], off[k + 1]):
            j = adj[e]
            if j >= k:
                continue
            a, c = find(k), find(j)
            if a == c:
                continue
            if k >= src:
                rs = find(src)
                if rs in (a, c):
                    for m in members[c if a == rs else a]:
                        b[m] = k
            if len(members[a]) < len(members[c]):
                a, c = c, a
            root[c] = a
            members[a] += members[c]
            members[c] = []
    return b


def walk(parent, target):
    """vertex indices source first; [] if unreachable"""
    if parent[target] == U32_MAX:
        return []
    path, v = [int(target)], int(target)
    while int(parent[v]) != v:
        v = int(parent[v])
        path.append(v)
        assert len(path) <= len(parent), "the parent chain does not end"
    return path[::-1]


def fold_cost(off, adj, w, path):
    """the left-folded float cost of a walk: per step the cheapest slot u -> v (fl32 adds).  Asserts the walk is
    in the graph."""
    c = F(0)
    for u, v in zip(path[:-1], path[1:]):
        slots = [e for e in range(int(off[u]), int(off[u + 1])) if int(adj[e]) == v]
        assert slots, f"({u}, {v}) is not an edge"
        c = min(F(c + F(w[e])) for e in slots)
    return F(c)


# ---- PRM::solve ---------------------------------------------------------------------------------------------------
def config_distance(a, b):
    """Configuration::distance: l2_norm of a - b in the AVX hsum order (vector/avx.hh:441-452), dim <= 8"""
    v = np.zeros(8, F)
    v[:len(a)] = np.asarray(a, F) - np.asarray(b, F)
    s = (v * v).astype(F)
    return np.sqrt(F(F(F(s[0] + s[4]) + F(s[2] + s[6])) + F(F(s[1] + s[5]) + F(s[3] + s[7]))))


def astar(neighbors, V, n_nodes):
    """utils::astar (planning/utils.hh:75-142) over nodes 0 .. n_nodes-1: start 0, goal 1.  The open set is a
    vector sorted by descending cost after every expansion and popped from the back; an improvement needs
    current_g + d < g.  The reference sorts with pdqsort, which is not stable: equal costs are ordered here by
    Python's stable sort.  Returns (parents list or None, g)."""
    g = np.full(n_nodes, INF, F)
    g[0] = F(0)
    parents = [U32_MAX] * n_nodes
    expanded = [False] * n_nodes
    parents[0] = 0
    open_set = [(0, config_distance(V[1], V[0]))]
    while open_set:
        cur, _ = open_set.pop()
        if cur == 1:
            break
        if expanded[cur]:
            continue
        expanded[cur] = True
        for j, d in neighbors[cur]:
            cand = F(g[cur] + d)
            if cand >= g[j]:
                continue
            g[j] = cand
            parents[j] = cur
            open_set.append((j, F(g[j] + config_distance(V[1], V[j]))))
        open_set.sort(key=lambda x: -float(x[1]))
    return (None if parents[1] == U32_MAX else parents), g


def prm_graph(oracle, robot, oenv, V, base100=(0, 0, 0)):
    """build_roadmap's graph over the vertex sequence V from the oracle: per vertex the (neighbour, dist) appends
    in the reference's order, as (neighbors lists, CSR offsets, adj, w)"""
    n = len(V)
    _, (nbr, dist, cnt, ok) = oracle.build_roadmap_edges(robot, oenv, V, base100)
    neighbors = [[] for _ in range(n)]
    e = 0
    for i in range(n):
        for m in range(int(cnt[i])):
            if ok[e]:
                j, d = int(nbr[i, m]), F(dist[i, m])
                neighbors[i].append((j, d))
                neighbors[j].append((i, d))
            e += 1
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(l) for l in neighbors])
    adj = np.array([j for l in neighbors for j, _ in l], np.uint32)
    w = np.array([d for l in neighbors for _, d in l], F)
    return neighbors, off, adj, w


def prm_solve(neighbors, V, draws, first_draw, max_iterations, max_samples):
    """PRM::solve's loop (prm.hh:109-195) after a failed straight line, over the whole build's `neighbors`
    (prm_graph) and the draw index of every vertex (draws[0] = draws[1] = -1): vertices enter in order, an edge
    exists once its later endpoint has entered, components merge, and astar runs over the graph as it stands
    when start and goal first share a component.  Returns dict(solved, path (vertex indices), cost, iterations,
    size, next_draw)."""
    n = min(len(V), max(max_samples, 2))
    root = list(range(n))

    def find(a):
        while root[a] != a:
            root[a] = root[root[a]]
            a = root[a]
        return a
    last = first_draw + max_iterations - 1
    for i in range(2, n):
        if draws[i] > last:
            n = i
            break
        for j, _ in neighbors[i]:
            if j < i:
                a, c = find(i), find(j)
                if a != c:
                    root[max(a, c)] = min(a, c)
        if find(0) == find(1):
            seen = [[(j, d) for j, d in neighbors[v] if j <= i] for v in range(i + 1)]
            parents, g = astar(seen, V, i + 1)
            assert parents is not None
            path, v = [1], 1
            while parents[v] != v:
                v = parents[v]
                path.append(v)
            it = int(draws[i]) - first_draw + 1
            return dict(solved=True, path=path[::-1], cost=g[1], iterations=it, size=[i + 1, 0],
                        next_draw=first_draw + it)
    if max_samples <= 2:
        taken = 0
    elif n >= max_samples:
        taken = int(draws[max_samples - 1]) - first_draw + 1
    else:
        taken = max_iterations
    return dict(solved=False, path=[], cost=F(0), iterations=taken + 1, size=[n, 0], next_draw=first_draw + taken)


# ---- the sphere-cage problems of the PRM tests (Panda base (0, 0, 0), Halton draws 1 .. 6000) --------------------
_CAGE = {}


def cage_draws(oracle):
    """(oracle environment, scaled draws q [6000, 7], valid [6000]) -- computed once per process"""
    if "draws" not in _CAGE:
        oenv = oracle.sphere_cage_env()
        q = oracle.scale(oracle.halton(7, range(1, 6001)))
        _CAGE["draws"] = (oenv, q, np.asarray(oracle.fkcc_threads(oenv, q), bool))
    return _CAGE["draws"]


def cage_problem(oracle, start_draw, goal_draw, first_draw):
    """start and goal = two valid draws, the sampler at first_draw: dict(V, draws, neighbors, off, adj, w) of the
    whole build over draws first_draw .. 6000 -- computed once per process and problem"""
    key = (start_draw, goal_draw, first_draw)
    if key not in _CAGE:
        oenv, q, valid = cage_draws(oracle)
        later = np.nonzero(valid[first_draw - 1:])[0] + first_draw  # draw indices
        V = np.concatenate([q[start_draw - 1][None], q[goal_draw - 1][None], q[later - 1]]).astype(F)
        draws = np.concatenate([[-1, -1], later]).astype(np.int64)
        neighbors, off, adj, w = prm_graph(oracle, "panda", oenv, V)
        _CAGE[key] = dict(V=V, draws=draws, neighbors=neighbors, off=off, adj=adj, w=w)
    return _CAGE[key]
