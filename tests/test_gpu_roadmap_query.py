"""The roadmap queries on the GPU (vgpu_roadmap_query.hip: vgpu_roadmap_sssp, vgpu_roadmap_bottleneck,
vgpu_roadmap_extract_paths, vgpu_roadmap_edge_weights) against the CPU functions, bit for bit, on the synthetic
graphs of tests/roadmap_query_py.py and a tie-heavy random graph; then Robot.prm, Roadmap.connect_index and
Roadmap.shortest_paths on the sphere cage against the restated PRM::solve (tests/test_roadmap_query.py pins the
CPU functions and the cage's facts to the restatement)."""
import numpy as np
import pytest

import roadmap_query_py as rq
from test_gpu_parity import gpu_env_from_oracle

pytestmark = pytest.mark.gpu
F = np.float32
MAX = 0xffffffff


@pytest.fixture(scope="module")
def vamp():
    import vamp_amd
    assert vamp_amd.context(0) is not None
    return vamp_amd


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def gpu_sssp(vamp, graph, sources, limits=None):
    """(g, hops, parent) host arrays of vgpu_roadmap_sssp, and the device graph"""
    import torch
    from vamp_amd import roadmap
    off, adj, w = graph
    dg = roadmap.DeviceGraph(torch, off, adj, vamp.context(0), weights=w)
    g, hops, parent = roadmap.sssp_device(torch, dg, sources, limits)
    return g.cpu().numpy(), u32(hops), u32(parent), dg, parent


def same_search(vamp, graph, sources, limits=None):
    """the GPU batch equals the CPU function bit for bit; returns the CPU result"""
    from vamp_amd import roadmap
    g, hops, parent, dg, _ = gpu_sssp(vamp, graph, sources, limits)
    wg, wh, wp = roadmap.cpu_sssp(*graph, sources, limits)
    assert np.array_equal(rq.bits(g), rq.bits(wg))
    assert np.array_equal(hops, wh)
    assert np.array_equal(parent, wp)
    return wg, wh, wp


def same_bottleneck(vamp, graph, sources):
    import torch
    from vamp_amd import roadmap
    dg = roadmap.DeviceGraph(torch, graph[0], graph[1], vamp.context(0), weights=graph[2])
    b = u32(roadmap.bottleneck_device(torch, dg, sources))
    assert np.array_equal(b, roadmap.cpu_bottleneck(graph[0], graph[1], sources))
    return b


def same_paths(vamp, graph, sources, targets, limits=None, cap=None):
    """vgpu_roadmap_extract_paths equals the host walk over the CPU function's parents"""
    import torch
    from vamp_amd import roadmap
    n = len(graph[0]) - 1
    cap = n if cap is None else cap
    _, _, _, _, parent = gpu_sssp(vamp, graph, sources, limits)
    idx, ln = roadmap.extract_paths_device(torch, parent, targets, cap, vamp.context(0))
    idx, ln = u32(idx), u32(ln)
    _, _, wp = roadmap.cpu_sssp(*graph, sources, limits)
    for s, t in enumerate(targets):
        want = roadmap.walk_parents(wp[s], int(t))
        if len(want) > cap:
            assert ln[s] == MAX
        else:
            assert ln[s] == len(want) and idx[s, :ln[s]].tolist() == want
    return ln


@pytest.mark.parametrize("name", sorted(rq.SMALL))
def test_small_graphs_equal_cpu(vamp, name):
    graph = rq.SMALL[name]()
    n = len(graph[0]) - 1
    sources = np.arange(n, dtype=np.uint32)
    same_search(vamp, graph, sources)
    same_search(vamp, graph, sources, np.maximum(sources, n - 2))
    same_bottleneck(vamp, graph, sources)
    for k in range(n):
        same_paths(vamp, graph, sources, (sources + k) % n)


def test_known_answers(vamp):
    """the tie rules on the GPU itself: fewest waypoints, then the smaller predecessor; plateaus by BFS level"""
    g, hops, parent, _, _ = gpu_sssp(vamp, rq.equal_cost_graph(), [0])
    assert g[0, 1] == 2.0 and parent[0, 1] == 0 and g[0, 8] == 3.0 and parent[0, 8] == 6 and hops[0, 8] == 2
    g, hops, parent, _, _ = gpu_sssp(vamp, rq.absorption_graph(), [0])
    assert g[0, 1:5].tolist() == [2.0 ** 24] * 4 and hops[0, 1:6].tolist() == [1, 2, 3, 3, 2]
    assert parent[0, 1:6].tolist() == [0, 1, 2, 2, 1]
    g, hops, parent, _, _ = gpu_sssp(vamp, rq.limit_graph(), [0, 0], [5, 4])
    assert g[:, 1].tolist() == [2.0, 6.0] and parent[0, 1] == 5 and parent[1, 1] == 3 and np.isinf(g[1, 5])


def test_path_graph_rounds_and_frontier_work(vamp):
    """2,000 rounds in a row; a frontier relaxes every slot once, a full sweep per round would relax 2,000 x"""
    from vamp_amd import roadmap
    graph = rq.path_graph()
    n_adj = len(graph[1])
    wg, wh, _ = same_search(vamp, graph, [0])
    stats = roadmap.sssp_stats(vamp.context(0))
    print("path graph stats", stats, "n_adj", n_adj)
    assert stats["relaxed_slots"] <= 4 * n_adj
    assert stats["relaxed_slots"] == n_adj and stats["rounds"] == 2000 and stats["frontier_items"] == 2000
    assert wh[0, -1] == 1999
    same_search(vamp, graph, [1234, 1999, 0], [1999, 1999, 1000])
    same_bottleneck(vamp, graph, [700, 0])
    ln = same_paths(vamp, graph, [0, 0, 5], [1999, 10, 5], cap=100)
    assert ln.tolist() == [MAX, 11, 1]  # a path longer than cap is reported, not written


def test_hub_wider_than_a_wave(vamp):
    graph = rq.hub_graph()
    n = len(graph[0]) - 1
    same_search(vamp, graph, [0, n - 1, 1])
    same_bottleneck(vamp, graph, [0, n - 1])
    same_paths(vamp, graph, [0, n - 1], [n - 1, 2])


def test_trivial_sizes_and_rejections(vamp):
    import torch
    from vamp_amd import VgpuError, roadmap
    ctx = vamp.context(0)
    one = (np.zeros(2, np.uint64), np.zeros(0, np.uint32), np.zeros(0, F))
    g, hops, parent, dg, _ = gpu_sssp(vamp, one, [0, 0])
    assert g.tolist() == [[0.0], [0.0]] and hops.tolist() == [[0], [0]] and parent.tolist() == [[0], [0]]
    assert u32(roadmap.bottleneck_device(torch, dg, [0])).tolist() == [[0]]
    graph = rq.limit_graph()
    assert gpu_sssp(vamp, graph, [])[0].shape == (0, 6)  # S = 0
    none = (np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, F))
    assert gpu_sssp(vamp, none, [])[0].shape == (0, 0)  # n = 0
    off, adj, w = graph
    for bad in (F(-1), F(np.nan)):
        wb = w.copy()
        wb[3] = bad
        with pytest.raises(VgpuError, match="invalid argument.*weight"):
            gpu_sssp(vamp, (off, adj, wb), [0])
    for sources, limits in (([6], None), ([3], [2]), ([0, 5], [5, 4])):
        with pytest.raises(VgpuError, match="invalid argument.*source"):
            gpu_sssp(vamp, graph, sources, limits)
    ab = adj.copy()
    ab[0] = 6  # a slot index >= n is refused before any round reads through it
    with pytest.raises(VgpuError, match="invalid argument.*slot"):
        gpu_sssp(vamp, (off, ab, w), [0])
    with pytest.raises(VgpuError, match="invalid argument"):
        same_bottleneck(vamp, graph, [6])
    same_search(vamp, graph, [0])  # the context still works after the refusals


@pytest.fixture(scope="module")
def random_case():
    """20,000 vertices, 8 partners drawn per vertex, weights from {1, 2, 3}; 65 searches (one more than a wave),
    each with a limit drawn from the upper quarter of the indices; the CPU result, computed once"""
    from vamp_amd import roadmap
    n = 20000
    graph = rq.random_graph(n)
    rng = np.random.default_rng(8)
    limits = rng.integers(3 * n // 4, n, 65).astype(np.uint32)
    sources = rng.integers(0, 3 * n // 4, 65).astype(np.uint32)
    targets = rng.integers(0, n, 65).astype(np.uint32)
    return graph, sources, limits, targets, roadmap.cpu_sssp(*graph, sources, limits)


def test_random_graph_ties_are_deterministic(vamp, random_case):
    graph, sources, limits, targets, (wg, wh, wp) = random_case
    multi = total = 0
    for s in range(len(sources)):
        reached = np.isfinite(wg[s])
        multi += int((rq.tight_predecessors(*graph, wg[s], int(limits[s]))[reached] > 1).sum())
        total += int(reached.sum())
    print("reached vertices with more than one tight predecessor:", multi / total)
    assert 2 * multi >= total  # the tie rule is not vacuous here
    first = gpu_sssp(vamp, graph, sources, limits)
    again = gpu_sssp(vamp, graph, sources, limits)
    for a, b in zip(first[:3], again[:3]):
        assert a.tobytes() == b.tobytes()
    assert np.array_equal(rq.bits(first[0]), rq.bits(wg))
    assert np.array_equal(first[1], wh) and np.array_equal(first[2], wp)
    same_paths(vamp, graph, sources, targets, limits, cap=64)
    b = same_bottleneck(vamp, graph, sources[:3])
    assert (b != MAX).all()


@pytest.mark.parametrize("robot,dim", [("ur5", 6), ("panda", 7), ("fetch", 8), ("baxter", 14)])
def test_edge_weights_equal_knn_distances(vamp, oracle, robot, dim):
    """the graph of ALL kNN candidates over 3,000 scaled configurations (one duplicated): a slot's weight has
    the bits of the neighbour query's dist, in both directions"""
    import torch
    from vamp_amd import roadmap
    rng = np.random.default_rng(30 + dim)
    n = 3000
    V = oracle.robot_scale(robot, rng.random((n, dim), dtype=F))
    V[n // 2] = V[n // 3]
    nbr, dist, cnt = oracle.roadmap_knn(V, oracle.SPACE_MEASURE[robot])
    edges = [(i, int(nbr[i, m]), dist[i, m]) for i in range(n) for m in range(int(cnt[i]))]
    off, adj, want = rq.csr(n, edges)
    assert len(adj) == 2 * len(edges) and (want == 0).sum() == 2
    dg = roadmap.DeviceGraph(torch, off, adj, vamp.context(0), vertices=V)
    got = dg.w.cpu().numpy()[:len(adj)]
    assert np.array_equal(rq.bits(got), rq.bits(want))


# ---- Robot.prm on the sphere cage -----------------------------------------------------------------------------------
def prm_settings(vamp, robot, max_iterations, max_samples=100000):
    s = vamp.PRMSettings(vamp.PRMNeighborParams(robot.dimension(), robot.space_measure()))
    s.max_iterations, s.max_samples = max_iterations, max_samples
    return s


def run_prm(vamp, oracle, problem, first_draw, max_iterations, max_samples=100000, **kw):
    oenv, _, _ = rq.cage_draws(oracle)
    env = gpu_env_from_oracle(vamp, oenv)
    robot = vamp.panda_0_0
    rng = robot.halton()
    rng.index = first_draw
    res = robot.prm(problem["V"][0], problem["V"][1], env, prm_settings(vamp, robot, max_iterations, max_samples), rng,
                    **kw)
    return res, rng


def same_result(res, rng, want, V):
    assert res.solved == want["solved"] and res.iterations == want["iterations"] and list(res.size) == want["size"]
    assert rng.index == want["next_draw"]
    assert np.array_equal(np.asarray(res.path).reshape(-1, V.shape[1]), V[want["path"]].reshape(-1, V.shape[1]))
    if want["solved"]:
        assert rq.bits(F(res.cost)) == rq.bits(want["cost"])


def test_prm_solved_at_the_first_connection(vamp, oracle):
    p = rq.cage_problem(oracle, 10, 13, 14)
    oenv, _, _ = rq.cage_draws(oracle)
    assert not oracle.validate_motions(oenv, p["V"][:1], p["V"][1:2])[0][0]  # the straight line is blocked
    want = rq.prm_solve(p["neighbors"], p["V"], p["draws"], 14, 5987, 100000)
    assert want["solved"] and want["size"] == [139, 0] and want["iterations"] == 768 and want["path"] == [0, 79, 62, 138, 1]
    res, rng = run_prm(vamp, oracle, p, 14, 5987)
    same_result(res, rng, want, p["V"])
    assert rng.index == 782 and len(res.path) == 5
    # schedule independence: a first chunk of 64 draws takes three stages to the same result
    res64, rng64 = run_prm(vamp, oracle, p, 14, 5987, _first_chunk=64)
    same_result(res64, rng64, want, p["V"])
    assert np.array_equal(res64.path, res.path) and res64.cost == res.cost
    # a sample limit below vertex 138 ends the loop first
    want100 = rq.prm_solve(p["neighbors"], p["V"], p["draws"], 14, 5987, 100)
    assert not want100["solved"] and want100["size"] == [100, 0]
    res100, rng100 = run_prm(vamp, oracle, p, 14, 5987, max_samples=100)
    same_result(res100, rng100, want100, p["V"])


def test_prm_unsolved(vamp, oracle):
    p = rq.cage_problem(oracle, 14, 22, 23)
    want = rq.prm_solve(p["neighbors"], p["V"], p["draws"], 23, 5978, 100000)
    assert not want["solved"] and want["iterations"] == 5979 and want["size"] == [1025, 0]
    res, rng = run_prm(vamp, oracle, p, 23, 5978)
    same_result(res, rng, want, p["V"])
    assert len(res.path) == 0 and rng.index == 6001


def test_prm_straight_line_and_goal_lists(vamp, oracle):
    p = rq.cage_problem(oracle, 10, 13, 14)
    oenv, _, _ = rq.cage_draws(oracle)
    env = gpu_env_from_oracle(vamp, oenv)
    robot = vamp.panda_0_0
    start = p["V"][0]
    goal = (start + F(0.01) * (p["V"][1] - start)).astype(F)
    assert oracle.validate_motions(oenv, start[None], goal[None])[0][0]
    rng = robot.halton()
    rng.index = 14
    res = robot.prm(start, goal, env, prm_settings(vamp, robot, 5987), rng)
    assert res.solved and res.iterations == 0 and list(res.size) == [1, 1] and rng.index == 14
    assert np.array_equal(res.path, np.stack([start, goal]))
    with pytest.raises(vamp.VgpuError, match="not supported"):
        robot.prm(start, [goal, p["V"][1]], env)


def test_roadmap_query_methods(vamp, oracle):
    """connect_index, shortest_paths and weights of the Roadmap that Robot.roadmap returns for the solved problem"""
    p = rq.cage_problem(oracle, 10, 13, 14)
    oenv, _, _ = rq.cage_draws(oracle)
    env = gpu_env_from_oracle(vamp, oenv)
    robot = vamp.panda_0_0
    rng = robot.halton()
    rng.index = 14
    rm = robot.roadmap(p["V"][0], p["V"][1], env, prm_settings(vamp, robot, 5987), rng)
    assert np.array_equal(rm.vertices, p["V"]) and np.array_equal(rm.adj, p["adj"])
    assert np.array_equal(rq.bits(rm.weights), rq.bits(p["w"]))
    assert rm.connect_index() == 138 and rm.connect_index(0, 0) == 0
    want = rq.prm_solve(p["neighbors"], p["V"], p["draws"], 14, 5987, 100000)
    (prefix, cost, hops), (full, cost_full, hops_full), (same, cost_same, _) = rm.shortest_paths([0, 0, 7], [1, 1, 7],
                                                                                                  [138, 1026, 1026])
    assert prefix.tolist() == want["path"] and rq.bits(cost) == rq.bits(want["cost"]) and hops == 4
    wg, _, wp = rq.sssp(p["off"], p["adj"], p["w"], 0)
    assert full.tolist() == rq.walk(wp, 1) and rq.bits(cost_full) == rq.bits(wg[1]) and hops_full == 5
    assert cost_full != cost and same.tolist() == [7] and cost_same == 0
    assert rm.shortest_paths([0], [1])[0][0].tolist() == full.tolist()  # no limit: the whole build
    stats = rm.sssp_stats()
    assert stats["rounds"] >= 5 and stats["relaxed_slots"] >= len(p["adj"]) // 2 and stats["host_reads"] > stats["rounds"]
    unsolved = rq.cage_problem(oracle, 14, 22, 23)
    rng.index = 23
    rm2 = robot.roadmap(unsolved["V"][0], unsolved["V"][1], env, prm_settings(vamp, robot, 5978), rng)
    assert rm2.connect_index() is None
    path, cost, hops = rm2.shortest_paths([0], [1])[0]
    assert len(path) == 0 and np.isinf(cost) and hops == -1
