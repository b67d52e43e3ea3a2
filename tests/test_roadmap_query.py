"""The roadmap queries on the host CPU (vgpu_cpu_roadmap_sssp, vgpu_cpu_roadmap_bottleneck) against the plain-Python
restatement (tests/roadmap_query_py.py), bit for bit: g, hops, parent, bottleneck and the walked paths on synthetic
CSR graphs, each the smallest shape at which something specific can break; then the reference's PRM::solve loop
restated over the oracle's roadmap of the sphere cage, whose facts the GPU tests of Robot.prm rely on.  No GPU."""
import numpy as np
import pytest

import roadmap_query_py as rq

F = np.float32
MAX = 0xffffffff


@pytest.fixture(scope="module")
def roadmap():
    from vamp_amd import roadmap
    return roadmap


def check_search(roadmap, graph, src, limit=None):
    """one search of the CPU function against the restatement, plus the path properties of every target"""
    off, adj, w = graph
    n = len(off) - 1
    g, hops, parent = roadmap.cpu_sssp(off, adj, w, [src], None if limit is None else [limit])
    wg, wh, wp = rq.sssp(off, adj, w, src, limit)
    assert np.array_equal(rq.bits(g[0]), rq.bits(wg))
    assert np.array_equal(hops[0], wh)
    assert np.array_equal(parent[0], wp)
    for t in range(n):
        path = roadmap.walk_parents(parent[0], t)
        assert path == rq.walk(wp, t)
        if not path:
            assert g[0, t] == np.inf and hops[0, t] == MAX
            continue
        assert path[0] == src and path[-1] == t and len(set(path)) == len(path) == int(hops[0, t]) + 1
        assert rq.bits(rq.fold_cost(off, adj, w, path)) == rq.bits(g[0, t])
    return g[0], hops[0], parent[0]


@pytest.mark.parametrize("name", sorted(rq.SMALL))
def test_small_graphs_equal_restatement(roadmap, name):
    graph = rq.SMALL[name]()
    n = len(graph[0]) - 1
    for src in range(n):
        check_search(roadmap, graph, src)
        check_search(roadmap, graph, src, limit=max(src, n - 2))
        b = roadmap.cpu_bottleneck(graph[0], graph[1], [src])
        assert np.array_equal(b[0], rq.bottleneck(graph[0], graph[1], src))


def test_path_graph_order(roadmap):
    """2,000 vertices in a row: every prefix sum depends on the order of the float additions"""
    graph = rq.path_graph()
    g, hops, parent = check_search(roadmap, graph, 0)
    assert np.array_equal(hops, np.arange(2000)) and np.array_equal(parent[1:], np.arange(1999))
    check_search(roadmap, graph, 1234)
    b = roadmap.cpu_bottleneck(graph[0], graph[1], [700])
    assert np.array_equal(b[0], np.maximum(np.arange(2000), 700))
    assert np.array_equal(b[0], rq.bottleneck(graph[0], graph[1], 700))


def test_hub_wider_than_a_wave(roadmap):
    graph = rq.hub_graph()
    n = len(graph[0]) - 1
    assert int(np.diff(graph[0].astype(np.int64)).max()) == 5000
    g, hops, parent = roadmap.cpu_sssp(*graph, [0, n - 1])
    for s, src in enumerate((0, n - 1)):
        wg, wh, wp = rq.sssp(*graph, src)
        assert np.array_equal(rq.bits(g[s]), rq.bits(wg)) and np.array_equal(hops[s], wh)
        assert np.array_equal(parent[s], wp)
    assert hops[0].max() == 3 and hops[1].max() == 6
    assert np.array_equal(roadmap.cpu_bottleneck(graph[0], graph[1], [n - 1])[0], rq.bottleneck(graph[0], graph[1], n - 1))


def test_plateaus_are_ordered_by_bfs_levels(roadmap):
    g, hops, parent = check_search(roadmap, rq.plateau_graph(), 0)
    assert g[1:6].tolist() == [1.5] * 5
    assert hops.tolist() == [0, 1, 2, 2, 3, 4, 5] and parent.tolist() == [0, 0, 1, 1, 3, 4, 5]
    g, hops, parent = check_search(roadmap, rq.absorption_graph(), 0)
    assert g[1:5].tolist() == [2.0 ** 24] * 4  # fl(2^24 + 0.5) == 2^24
    assert g[5] == F(2.0 ** 24 + 2) and parent[5] == 1 and hops[5] == 2  # 2.5 and 2.0 round alike: fewest hops
    assert hops[1:5].tolist() == [1, 2, 3, 3] and parent[1:5].tolist() == [0, 1, 2, 2]


def test_equal_cost_alternatives(roadmap):
    g, hops, parent = check_search(roadmap, rq.equal_cost_graph(), 0)
    assert g[1] == 2.0 and parent[1] == 0 and hops[1] == 1  # direct beats 1 + 1 and 0.5 x 4
    assert g[8] == 3.0 and parent[8] == 6 and hops[8] == 2  # of two 2-hop routes, the smaller predecessor


def test_disconnected_isolated_and_trivial(roadmap):
    graph = rq.disconnected_graph()
    g, hops, parent = check_search(roadmap, graph, 0)
    assert np.isinf(g[3:]).all() and (hops[3:] == MAX).all() and (parent[3:] == MAX).all()
    g, hops, parent = check_search(roadmap, graph, 6)  # an isolated source; source == target
    assert g[6] == 0 and parent[6] == 6 and hops[6] == 0 and np.isinf(g[:6]).all()
    assert roadmap.walk_parents(parent, 6) == [6]
    b = roadmap.cpu_bottleneck(graph[0], graph[1], [4, 6])
    assert b.tolist() == [[MAX] * 3 + [4, 4, 5, MAX], [MAX] * 6 + [6]]
    # n = 1, n = 0 and S = 0
    one = (np.zeros(2, np.uint64), np.zeros(0, np.uint32), np.zeros(0, F))
    g, hops, parent = roadmap.cpu_sssp(*one, [0])
    assert g.tolist() == [[0.0]] and hops.tolist() == [[0]] and parent.tolist() == [[0]]
    assert roadmap.cpu_bottleneck(one[0], one[1], [0]).tolist() == [[0]]
    none = (np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, F))
    assert roadmap.cpu_sssp(*none, [])[0].shape == (0, 0)
    assert roadmap.cpu_sssp(*graph, [])[0].shape == (0, 7) and roadmap.cpu_bottleneck(graph[0], graph[1], []).shape == (0, 7)
    from vamp_amd import VgpuError
    with pytest.raises(VgpuError, match="invalid argument"):
        roadmap.cpu_sssp(*none, [0])


def test_loops_repeats_and_inf_edges(roadmap):
    g, hops, parent = check_search(roadmap, rq.loops_graph(), 0)
    assert g.tolist() == [0, 1, 2, 3, 4, np.inf] and parent[4] == 3 and parent[5] == MAX


def test_bad_weights_and_sources_are_rejected(roadmap):
    from vamp_amd import VgpuError
    off, adj, w = rq.limit_graph()
    for bad in (F(-1), F(np.nan)):
        wb = w.copy()
        wb[3] = bad
        with pytest.raises(VgpuError, match="invalid argument"):
            roadmap.cpu_sssp(off, adj, wb, [0])
    for sources, limits in (([6], None), ([3], [2]), ([0, 5], [5, 4])):
        with pytest.raises(VgpuError, match="invalid argument"):
            roadmap.cpu_sssp(off, adj, w, sources, limits)
    with pytest.raises(VgpuError, match="invalid argument"):
        roadmap.cpu_bottleneck(off, adj, [6])
    ab = adj.copy()
    ab[0] = 6
    with pytest.raises(VgpuError, match="invalid argument"):
        roadmap.cpu_sssp(off, ab, w, [0])


def test_limit_cuts_the_short_route(roadmap):
    graph = rq.limit_graph()
    g, _, parent = check_search(roadmap, graph, 0)
    assert g[1] == 2.0 and roadmap.walk_parents(parent, 1) == [0, 5, 1]
    g, _, parent = check_search(roadmap, graph, 0, limit=4)
    assert g[1] == 6.0 and roadmap.walk_parents(parent, 1) == [0, 2, 3, 1] and np.isinf(g[5])
    g, hops, parent = roadmap.cpu_sssp(*graph, [0, 0, 0], [5, 4, 3])  # one limit per search
    assert g[:, 1].tolist() == [2.0, 6.0, 6.0] and np.isinf(g[2, 4]) and g[1, 4] == 9.0
    assert rq.bottleneck(graph[0], graph[1], 0)[1] == 3 == roadmap.cpu_bottleneck(graph[0], graph[1], [0])[0, 1]


def test_random_graph_ties_equal_restatement(roadmap):
    """a smaller cut of the GPU tests' tie-heavy graph, against the restatement"""
    graph = rq.random_graph(3000, 8, 11)
    g, hops, parent = check_search(roadmap, graph, 17, limit=2500)
    reached = np.isfinite(g)
    assert (rq.tight_predecessors(*graph, g, 2500)[reached] > 1).mean() > 0.5
    assert np.array_equal(roadmap.cpu_bottleneck(graph[0], graph[1], [17])[0], rq.bottleneck(graph[0], graph[1], 17))


# ---- PRM::solve restated on the sphere cage ------------------------------------------------------------------------
def test_cage_facts(oracle):
    _, _, valid = rq.cage_draws(oracle)
    assert int(valid.sum()) == 1027 and (np.nonzero(valid)[0][:4] + 1).tolist() == [10, 13, 14, 22]
    p = rq.cage_problem(oracle, 10, 13, 14)
    assert len(p["V"]) == 1027 and len(p["adj"]) == 16196 and max(len(l) for l in p["neighbors"]) == 75


def test_prm_solve_restated_equals_cpu_search(oracle, roadmap):
    """the solved problem: astar over the graph at its first connection and the CPU search over the prefix agree"""
    p = rq.cage_problem(oracle, 10, 13, 14)
    res = rq.prm_solve(p["neighbors"], p["V"], p["draws"], 14, 5987, 100000)
    assert res["solved"] and res["size"] == [139, 0] and res["iterations"] == 768 and res["next_draw"] == 782
    assert p["draws"][138] == 781 and res["path"] == [0, 79, 62, 138, 1]
    assert abs(float(res["cost"]) - 15.352402) < 1e-5
    off, adj, w = p["off"], p["adj"], p["w"]
    assert roadmap.cpu_bottleneck(off, adj, [0])[0, 1] == 138 == rq.bottleneck(off, adj, 0)[1]
    g, hops, parent = roadmap.cpu_sssp(off, adj, w, [0, 0], [138, len(off) - 2])
    assert roadmap.walk_parents(parent[0], 1) == res["path"] and rq.bits(g[0, 1]) == rq.bits(res["cost"])
    # over the whole build the shortest path is another one: searching the full graph is a different answer
    full = roadmap.walk_parents(parent[1], 1)
    assert len(full) == 6 and abs(float(g[1, 1]) - 13.302937) < 1e-5 and g[1, 1] != g[0, 1]
    # no vertex of this graph has two tight predecessors (ties are tested on synthetic graphs)
    assert rq.tight_predecessors(off, adj, w, g[1]).max() == 1
    wg, wh, wp = rq.sssp(off, adj, w, 0, 138)
    assert np.array_equal(rq.bits(g[0]), rq.bits(wg)) and np.array_equal(hops[0], wh) and np.array_equal(parent[0], wp)


def test_prm_unsolved_and_sample_limit_restated(oracle, roadmap):
    p = rq.cage_problem(oracle, 14, 22, 23)
    assert len(p["V"]) == 1025
    res = rq.prm_solve(p["neighbors"], p["V"], p["draws"], 23, 5978, 100000)
    assert not res["solved"] and res["iterations"] == 5979 and res["size"] == [1025, 0] and res["path"] == []
    g, _, _ = roadmap.cpu_sssp(p["off"], p["adj"], p["w"], [0])
    assert int(np.isfinite(g[0]).sum()) == 973 and np.isinf(g[0, 1])
    assert roadmap.cpu_bottleneck(p["off"], p["adj"], [0])[0, 1] == MAX
    p = rq.cage_problem(oracle, 10, 13, 14)
    res = rq.prm_solve(p["neighbors"], p["V"], p["draws"], 14, 5987, 100)
    assert not res["solved"] and res["size"] == [100, 0] and res["iterations"] == int(p["draws"][99]) - 14 + 2


# ---- the new kernels' registers (as tests/test_kernel_resources.py reads them) -------------------------------------
QUERY_KERNELS = [r"vgpu::rq::relax_kernel<true>", r"vgpu::rq::relax_kernel<false>", r"vgpu::rq::tight_kernel",
                 r"vgpu::rq::seed_kernel<true>", r"vgpu::rq::seed_kernel<false>", r"vgpu::rq::tight_seed_kernel",
                 r"vgpu::rq::check_kernel", r"vgpu::rq::fill_kernel", r"vgpu::rq::extract_kernel",
                 r"vgpu::edge_weights_kernel<6>", r"vgpu::edge_weights_kernel<7>", r"vgpu::edge_weights_kernel<8>",
                 r"vgpu::edge_weights_kernel<14>"]


def test_query_kernels_do_not_spill():
    """every kernel of the query path is in the built library's gfx950 code object with 0 scratch and 0 VGPR
    spills (AMDGPU metadata note, tools/kernel_resources.py)"""
    import os
    import re
    import sys

    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    kernels = kernel_resources.kernels(os.path.join(ROOT, "mr-vamp_amd", "vamp_amd", "libvampgpu.so"))
    for pattern in QUERY_KERNELS:
        got = [k for k in kernels if re.search(re.escape(pattern), k["name"])]
        assert got, f"no kernel matches {pattern}"
        bad = [(k["name"][:100], k["vgpr"], k["vgpr_spill"], k["scratch"]) for k in got if k["scratch"] or k["vgpr_spill"]]
        assert not bad, bad
