"""The neighbour query with caller-chosen k, r and kmax, off the GPU: the host k-d tree (vgpu_cpu_roadmap_knn)
against the plain loop (oracle_py.roadmap_knn_kr) on the cases of tests/knn_cases.py -- every list width, k above
kmax, the admission edges (r = 0, d == r, +inf, k = 0), tie groups cut by k, clustered / flat / outlier data and
the structural sizes -- in shuffled query order, with 1 and 4 threads.  cnt must be equal, nbr and dist bit for
bit on the first cnt slots.  The plain loop itself is pinned to the PRM* entry (vo_roadmap_knn, which
tests/test_oracle_roadmap.py checks against numpy) by running both on the same schedule."""
import numpy as np
import pytest

import knn_cases

F = np.float32


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("name", knn_cases.SMALL)
def test_cpu_kdtree_equals_oracle(oracle, name, threads):
    from vamp_amd import roadmap
    case = knn_cases.get(name)
    q = case.queries()
    order = np.random.default_rng(len(q)).permutation(len(q))
    want = [np.concatenate([case.ref(i)[j] for i in range(len(case.ranges))])[order] for j in range(3)]
    got = roadmap.cpu_knn(case.V, q[order], kmax=case.kmax, threads=threads, k=case.k, r=case.r)
    assert got[2].max() <= case.kmax
    knn_cases.same_lists(got, want, case.kmax)


@pytest.mark.parametrize("robot,dim,n", [("panda", 7, 700), ("fetch", 8, 900), ("baxter", 14, 500)])
def test_kr_with_prm_arrays_equals_prm_entry(oracle, robot, dim, n):
    """roadmap_knn_kr fed the PRM* schedule == roadmap_knn (the wrapper fills the same arrays), also with a kmax
    that truncates the lists, and a query list picks the same rows"""
    rng = np.random.default_rng(31)
    V = oracle.robot_scale(robot, rng.random((n, dim), dtype=F))
    V[n // 2] = V[n // 3]
    sm = oracle.SPACE_MEASURE[robot]
    k = np.array([oracle.prm_max_neighbors(dim, i) if i >= 2 else 0 for i in range(n)], np.uint32)
    r = np.array([oracle.prm_neighbor_radius(dim, sm, 2.0, i) if i >= 2 else 0 for i in range(n)], F)
    for kmax in (int(k.max()), 7):
        want = oracle.roadmap_knn(V, sm, kmax=kmax)
        got = oracle.roadmap_knn_kr(V, k, r, kmax)
        assert want[2][2:].min() >= 1 and want[2].max() == kmax
        for a, b in zip(got, want):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))  # untouched slots are 0 in both
        q = rng.permutation(n)[:200].astype(np.uint32)
        sub = oracle.roadmap_knn_kr(V, k, r, kmax, q, threads=3)
        for a, b in zip(sub, want):
            assert np.array_equal(a.view(np.uint32), b[q].view(np.uint32))


def test_cpu_knn_default_is_the_prm_schedule(oracle):
    """cpu_knn without k, r still runs the PRM* schedule; with them, those arrays; one without the other is an
    error"""
    from vamp_amd import roadmap
    rng = np.random.default_rng(32)
    n, dim = 400, 8
    V = oracle.robot_scale("fetch", rng.random((n, dim), dtype=F))
    sm = oracle.SPACE_MEASURE["fetch"]
    q = np.arange(n, dtype=np.uint32)
    k, r = roadmap.prm_neighbor_params(dim, sm, n)
    a = roadmap.cpu_knn(V, q, sm, threads=2)
    b = roadmap.cpu_knn(V, q, threads=2, k=k, r=r)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert a[0].shape[1] == int(k.max())
    with pytest.raises(ValueError):
        roadmap.cpu_knn(V, q, sm, k=k)
