"""Batched RRT-Connect on the GPU (mr-vamp_amd/csrc/vgpu_rrtc.hip, vgpu_rrtc_batch: one wave per planning problem)
against the CPU planner problem by problem.  The reference throughout is Robot.rrtc (vgpu_cpu_rrtc), which
tests/test_rrtc.py pins to the restatement tests/rrtc_py.py; every equality is bitwise: the path viewed as uint32,
the cost's bits, iterations, tree sizes, solved and the advanced rng index, each compared with a CPU call given the
same rng_first.

The 16 table_pick problems of the fixture each come with their OWN scene (same obstacle counts, different
obstacles), and a batch call has one environment: so a problem runs in a batch of its own scene -- with several
sampler offsets, which are different searches -- and the ragged many-problem batches put all 16 start/goal pairs into
one of the scenes under an iteration bound (most of them are then unsolvable there, and stop at the bound).

Settings, goals, bases and scenes come from tests/rrtc_cases.py, whose every case tests/test_rrtc.py compares
between the CPU planner and the restatement; only what exists for a limit or an error code (an arena or a
path_cap chosen to be hit) is stated here."""
import numpy as np
import pytest

import oracle_py as op
import rrtc_cases as rc
from conftest import host_fixture
from test_gpu_parity import gpu_env_from_oracle
from test_rrtc import problem

pytestmark = pytest.mark.gpu
F = np.float32
BIG = rc.BIG
DEFAULT = rc.CASES["default"].settings


@pytest.fixture(scope="module")
def vamp():
    import vamp_amd
    return vamp_amd


@pytest.fixture(scope="module")
def scenes(vamp):
    """problem k -> (oracle environment, vamp environment, start, goal)"""
    fx = host_fixture("panda_table_pick_problems.npz", op)
    assert int(fx["n_problems"]) == 16
    out = {}
    for k in range(1, 17):
        o, s, g = problem(op, fx, k)
        out[k] = (o, gpu_env_from_oracle(vamp, o), s.astype(F), g.astype(F))
    return out


def cpu_run(vamp, robot, env, s, g, settings, first):
    rng = robot.halton()
    rng.skip(int(first) - 1)
    return robot.rrtc(s, g, env, vamp.RRTCSettings(**settings), rng), rng.index


def same_result(got, idx, want, widx, tag):
    assert (got.solved, got.iterations, tuple(got.size)) == (want.solved, want.iterations, tuple(want.size)), \
        (tag, got.solved, got.iterations, got.size, want.solved, want.iterations, want.size)
    assert got.path.shape == want.path.shape, (tag, got.path.shape, want.path.shape)
    assert np.array_equal(got.path.view(np.uint32), want.path.view(np.uint32)), tag
    assert np.float32(got.cost).view(np.uint32) == np.float32(want.cost).view(np.uint32), (tag, got.cost, want.cost)
    assert int(idx) == int(widx), (tag, int(idx), int(widx))


def check_batch(vamp, robot, env, starts, goals, settings, firsts, cpu_settings=None, tag=None, **kw):
    """rrtc_batch == rrtc problem by problem; returns (batch results, status, CPU results)"""
    starts, goals = np.asarray(starts, F), np.asarray(goals, F)
    got, status, idx = robot.rrtc_batch(starts, goals, env, vamp.RRTCSettings(**settings), rng_first=firsts, **kw)
    firsts = np.broadcast_to(np.asarray(firsts, np.uint64), (len(starts),))
    assert len(got) == len(status) == len(idx) == len(starts)
    want = []
    for k in range(len(starts)):
        w, widx = cpu_run(vamp, robot, env, starts[k], goals[k], cpu_settings or settings, firsts[k])
        same_result(got[k], idx[k], w, widx, (tag, k))
        assert got[k].nanoseconds == 0
        want.append(w)
    stats = robot.rrtc_stats()
    assert stats["iterations"] == sum(r.iterations for r in want)
    assert stats["max_iterations"] == max(r.iterations for r in want)
    return got, status, want


def check_own_scene(vamp, scenes, k, settings, firsts=(1, 1001), robot=None, **kw):
    """problem k in its scene, once per sampler offset, as one batch"""
    _, env, s, g = scenes[k]
    n = len(firsts)
    return check_batch(vamp, robot or vamp.panda_0_0, env, np.tile(s, (n, 1)), np.tile(g, (n, 1)), settings,
                       np.array(firsts, np.uint64), tag=k, **kw)


def run_case(vamp, scenes, name, **kw):
    """every batch of a case of the table, one call each; returns [(batch results, status, CPU results)]"""
    case = rc.CASES[name]
    out = []
    for b in range(len(case.batches)):
        k, starts, goals, firsts = case.arrays(b)
        env = rc.vamp_env(vamp, k, True) if case.cloud else scenes[k][1]
        out.append(check_batch(vamp, vamp.PandaBase(*case.base), env, starts, goals, case.settings, firsts,
                               tag=(name, k), **dict(case.gpu, **kw)))
    return out


# ---- 1. the default range: all 16 problems, two sampler offsets, two bases --------------------------------------------
@pytest.mark.parametrize("base", [(0, 0, 0), (200, 200, 0)], ids=["base0", "base200"])
def test_default_range_matches_cpu(vamp, scenes, base):
    case = rc.CASES["default" if base == (0, 0, 0) else "default-base200"]
    assert case.base == base and case.batches == rc.own(range(1, 17))
    robot = vamp.PandaBase(*base)
    its = []
    for k in range(1, 17):
        got, status, want = check_own_scene(vamp, scenes, k, case.settings, robot=robot, node_cap=256, path_cap=64)
        assert not status.any()
        its += [r.iterations for r in want]
        if base == (0, 0, 0) and k in (1, 15):  # the straight-line problems
            for r in got:
                assert r.iterations == 0 and r.size == (1, 1) and r.cost == 0 and len(r.path) == 2
    if base == (0, 0, 0):
        assert min(its) == 0 and max(its) >= 100, its


def test_ragged_batch_in_one_scene(vamp, scenes):
    """P = 32 in one call: all 16 start/goal pairs x two offsets in problem 4's scene, at most 300 iterations:
    problem 4 itself solves, problems foreign to the scene mostly stop at the bound, some connect at once"""
    (_, status, want), = run_case(vamp, scenes, "ragged32")
    assert len(want) == 32 and not status.any()
    assert want[3].solved and want[3].iterations > 1
    assert len({r.iterations for r in want}) >= 3, [r.iterations for r in want]


# ---- 2. trees wider than a wave; the sample cap ---------------------------------------------------------------------
WIDE = list(rc.WIDE)


def test_wide_trees_and_sample_cap(vamp, scenes):
    settings = rc.CASES["wide"].settings
    assert rc.CASES["wide"].batches == rc.own(WIDE) and settings["max_samples"] == 200
    arena = dict(settings, max_samples=BIG)
    sizes, capped = [], []
    for k in WIDE:
        _, status, want = check_own_scene(vamp, scenes, k, settings, node_cap=256, path_cap=256)
        assert not status.any()
        hit = [not r.solved and sum(r.size) == 200 for r in want]
        # the arena as the limit: the same results, CAPACITY on exactly the problems that hit it
        _, status, _ = check_own_scene(vamp, scenes, k, arena, cpu_settings=settings, node_cap=200, path_cap=256)
        assert status.tolist() == [vamp.Robot.RRTC_CAPACITY if c else vamp.Robot.RRTC_DONE for c in hit], (k, status)
        sizes += [max(r.size) for r in want]
        capped += hit
    assert max(sizes) >= 65, sizes           # a tree wider than the wave
    assert any(capped) and not all(capped)   # a search that ends unsolved at the cap, in mid-connect or not


# ---- 3. the iteration bound and slicing ----------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 8, 11])
def test_iteration_bound_and_slices(vamp, scenes, k):
    settings = rc.CASES["iter40"].settings
    assert (k, [(k, (k,), 1), (k, (k,), 1001)]) in rc.CASES["iter40"].batches
    robot = vamp.panda_0_0
    first = None
    for sl in (1, 7, 256):
        got, _, want = check_own_scene(vamp, scenes, k, settings, node_cap=256, path_cap=64, slice=sl)
        assert not want[0].solved and want[0].iterations == 41
        most = max(r.iterations for r in want)
        launches = robot.rrtc_stats()["launches"]
        assert -(-most // sl) <= launches <= -(-most // sl) + 1, (sl, launches, most)
        key = [(r.path.tobytes(), r.iterations, r.size, r.cost) for r in got]
        first = first or key
        assert key == first
    # the default slice is back after a call that chose one
    check_own_scene(vamp, scenes, k, settings, node_cap=256, path_cap=64)
    assert robot.rrtc_stats()["launches"] == 1


# ---- 4. the settings ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(dynamic_domain=False), dict(balance=False), dict(start_tree_first=False),
                                dict(radius=0.5, min_radius=0.2, alpha=0.25)],
                         ids=["no_dynamic_domain", "no_balance", "goal_tree_first", "small_domain"])
def test_settings(vamp, scenes, kw, request):
    """the CPU runs see max_samples = the arena's 512 nodes (balance = 0 grows one tree only, and fast)"""
    case = rc.CASES[request.node.callspec.id]
    assert case.settings == dict(range=1.0, max_iterations=400, max_samples=512, **kw)
    assert case.batches == rc.own((4, 8, 14))
    for k in (4, 8, 14):
        check_own_scene(vamp, scenes, k, case.settings, node_cap=512, path_cap=128)


def test_two_goals(vamp, scenes):
    """n_goals = 2, the second goal another problem's, and in the other order"""
    case = rc.CASES["two_goals"]
    assert [(k, items[0][1][1]) for k, items in case.batches] == [(4, 7), (8, 14), (1, 2)]
    for (k, other), (got, _, _) in zip(((4, 7), (8, 14), (1, 2)), run_case(vamp, scenes, "two_goals")):
        g, g2 = scenes[k][3], scenes[other][3]
        if k == 1:  # the direct connection, whichever goal it is
            assert [r.iterations for r in got] == [0, 0, 0]
            assert got[1].path[1].tobytes() in (g.tobytes(), g2.tobytes())


# ---- 5. EXT: the scene plus a point cloud ---------------------------------------------------------------------------
def test_pointcloud_scene(vamp, scenes):
    case = rc.CASES["pointcloud"]
    assert case.cloud and case.batches == rc.own((1, 4, 8, 14), (1,))
    differs = []
    for k, (_, _, want) in zip((1, 4, 8, 14), run_case(vamp, scenes, "pointcloud")):
        _, plain, s, g = scenes[k]
        differs.append(cpu_run(vamp, vamp.panda_0_0, plain, s, g, case.settings, 1)[0].iterations != want[0].iterations)
    assert any(differs)  # the cloud matters to at least one search


# ---- 5b. the rest of the case table: block counts 2 .. 18, the domain branches, tree_ratio, three goals, a base ----------
# the cases the tests above run in full, with assertions of their own
DEDICATED = ("default", "default-base200", "ragged32", "ragged257", "wide", "iter40", "no_dynamic_domain", "no_balance",
             "goal_tree_first", "small_domain", "two_goals", "pointcloud")


def test_every_case_has_a_test():
    assert set(DEDICATED) <= set(rc.CASES) and len(rc.CASES) > len(DEDICATED)


@pytest.mark.parametrize("name", [n for n in rc.CASES if n not in DEDICATED])
def test_table_case(vamp, scenes, name):
    """one call per scene with its sampler offsets as the batch; the arena holds max_samples nodes, so every
    problem ends DONE"""
    solved = []
    for _, status, want in run_case(vamp, scenes, name):
        assert not status.any(), (name, status)
        solved += [r.solved for r in want]
    # base5: the goals of two scenes are out of reach, those searches run to the bound
    assert all(solved) if name != "base5" else any(solved) and not all(solved), (name, solved)


# ---- 5c. ties of the nearest-neighbour scan ---------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["adjacent", "stride"])
def test_nearest_tie(vamp, scenes, layout):
    """two goals at bitwise equal distance from draw 1 (rrtc_cases.tie_layouts; tests/test_rrtc.py shows that the
    search depends on which one is taken), as one batch of the layout and its reverse: arena nodes 1 and 2 meet in
    the cross-lane reduction (`oi < bi`), nodes 1 and 65 in one lane's stride (`dd < bd`)."""
    goals = np.stack([rc.tie_layouts()[layout], rc.tie_layouts()[layout + "-rev"]])
    _, env, s, _ = scenes[rc.TIE_PROBLEM]
    _, status, want = check_batch(vamp, vamp.panda_0_0, env, np.stack([s, s]), goals, rc.TIE_SETTINGS, 1, tag=layout,
                                  node_cap=rc.TIE_SETTINGS["max_samples"], path_cap=128)
    assert not status.any() and all(r.solved for r in want)
    assert want[0].iterations != want[1].iterations  # the order of the goals decides the search


# ---- 5d. the exact limits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rc.LIMITS))
def test_exact_limits(vamp, scenes, name):
    """path_cap at the path's length L and one below, the arena at the search's node count N and one below (both
    taken from the CPU planner here); `packed` (range 0.1) has the N - 1 cut inside a pass of 8 segments"""
    settings, k, first = rc.LIMITS[name]
    robot = vamp.panda_0_0
    _, env, s, g = scenes[k]
    free, widx = cpu_run(vamp, robot, env, s, g, settings, first)
    assert free.solved
    L, N = len(free.path), sum(free.size)
    assert L > 2 and N > L
    run = dict(starts=[s], goals=[g], settings=settings, firsts=first, tag=name)
    _, status, _ = check_batch(vamp, robot, env, node_cap=512, path_cap=L, **run)
    assert status.tolist() == [robot.RRTC_DONE]
    got, status, idx = robot.rrtc_batch([s], [g], env, vamp.RRTCSettings(**settings), rng_first=first, node_cap=512,
                                        path_cap=L - 1)
    assert status.tolist() == [robot.RRTC_PATH_CAPACITY] and got[0].path_len == L and len(got[0].path) == 0
    assert (got[0].solved, got[0].iterations, tuple(got[0].size), int(idx[0])) == (True, free.iterations, free.size, widx)
    assert np.float32(got[0].cost).view(np.uint32) == np.float32(free.cost).view(np.uint32)
    # the arena as the sample limit: the CPU run with max_samples = node_cap
    _, status, want = check_batch(vamp, robot, env, cpu_settings=dict(settings, max_samples=N), node_cap=N, path_cap=L,
                                  **run)
    assert status.tolist() == [robot.RRTC_DONE] and want[0].solved and want[0].path.tobytes() == free.path.tobytes()
    _, status, want = check_batch(vamp, robot, env, cpu_settings=dict(settings, max_samples=N - 1), node_cap=N - 1,
                                  path_cap=L, **run)
    assert status.tolist() == [robot.RRTC_CAPACITY] and not want[0].solved and sum(want[0].size) == N - 1


# ---- 5e. more problems than a few waves -------------------------------------------------------------------------------------
def test_ragged_batch_of_257(vamp, scenes):
    """P = 257 in problem 4's scene, the 16 start/goal pairs in turn, sampler offsets 1 + 97 p, at most 60
    iterations, 16 per launch: the per-problem strides of the control words, the sampler indices and the arenas, and
    finished problems returning at once over the later launches (check_batch compares every problem and the
    iteration counters with the CPU planner)"""
    case = rc.CASES["ragged257"]
    assert case.gpu == dict(node_cap=128, path_cap=32, slice=16) and case.settings["max_iterations"] == 60
    (got, status, want), = run_case(vamp, scenes, "ragged257")
    assert len(want) == 257 and not status.any()
    assert len({r.iterations for r in want}) >= 3
    assert any(r.solved for r in want) and not all(r.solved for r in want)
    assert vamp.panda_0_0.rrtc_stats()["launches"] >= 4  # 61 iterations at 16 per launch


# ---- 6. the chain: planner output to the simplifier without leaving the device --------------------------------------
def test_device_chain_to_simplify(vamp, scenes):
    import ctypes

    import torch
    from vamp_amd import _lib
    robot = vamp.panda_0_0
    _, env, s, g = scenes[4]
    firsts = [1, 1001, 2001, 3001, 4001]
    P, cap, node_cap = len(firsts), 128, 256
    ds = torch.from_numpy(np.tile(s, (P, 1))).cuda()
    dg = torch.from_numpy(np.tile(g, (P, 1))).cuda()
    di = torch.tensor(firsts, dtype=torch.int64).cuda()  # uint64 words
    dw = torch.zeros((P, cap, 7), dtype=torch.float32).cuda()
    dl = torch.zeros(P, dtype=torch.int32).cuda()
    dr = torch.zeros(P * ctypes.sizeof(_lib.VgpuPlanResult), dtype=torch.uint8).cuda()
    dst = torch.zeros(P, dtype=torch.uint8).cuda()
    it = torch.zeros(P, dtype=torch.int32).cuda()
    cost = torch.zeros(P, dtype=torch.float32).cuda()
    torch.cuda.synchronize()
    robot.rrtc_device(ds.data_ptr(), dg.data_ptr(), 1, P, env, vamp.RRTCSettings(**DEFAULT), di.data_ptr(), node_cap,
                      dw.data_ptr(), cap, dl.data_ptr(), dr.data_ptr(), dst.data_ptr())
    robot.simplify_device(dw.data_ptr(), cap, dl.data_ptr(), P, env, None, it.data_ptr(), 0, cost.data_ptr())
    vamp.context().sync()
    w, ln, it, cost, idx = dw.cpu().numpy(), dl.cpu().numpy(), it.cpu().numpy(), cost.cpu().numpy(), di.cpu().numpy()
    res = (_lib.VgpuPlanResult * P).from_buffer_copy(dr.cpu().numpy().tobytes())
    assert not dst.cpu().numpy().any()
    for k in range(P):
        planned, widx = cpu_run(vamp, robot, env, s, g, DEFAULT, firsts[k])
        assert res[k].solved and res[k].iterations == planned.iterations and int(idx[k]) == widx
        want = robot.simplify(planned.path, env)
        assert ln[k] == len(want.path) and it[k] == want.iterations
        assert w[k, :ln[k]].tobytes() == want.path.tobytes()
        assert cost[k].tobytes() == np.float32(want.cost).tobytes()


# ---- 7. errors ----------------------------------------------------------------------------------------------------------
def test_errors(vamp, scenes):
    _, env, s, g = scenes[4]
    starts, goals = np.tile(s, (3, 1)), np.tile(g, (3, 1))
    settings = vamp.RRTCSettings(**DEFAULT)
    with pytest.raises(vamp.VgpuError, match="unsupported"):
        vamp.fetch.rrtc_batch(np.zeros((2, 8), F), np.zeros((2, 8), F), vamp.Environment())
    attached = vamp.Environment()
    a = vamp.Attachment([0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0])
    a.add_sphere(vamp.Sphere([0.0, 0.0, 0.05], 0.02))
    attached.attach(a)
    with pytest.raises(vamp.VgpuError, match="unsupported"):
        vamp.panda_0_0.rrtc_batch(starts, goals, attached)
    with pytest.raises(vamp.VgpuError, match="invalid argument"):
        vamp.panda_0_0.rrtc_batch(starts, goals, env, settings, rng_first=[1, 0, 1], node_cap=64, path_cap=16)
    with pytest.raises(vamp.VgpuError, match="invalid argument"):  # no room for the start and the goal
        vamp.panda_0_0.rrtc_batch(starts, goals, env, settings, node_cap=1, path_cap=16)
    # a path that does not fit: the CPU's length, no waypoints; a straight connection (problem 1) fits
    hit = 0
    for k in (4, 1):
        _, env, s, g = scenes[k]
        firsts = np.array([1, 1001, 2001], np.uint64)
        got, status, idx = vamp.panda_0_0.rrtc_batch(np.tile(s, (3, 1)), np.tile(g, (3, 1)), env, settings,
                                                     rng_first=firsts, node_cap=256, path_cap=4)
        for j in range(3):
            want, widx = cpu_run(vamp, vamp.panda_0_0, env, s, g, DEFAULT, firsts[j])
            assert got[j].path_len == len(want.path) and got[j].iterations == want.iterations and idx[j] == widx
            if len(want.path) > 4:
                assert status[j] == vamp.Robot.RRTC_PATH_CAPACITY and len(got[j].path) == 0
                hit += 1
            else:
                assert status[j] == vamp.Robot.RRTC_DONE and got[j].path.tobytes() == want.path.tobytes()
    assert 0 < hit < 6
