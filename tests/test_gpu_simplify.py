"""Batched path simplification on the GPU (mr-vamp_amd/csrc/vgpu_simplify.hip, vgpu_simplify_paths) against the
sequential CPU function path by path: waypoints bit for bit, length, iterations, status and cost.  The CPU
function itself is pinned to the Python restatement of simplify.hh by tests/test_simplify.py, whose seeded
cage paths (first shortcut rows of 1 to 65 candidates, paths that collapse, paths that grow several-fold) are
the cases here too; one batch holds them all, so paths finish in different rounds and iterations.

The kernels work in 64-lane chunks with a carry from chunk to chunk (the row's first-valid ballots, the erase,
the B-spline candidate compaction, the emit and resolve strides, the 1024-wide scan, the cost sum): sections 10
to 12 run the cases of tests/simplify_cases.py, whose restatement trace proves that the second chunk of each is
entered, on the Panda, the Fetch, the UR5 and the Baxter."""
import numpy as np
import pytest

import oracle_py as op
import simplify_cases as sc
from test_gpu_parity import gpu_env_from_oracle
from test_rrtc import SETTINGS, problem
from test_simplify import (BASES, F, cage_env, cage_paths, make_settings, pair_paths, same_path, settings_paths,
                           settings_variants)
from conftest import host_fixture

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vamp():
    import vamp_amd
    return vamp_amd


def check_batch(vamp, robot, env, paths, settings=None, capacity=None):
    """simplify_batch == simplify path by path (the CPU run limited to `capacity` when one is given); returns the
    status array"""
    settings = settings or vamp.SimplifySettings()
    got, status = robot.simplify_batch(paths, env, settings, capacity=capacity)
    assert len(got) == len(paths) == len(status)
    cpu = make_settings(vamp, dict(max_iterations=settings.max_iterations, operations=list(settings.operations),
                                   max_steps=settings.bspline.max_steps, min_change=settings.bspline.min_change,
                                   midpoint_interpolation=settings.bspline.midpoint_interpolation,
                                   max_path_len=settings.max_path_len))
    if capacity is not None:
        cpu.max_path_len = min(capacity, settings.max_path_len) if settings.max_path_len else capacity
    for k, (p, g) in enumerate(zip(paths, got)):
        want = robot.simplify(p, env, cpu)
        assert (len(g.path), g.iterations, g.status) == (len(want.path), want.iterations, want.status), \
            (k, len(p), len(g.path), len(want.path), g.iterations, want.iterations, g.status, want.status)
        assert same_path(g.path, want.path), (k, len(p))
        assert np.float32(g.cost).view(np.uint32) == np.float32(want.cost).view(np.uint32), (k, g.cost, want.cost)
        assert status[k] == want.status
    return status


# ---- 5. every cage path in one call ---------------------------------------------------------------------------------
@pytest.mark.parametrize("base", BASES, ids=["base0", "base200"])
def test_cage_batch_matches_cpu(vamp, base):
    robot = vamp.PandaBase(*base)
    paths = [p for _, p in cage_paths(base)]
    paths += [np.zeros((0, 7), F), paths[-1][:1]]
    status = check_batch(vamp, robot, cage_env(vamp), paths)
    assert not status.any()
    stats = robot.simplify_stats()
    assert 0 < stats["validate_calls"] <= stats["rounds"] and stats["edges"] > 0


# ---- 6. grid and batch shapes -----------------------------------------------------------------------------------------
def test_single_path_batch(vamp):
    paths = dict(cage_paths((0, 0, 0)))
    for name in ("raw67", "cap9"):
        check_batch(vamp, vamp.panda_0_0, cage_env(vamp), [paths[name]])


def test_many_short_paths(vamp):
    """257 paths of 3 to 9 waypoints: windows of the seeded cage paths"""
    src = [p for _, p in cage_paths((0, 0, 0)) if len(p) >= 33]
    paths = []
    for k in range(257):
        p = src[k % len(src)]
        n = 3 + k % 7
        at = (5 * k) % (len(p) - n)
        paths.append(p[at:at + n].copy())
    check_batch(vamp, vamp.panda_0_0, cage_env(vamp), paths)


def test_capacity_stops_some_paths(vamp):
    """a buffer of 70 waypoints per path (the longest input has 67): the restatement's unlimited results reach 73
    to 85 waypoints on three of the paths, and a path only grows by subdividing, so those must stop with
    VGPU_SIMPLIFY_CAPACITY before the subdivide that would not fit -- exactly where the CPU function stops under
    max_path_len = 70; the paths that collapse to two waypoints finish"""
    from test_simplify import cage_expected
    lens = [len(r) for r, _ in cage_expected((0, 0, 0))[0].values()]
    assert max(lens) > 70 and min(lens) == 2
    paths = [p for _, p in cage_paths((0, 0, 0))]
    status = check_batch(vamp, vamp.panda_0_0, cage_env(vamp), paths, capacity=70)
    assert set(status.tolist()) == {0, 1}, status


# ---- 7. a table_pick scene and the composite ----------------------------------------------------------------------------
def test_table_pick_scene_batch(vamp):
    """one MotionBenchMaker table_pick scene (cuboids; problem 2, whose straight line is blocked so that the
    planner has to search), RRT-Connect paths from different Halton offsets"""
    fx = host_fixture("panda_table_pick_problems.npz", op)
    o, s, g = problem(op, fx, 2)
    assert len(o.cuboids) + len(o.zcuboids) > 0
    env = gpu_env_from_oracle(vamp, o)
    paths = []
    for k in range(10):
        rng = vamp.panda_0_0.halton()
        rng.skip(1000 * k)
        res = vamp.panda_0_0.rrtc(s, g, env, vamp.RRTCSettings(**SETTINGS), rng)
        assert res.solved
        paths.append(res.path)
    assert len({p.tobytes() for p in paths}) >= 8
    check_batch(vamp, vamp.panda_0_0, env, paths)


def test_composite_batch(vamp):
    o, paths = pair_paths()
    assert len(paths) == 2
    check_batch(vamp, vamp.panda_pair, gpu_env_from_oracle(vamp, o), list(paths))


# ---- 8. device pointers; the settings variants ----------------------------------------------------------------------------
def test_device_pointers_match_host_call(vamp):
    import torch
    robot, env = vamp.panda_0_0, cage_env(vamp)
    paths = [p for _, p in cage_paths((0, 0, 0))][:12]
    settings = vamp.SimplifySettings()
    cap = robot.simplify_capacity(max(len(p) for p in paths), settings, len(paths))
    host, status = robot.simplify_batch(paths, env, settings, capacity=cap)
    w = np.zeros((len(paths), cap, 7), F)
    for i, p in enumerate(paths):
        w[i, :len(p)] = p
    dw = torch.from_numpy(w).cuda()
    dl = torch.tensor([len(p) for p in paths], dtype=torch.int32).cuda()  # uint32 words
    it = torch.zeros(len(paths), dtype=torch.int32).cuda()
    st = torch.zeros(len(paths), dtype=torch.uint8).cuda()
    cost = torch.zeros(len(paths), dtype=torch.float32).cuda()
    torch.cuda.synchronize()
    robot.simplify_device(dw.data_ptr(), cap, dl.data_ptr(), len(paths), env, settings, it.data_ptr(), st.data_ptr(),
                          cost.data_ptr())
    vamp.context().sync()
    w2, l2, it2, st2, c2 = dw.cpu().numpy(), dl.cpu().numpy(), it.cpu().numpy(), st.cpu().numpy(), cost.cpu().numpy()
    for i, h in enumerate(host):
        assert l2[i] == len(h.path) and it2[i] == h.iterations and st2[i] == h.status
        assert w2[i, :l2[i]].tobytes() == h.path.tobytes()
        assert c2[i].tobytes() == np.float32(h.cost).tobytes()


@pytest.mark.parametrize("variant", [v[0] for v in settings_variants(None)])
def test_settings_through_the_batch(vamp, variant):
    kw = {v[0]: v[1] for v in settings_variants(vamp)}[variant]
    paths = [p for _, p in settings_paths()]
    status = check_batch(vamp, vamp.panda_0_0, cage_env(vamp), paths, make_settings(vamp, kw))
    if variant == "limit40":
        assert set(status.tolist()) == {0, 1}


# ---- 9. kernel resources ------------------------------------------------------------------------------------------------------
def test_simplify_kernels_do_not_spill():
    from test_kernel_resources import LIB
    import kernel_resources
    ks = [k for k in kernel_resources.kernels(LIB) if "vgpu::simplify_" in k["name"]]
    names = {k["name"].split("(")[0].split("::")[-1] for k in ks}
    assert names == {"simplify_init_kernel", "simplify_prepare_kernel", "simplify_scan_kernel", "simplify_emit_kernel",
                     "simplify_resolve_kernel", "simplify_finish_kernel"}, names
    bad = [(k["name"][:80], k["vgpr"], k["vgpr_spill"], k["scratch"]) for k in ks if k["scratch"] or k["vgpr_spill"]]
    assert not bad, bad


# ---- 10. the shared case table (tests/simplify_cases.py): second chunks of every 64-lane loop ---------------------------------
def case_batch(vamp, name):
    """(robot, environment, paths, settings, capacity) of a case"""
    case = sc.cases()[name]
    robot, env = sc.product(vamp, case)
    return robot, env, [p for _, p in case.paths], make_settings(vamp, case.settings), case.capacity


def check_case(vamp, name, singles=False):
    """the case as one batch (its paths finish in different rounds) and, with `singles`, every path alone"""
    robot, env, paths, settings, capacity = case_batch(vamp, name)
    status = check_batch(vamp, robot, env, paths, settings, capacity)
    assert status.tolist() == [st for _, _, st, _ in sc.restated(name)[0]]
    for p in paths if singles else ():
        check_batch(vamp, robot, env, [p], settings, capacity)


def test_constructed_shortcut_rows(vamp):
    """rows whose first valid candidate is at position 0 .. 128 (the last of its row, or with valid and invalid
    ones after it) and rows of 64, 65 and 129 candidates without one: the ballot loop's k0, its break, the
    overlapping erase"""
    seen = sc.check_group("rows")
    assert seen["hit_k>=64"] and seen["hit_k>=128"] and seen["hit_nearest_long"] and seen["row_none_over_64"]
    check_case(vamp, "rows", singles=True)


@pytest.mark.parametrize("name", ["bspline_only", "bspline_first-steps1", "bspline_first-steps2"])
def test_long_bspline_steps(vamp, name):
    """B-spline steps of more than 64 even indices with non-candidates among the first 64: the compaction's base,
    candidate slots, emit and resolve iterations past 64"""
    seen = sc.check_group("bspline")
    assert seen["bs_accept_slot>=64"] and seen["bs_reject_slot>=64"] and seen["bs_gap_before_64"]
    check_case(vamp, name, singles=True)


@pytest.mark.parametrize("name", ["cost_pass", "cost_subdivide"])
def test_cost_chunk_edges(vamp, name):
    """results of 64, 65, 66, 128 and 129 waypoints: the cost sum's last chunk one short of full, full, and one
    segment into the next"""
    sc.check_group("cost")
    check_case(vamp, name, singles=True)


@pytest.mark.parametrize("robot", sorted(sc.ROBOT_FIXTURES))
def test_other_robots(vamp, robot):
    """Fetch (dim 8: all eight lanes of the one-register distance), UR5 (dim 6), Baxter (dim 14, resolution 64)"""
    sc.check_group(robot)
    assert getattr(vamp, robot).dimension() == op.ROBOTS[robot][1]
    check_case(vamp, f"{robot}-default")
    check_case(vamp, f"{robot}-bspline")


# ---- 11. more paths than the scan's block ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sc.MANY)
def test_more_paths_than_a_scan_block(vamp, n):
    """1023 .. 2049 paths, some idle from the start, a 129-candidate row at index 1024 and at the end.  The batch
    validates whole rounds: exactly the restatement's edges_whole (every candidate of a row, both edges of every
    B-spline candidate), which is at least the sequential walk's count; and it takes the rounds of its slowest
    path, however many paths there are."""
    sc.check_group("many")
    name = f"many{n}"
    robot, env, paths, settings, capacity = case_batch(vamp, name)
    assert len(paths) == n
    runs, T = sc.restated(name)
    check_case(vamp, name)
    stats = robot.simplify_stats()
    print("stats", n, stats, "sequential edges", T["edges"], "whole rounds", T["edges_whole"])
    assert stats["edges"] == T["edges_whole"] >= T["edges"]
    assert 0 < stats["validate_calls"] <= stats["rounds"]
    slow = sc.slowest(name)
    assert stats["rounds"] == runs[slow][3]["rounds"]
    check_batch(vamp, robot, env, [paths[slow]], settings, capacity)
    alone = robot.simplify_stats()
    assert stats["rounds"] <= alone["rounds"], (stats, alone)


def test_workspace_regrows_and_is_reused(vamp):
    """2049 paths, then one path with a capacity that outgrows the context's workspace, then the 2049 again in the
    larger workspace over the first call's leftovers: all three equal the CPU"""
    robot, env, paths, settings, capacity = case_batch(vamp, "many2049")
    check_batch(vamp, robot, env, paths, settings, capacity)
    first = robot.simplify_stats()
    one = dict(cage_paths((0, 0, 0)))["cap9"]
    check_batch(vamp, robot, env, [one], settings, 2 * len(paths) * capacity)
    check_batch(vamp, robot, env, paths, settings, capacity)
    assert robot.simplify_stats() == first


# ---- 12. device pointers: a path longer than the capacity, absent outputs -------------------------------------------------------
def test_device_length_over_capacity_and_null_outputs(vamp):
    import torch
    robot, env = vamp.panda_0_0, cage_env(vamp)
    named = dict(cage_paths((0, 0, 0)))
    a, b = named["cap9"], named["raw33"]
    settings = vamp.SimplifySettings()
    cap = 70
    host, hstatus = robot.simplify_batch([a, b], env, settings, capacity=cap)
    w = np.zeros((3, cap, 7), F)
    w[0, :len(a)], w[2, :len(b)] = a, b
    w[1] = np.arange(cap * 7, dtype=F).reshape(cap, 7)  # len[1] = cap + 5: nothing of it may be read or written
    lens = [len(a), cap + 5, len(b)]

    def run(with_it=True, with_st=True, with_cost=True):
        dw = torch.from_numpy(w).cuda()
        dl = torch.tensor(lens, dtype=torch.int32).cuda()  # uint32 words
        it = torch.full((3,), -7, dtype=torch.int32).cuda()
        st = torch.full((3,), 99, dtype=torch.uint8).cuda()
        cost = torch.full((3,), -7.0, dtype=torch.float32).cuda()
        torch.cuda.synchronize()
        robot.simplify_device(dw.data_ptr(), cap, dl.data_ptr(), 3, env, settings, it.data_ptr() if with_it else 0,
                              st.data_ptr() if with_st else 0, cost.data_ptr() if with_cost else 0)
        vamp.context().sync()
        return dw.cpu().numpy(), dl.cpu().numpy(), it.cpu().numpy(), st.cpu().numpy(), cost.cpu().numpy()

    for absent in (None, "it", "st", "cost"):
        w2, l2, it2, st2, c2 = run(absent != "it", absent != "st", absent != "cost")
        assert l2[1] == cap + 5 and w2[1].tobytes() == w[1].tobytes()
        for i, h in ((0, host[0]), (2, host[1])):
            assert l2[i] == len(h.path) and w2[i, :l2[i]].tobytes() == h.path.tobytes()
        want = dict(it=[host[0].iterations, 0, host[1].iterations],
                    st=[host[0].status, 1, host[1].status],  # 1: VGPU_SIMPLIFY_CAPACITY
                    cost=np.array([host[0].cost, np.inf, host[1].cost], F))
        untouched = dict(it=[-7] * 3, st=[99] * 3, cost=np.full(3, -7.0, F))
        for key, got in (("it", it2), ("st", st2), ("cost", c2)):
            exp = untouched[key] if absent == key else want[key]
            assert np.asarray(got).tobytes() == np.asarray(exp, got.dtype).tobytes(), (absent, key, got, exp)
