"""Batched RRT-Connect across scenes (vgpu_rrtc_batch_scenes, Robot.rrtc_batch_scenes: one call, one wave per
problem, each problem naming its environment) against the CPU planner problem by problem.

The reference throughout is Robot.rrtc (vgpu_cpu_rrtc) run in THAT problem's environment with the same rng_first,
and the comparison is tests/test_gpu_rrtc_batch.py's same_result: solved, iterations, tree sizes, the path's bits,
the cost's bits and the advanced rng index.  There are no tolerances.

The 16 table_pick problems of the fixture each come with their own scene, which is the shape this call exists for:
test 1 runs all of them in one call.  Settings come from tests/rrtc_cases.py (the `default` case, which
tests/test_rrtc.py pins to the restatement); arenas are node_cap = 256, path_cap = 64 unless a test is about them."""
import ctypes

import numpy as np
import pytest

import oracle_py as op
import rrtc_cases as rc
from conftest import host_fixture
from test_gpu_parity import gpu_env_from_oracle
from test_gpu_rrtc_batch import cpu_run, same_result
from test_rrtc import problem

pytestmark = pytest.mark.gpu
F = np.float32
DEFAULT = rc.CASES["default"].settings
CAPS = dict(node_cap=256, path_cap=64)
OFFSETS = (1, 1001)
# foreign-scene runs (the sensitivity condition) stop here: a start or goal may be in collision in another scene.
# Every own-scene search from a fresh sampler ends sooner (asserted), so the bound changes no result it is compared to.
FOREIGN_BOUND = 300


@pytest.fixture(scope="module")
def vamp():
    import vamp_amd
    return vamp_amd


@pytest.fixture(scope="module")
def table(vamp):
    """problem k -> (vamp environment, start, goal)"""
    fx = host_fixture("panda_table_pick_problems.npz", op)
    assert int(fx["n_problems"]) == 16
    out = {}
    for k in range(1, 17):
        o, s, g = problem(op, fx, k)
        out[k] = (gpu_env_from_oracle(vamp, o), s.astype(F), g.astype(F))
    return out


@pytest.fixture(scope="module")
def own(vamp, table):
    """(k, first) -> (CPU result, advanced index) of problem k in its own scene, default settings; computed once,
    nobody writes to it"""
    return {(k, f): cpu_run(vamp, vamp.panda_0_0, table[k][0], table[k][1], table[k][2], DEFAULT, f)
            for f in OFFSETS for k in range(1, 17)}


def all32(table):
    """test 1's batch: the 16 problems at offset 1, then at offset 1001; problem k names environment k - 1"""
    ks = [k for _ in OFFSETS for k in range(1, 17)]
    firsts = np.array([f for f in OFFSETS for _ in range(1, 17)], np.uint64)
    starts = np.stack([table[k][1] for k in ks])
    goals = np.stack([table[k][2] for k in ks])
    envs = [table[k][0] for k in range(1, 17)]
    return ks, firsts, starts, goals, envs, np.array([k - 1 for k in ks], np.uint32)


def extra_spheres(vamp, env, n):
    """n small spheres three metres away, out of the arm's reach: records that change the scene's shape (near sets,
    clearance grid) and none of its searches"""
    for i in range(n):
        env.add_sphere(vamp.Sphere([3.0, -1.5 + 0.01 * i, 2.5], 0.004))
    return env


# ---- 1. all 16 problems, each in its own scene, one call -------------------------------------------------------------
def test_all_problems_in_one_call(vamp, table, own):
    robot = vamp.panda_0_0
    ks, firsts, starts, goals, envs, index = all32(table)
    got, status, idx = robot.rrtc_batch_scenes(starts, goals, envs, index, vamp.RRTCSettings(**DEFAULT),
                                               rng_first=firsts, **CAPS)
    assert len(got) == len(status) == len(idx) == 32 and not status.any()
    for p, k in enumerate(ks):
        want, widx = own[k, int(firsts[p])]
        same_result(got[p], idx[p], want, widx, (k, int(firsts[p])))
        assert got[p].nanoseconds == 0
    stats = robot.rrtc_stats()
    assert stats["iterations"] == sum(r.iterations for r, _ in own.values())
    most = max(r.iterations for r, _ in own.values())
    assert stats["max_iterations"] == most
    assert -(-most // 256) <= stats["launches"] <= -(-most // 256) + 1  # ONE call; the default slice is 256
    # env_index defaults to 0 .. P - 1 with one environment per problem
    got16, _, idx16 = robot.rrtc_batch_scenes(starts[:16], goals[:16], envs, settings=vamp.RRTCSettings(**DEFAULT),
                                              **CAPS)
    for p in range(16):
        same_result(got16[p], idx16[p], *own[p + 1, 1], tag=("default index", p + 1))


def test_the_scene_decides_the_search(vamp, table, own):
    """the condition that makes test 1 sensitive to env_index: on the CPU, at least half of the 16 problems take
    another course in the NEXT problem's scene than in their own, so a kernel that ignored the index (or used
    another problem's) could not produce test 1's results"""
    assert max(own[k, 1][0].iterations for k in range(1, 17)) < FOREIGN_BOUND
    bounded = dict(DEFAULT, max_iterations=FOREIGN_BOUND)
    differ = 0
    for k in range(1, 17):
        foreign, _ = cpu_run(vamp, vamp.panda_0_0, table[k % 16 + 1][0], table[k][1], table[k][2], bounded, 1)
        mine = own[k, 1][0]
        differ += (foreign.iterations, foreign.path.tobytes()) != (mine.iterations, mine.path.tobytes())
    assert differ >= 8, differ


# ---- 2. unordered and shared indices ---------------------------------------------------------------------------------
def test_unordered_and_shared_indices(vamp, table, own):
    """P = 19 over 6 list entries: entries 0 and 2 are the SAME Environment object (scene 3), entry 3 (scene 12) is
    named by nobody, entries 0 / 2 and 4 are shared by several problems, and the order follows neither the list nor
    the problems"""
    robot = vamp.panda_0_0
    scenes_of = [3, 7, 3, 12, 9, 5]
    envs = [table[k][0] for k in scenes_of]
    assert envs[0] is envs[2]
    index = np.array([4, 1, 0, 5, 2, 4, 1, 5, 0, 2, 4, 1, 2, 5, 0, 4, 1, 0, 5], np.uint32)
    assert len(index) == 19 and 3 not in index and set(index.tolist()) == {0, 1, 2, 4, 5}
    firsts = np.array([OFFSETS[(p // 3) % 2] for p in range(19)], np.uint64)
    ks = [scenes_of[e] for e in index]
    got, status, idx = robot.rrtc_batch_scenes(np.stack([table[k][1] for k in ks]), np.stack([table[k][2] for k in ks]),
                                               envs, index, vamp.RRTCSettings(**DEFAULT), rng_first=firsts, **CAPS)
    assert not status.any()
    for p, k in enumerate(ks):
        same_result(got[p], idx[p], *own[k, int(firsts[p])], tag=(p, k))
    assert len({(k, int(f)) for k, f in zip(ks, firsts)}) >= 8  # not one search many times over


# ---- 3. scenes that differ in shape, in one launch -------------------------------------------------------------------
def test_scenes_of_different_shape(vamp, table, own):
    """(a) no obstacle at all, (b) a fixture scene, (c) the scene plus far spheres beyond the near sets' 64 records,
    (d) beyond the clearance grid's 256 records, (e) a scene with a point cloud, which makes the launch an EXT one
    with primitive-only scenes in it"""
    robot = vamp.panda_0_0
    k = 4
    _, s, g = table[k]
    n_records = len(rc.scene(k)[0].spheres) + len(rc.scene(k)[0].capsules) + len(rc.scene(k)[0].zcapsules) + \
        len(rc.scene(k)[0].cuboids) + len(rc.scene(k)[0].zcuboids)
    assert 0 < n_records <= 64
    c_env = extra_spheres(vamp, gpu_env_from_oracle(vamp, rc.scene(k)[0]), 65 - n_records)      # 65 records
    d_env = extra_spheres(vamp, gpu_env_from_oracle(vamp, rc.scene(k)[0]), 257 - n_records)     # 257 records
    envs = [vamp.Environment(), table[k][0], c_env, d_env, rc.vamp_env(vamp, 14, cloud=True)]
    e_s, e_g = rc.scene(14)[1], rc.scene(14)[2]
    # two offsets per scene, the scenes interleaved
    index = np.array([0, 1, 2, 3, 4, 4, 3, 2, 1, 0], np.uint32)
    firsts = np.array([1] * 5 + [1001] * 5, np.uint64)
    starts = np.stack([e_s if e == 4 else s for e in index])
    goals = np.stack([e_g if e == 4 else g for e in index])
    settings = dict(DEFAULT, max_iterations=400)  # the pointcloud case's bound
    want = [cpu_run(vamp, robot, envs[e], starts[p], goals[p], settings, firsts[p]) for p, e in enumerate(index)]
    got, status, idx = robot.rrtc_batch_scenes(starts, goals, envs, index, vamp.RRTCSettings(**settings),
                                               rng_first=firsts, **CAPS)
    assert not status.any()
    for p in range(10):
        same_result(got[p], idx[p], *want[p], tag=(p, int(index[p])))
    assert got[0].iterations == 0 and len(got[0].path) == 2      # (a): the straight line
    assert want[1][0].iterations > 1                                # (b): a search
    assert want[4][0].iterations != own[14, 1][0].iterations        # (e): the cloud decides this search
    for p in (2, 3):                                                # (c), (d): the far spheres change nothing
        assert got[p].path.tobytes() == got[1].path.tobytes() and got[p].iterations == got[1].iterations
    # (b) in a launch without (e): the primitive kernel gives the same bits as the EXT kernel gave
    sel = [p for p in range(10) if index[p] != 4]
    got2, status2, idx2 = robot.rrtc_batch_scenes(starts[sel], goals[sel], envs[:4], index[sel],
                                                  vamp.RRTCSettings(**settings), rng_first=firsts[sel], **CAPS)
    assert not status2.any()
    for j, p in enumerate(sel):
        same_result(got2[j], idx2[j], got[p], idx[p], tag=("primitive launch", p))


# ---- 4. slices and resumption ----------------------------------------------------------------------------------------
def test_slices(vamp, table, own):
    robot = vamp.panda_0_0
    ks, firsts, starts, goals, envs, index = all32(table)
    got, status, idx = robot.rrtc_batch_scenes(starts, goals, envs, index, vamp.RRTCSettings(**DEFAULT),
                                               rng_first=firsts, slice=16, **CAPS)
    most = max(r.iterations for r, _ in own.values())
    launches = robot.rrtc_stats()["launches"]
    assert most > 16 and launches > 1 and -(-most // 16) <= launches <= -(-most // 16) + 1, (most, launches)
    assert not status.any()
    for p, k in enumerate(ks):
        same_result(got[p], idx[p], *own[k, int(firsts[p])], tag=(k, int(firsts[p])))
    # the default slice is back after a call that chose one
    robot.rrtc_batch_scenes(starts, goals, envs, index, vamp.RRTCSettings(**DEFAULT), rng_first=firsts, **CAPS)
    assert robot.rrtc_stats()["launches"] <= -(-most // 256) + 1 < launches


# ---- 5. the caps at their edge in a mixed call -----------------------------------------------------------------------
def test_caps_at_their_edge(vamp, table, own):
    """the problem with the most nodes (N) and the one with the longest path (L) of the 16: node_cap = N - 1 stops
    that problem alone with RRTC_CAPACITY (the CPU run with max_samples = N - 1), path_cap = L - 1 leaves that
    problem alone with RRTC_PATH_CAPACITY, and every other scene's problem is what it was"""
    robot = vamp.panda_0_0
    ks = list(range(1, 17))
    nodes = {k: sum(own[k, 1][0].size) for k in ks}
    lens = {k: len(own[k, 1][0].path) for k in ks}
    kn, kl = max(ks, key=nodes.get), max(ks, key=lens.get)
    N, L = nodes[kn], lens[kl]
    assert sorted(nodes.values())[-2] < N - 1 and sorted(lens.values())[-2] <= L - 1 and L > 2, (nodes, lens)
    starts, goals = np.stack([table[k][1] for k in ks]), np.stack([table[k][2] for k in ks])
    envs = [table[k][0] for k in ks]
    settings = vamp.RRTCSettings(**DEFAULT)
    # the arena one node short
    got, status, idx = robot.rrtc_batch_scenes(starts, goals, envs, settings=settings, node_cap=N - 1, path_cap=64)
    assert status.tolist() == [robot.RRTC_CAPACITY if k == kn else robot.RRTC_DONE for k in ks]
    capped = cpu_run(vamp, robot, table[kn][0], table[kn][1], table[kn][2], dict(DEFAULT, max_samples=N - 1), 1)
    assert not capped[0].solved and sum(capped[0].size) == N - 1
    for p, k in enumerate(ks):
        same_result(got[p], idx[p], *(capped if k == kn else own[k, 1]), tag=("node_cap", k))
    # the path one waypoint short
    got, status, idx = robot.rrtc_batch_scenes(starts, goals, envs, settings=settings, node_cap=256, path_cap=L - 1)
    assert status.tolist() == [robot.RRTC_PATH_CAPACITY if k == kl else robot.RRTC_DONE for k in ks]
    for p, k in enumerate(ks):
        want, widx = own[k, 1]
        if k != kl:
            same_result(got[p], idx[p], want, widx, tag=("path_cap", k))
            continue
        assert got[p].path_len == L and len(got[p].path) == 0
        assert (got[p].solved, got[p].iterations, tuple(got[p].size), int(idx[p])) == \
            (True, want.iterations, tuple(want.size), widx)
        assert np.float32(got[p].cost).view(np.uint32) == np.float32(want.cost).view(np.uint32)


# ---- 6. the chain: planner output to the simplifier without leaving the device ---------------------------------------
def test_device_chain_to_simplify(vamp, table, own):
    """problems sorted by scene: each scene's paths are a contiguous sub-range, which simplify_device takes with
    offset pointers"""
    import torch
    from vamp_amd import _lib
    robot = vamp.panda_0_0
    order = [(4, 1), (4, 1001), (8, 1), (8, 1001)]  # (scene, offset), sorted by scene
    envs = [table[4][0], table[8][0]]
    P, cap, node_cap = 4, 64, 256
    ds = torch.from_numpy(np.stack([table[k][1] for k, _ in order])).cuda()
    dg = torch.from_numpy(np.stack([table[k][2] for k, _ in order])).cuda()
    de = torch.tensor([0, 0, 1, 1], dtype=torch.int32).cuda()  # uint32 words
    di = torch.tensor([f for _, f in order], dtype=torch.int64).cuda()  # uint64 words
    dw = torch.zeros((P, cap, 7), dtype=torch.float32).cuda()
    dl = torch.zeros(P, dtype=torch.int32).cuda()
    dr = torch.zeros(P * ctypes.sizeof(_lib.VgpuPlanResult), dtype=torch.uint8).cuda()
    dst = torch.zeros(P, dtype=torch.uint8).cuda()
    it = torch.zeros(P, dtype=torch.int32).cuda()
    cost = torch.zeros(P, dtype=torch.float32).cuda()
    torch.cuda.synchronize()
    robot.rrtc_scenes_device(ds.data_ptr(), dg.data_ptr(), 1, P, envs, de.data_ptr(), vamp.RRTCSettings(**DEFAULT),
                             di.data_ptr(), node_cap, dw.data_ptr(), cap, dl.data_ptr(), dr.data_ptr(), dst.data_ptr())
    for j, env in enumerate(envs):  # scene j's problems: 2 j and 2 j + 1
        robot.simplify_device(dw.data_ptr() + 2 * j * cap * 7 * 4, cap, dl.data_ptr() + 2 * j * 4, 2, env, None,
                              it.data_ptr() + 2 * j * 4, 0, cost.data_ptr() + 2 * j * 4)
    vamp.context().sync()
    w, ln, it, cost, idx = dw.cpu().numpy(), dl.cpu().numpy(), it.cpu().numpy(), cost.cpu().numpy(), di.cpu().numpy()
    res = (_lib.VgpuPlanResult * P).from_buffer_copy(dr.cpu().numpy().tobytes())
    assert not dst.cpu().numpy().any()
    for p, (k, f) in enumerate(order):
        planned, widx = own[k, f]
        assert res[p].solved and res[p].iterations == planned.iterations and int(idx[p]) == widx
        want = robot.simplify(planned.path, table[k][0])
        assert ln[p] == len(want.path) and it[p] == want.iterations
        assert w[p, :ln[p]].tobytes() == want.path.tobytes()
        assert cost[p].tobytes() == np.float32(want.cost).tobytes()


# ---- 7. errors -------------------------------------------------------------------------------------------------------
def test_errors(vamp, table, own):
    import torch
    from vamp_amd import _lib
    robot = vamp.panda_0_0
    ks = [4, 8, 14]
    envs = [table[k][0] for k in ks]
    starts, goals = np.stack([table[k][1] for k in ks]), np.stack([table[k][2] for k in ks])
    settings = vamp.RRTCSettings(**DEFAULT)

    def good_call():
        got, status, idx = robot.rrtc_batch_scenes(starts, goals, envs, settings=settings, **CAPS)
        for p, k in enumerate(ks):
            same_result(got[p], idx[p], *own[k, 1], tag=("after an error", k))

    # an index equal to n_envs: the host path refuses it before any launch ...
    with pytest.raises(vamp.VgpuError, match="invalid argument.*env_index"):
        robot.rrtc_batch_scenes(starts, goals, envs, [0, 3, 2], settings, **CAPS)
    # ... the device path finds it in the kernel, which runs no search for that problem and reads no view
    P, cap = 3, 64
    ds, dg = torch.from_numpy(starts).cuda(), torch.from_numpy(goals).cuda()
    de = torch.tensor([0, 3, 2], dtype=torch.int32).cuda()
    di = torch.ones(P, dtype=torch.int64).cuda()
    dw = torch.zeros((P, cap, 7), dtype=torch.float32).cuda()
    dl = torch.zeros(P, dtype=torch.int32).cuda()
    dr = torch.zeros(P * ctypes.sizeof(_lib.VgpuPlanResult), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    with pytest.raises(vamp.VgpuError, match="invalid argument.*env_index"):
        robot.rrtc_scenes_device(ds.data_ptr(), dg.data_ptr(), 1, P, envs, de.data_ptr(), settings, di.data_ptr(), 256,
                                 dw.data_ptr(), cap, dl.data_ptr(), dr.data_ptr())
    vamp.context().sync()
    assert int(di.cpu()[1]) == 1 and int(dl.cpu()[1]) == 0  # the refused problem drew nothing and wrote nothing
    good_call()
    # an attached environment in the list
    attached = vamp.Environment()
    a = vamp.Attachment([0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0])
    a.add_sphere(vamp.Sphere([0.0, 0.0, 0.05], 0.02))
    attached.attach(a)
    with pytest.raises(vamp.VgpuError, match="unsupported"):
        robot.rrtc_batch_scenes(starts, goals, [envs[0], attached, envs[2]], settings=settings, **CAPS)
    # an environment of another context
    other = vamp.Context(0)
    stray = vamp.Environment()
    stray.add_sphere(vamp.Sphere([3.0, 0.0, 2.5], 0.01))
    try:
        handles = (ctypes.c_void_p * 3)(envs[0].handle(vamp.context()), stray.handle(other),
                                        envs[2].handle(vamp.context()))
        index = np.arange(3, dtype=np.uint32)
        idx = np.ones(3, np.uint64)
        paths, ln = np.zeros((3, cap, 7), F), np.zeros(3, np.uint32)
        res = (_lib.VgpuPlanResult * 3)()
        cs = settings.c()
        rc_ = _lib.load().vgpu_rrtc_batch_scenes_host(
            vamp.context().h, ctypes.byref(robot.c_robot), handles, 3, index.ctypes.data_as(_lib.U32P),
            starts.ctypes.data_as(_lib.F32P), goals.ctypes.data_as(_lib.F32P), 1, 3, ctypes.byref(cs),
            idx.ctypes.data_as(_lib.U64P), 256, paths.ctypes.data_as(_lib.F32P), cap, ln.ctypes.data_as(_lib.U32P), res,
            None)
        assert rc_ == -1 and idx.tolist() == [1, 1, 1]  # VGPU_ERR_INVALID_ARG, nothing ran
    finally:
        stray._changed()  # drops the copy realised on the other context, which then goes
        other.close()
    # no environment; a robot that is not the Panda
    with pytest.raises(vamp.VgpuError, match="invalid argument"):
        robot.rrtc_batch_scenes(starts, goals, [], [0, 0, 0], settings, **CAPS)
    with pytest.raises(vamp.VgpuError, match="unsupported"):
        vamp.fetch.rrtc_batch_scenes(np.zeros((2, 8), F), np.zeros((2, 8), F), [vamp.Environment()], [0, 0])
    # rng_first = 0 is refused as in rrtc_batch
    with pytest.raises(vamp.VgpuError, match="invalid argument"):
        robot.rrtc_batch_scenes(starts, goals, envs, settings=settings, rng_first=[1, 0, 1], **CAPS)
    # P = 0: empty results
    got, status, idx = robot.rrtc_batch_scenes(np.zeros((0, 7), F), np.zeros((0, 7), F), envs[:1], [], settings)
    assert got == [] and len(status) == 0 and len(idx) == 0
    good_call()
