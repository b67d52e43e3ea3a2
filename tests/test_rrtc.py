"""BASELINE configs[0]: Panda RRT-Connect on MotionBenchMaker table_pick problems on the CPU rake
(mr-vamp_amd/csrc/cpu/vcpu_rrtc.cpp, planning/rrtc.hh:33-248), RRTCSettings with range 1.0 and 1e6
iterations/samples (src/vamp/constants.py:1,49-55; src/vamp/__init__.py:80-102), Halton<7> reset per
problem (scripts/evaluate_mbm.py:95-96).

Checks: the straight start -> goal validate_motion of each problem equals the reference-DAG fixture;
the product planner equals an independent Python restatement (tests/rrtc_py.py, oracle
validate_vector) path for path, bit for bit, with the same iterations, tree sizes and cost; every
solved path starts at the start, ends at the goal (to the last increment), and each of its segments passes validate_motion
(oracle) or is one of the planner's own validate_vector-checked extensions.

The same equality holds on every case of tests/rrtc_cases.py -- the settings, goals, bases and scenes at which
tests/test_gpu_rrtc_batch.py compares the GPU batch with this planner --, at the exact sample limits, and on goals
constructed to tie in the nearest-neighbour scan; the restatement's trace shows which branches the table takes."""
import numpy as np
import pytest

import rrtc_cases as rc
import rrtc_py
from conftest import host_fixture
from rrtc_cases import problem  # noqa: F401  (tests/test_gpu_rrtc_batch.py imports it from here)
from test_gpu_parity import gpu_env_from_oracle
from test_oracle import EDGE_MIN_COVERAGE, MARGIN_TEST, fixture_check, same_rsqrt_host, stable

F = np.float32
SETTINGS = dict(range=1.0, max_iterations=1000000, max_samples=1000000)


@pytest.fixture(scope="module")
def vamp():
    import vamp_amd
    return vamp_amd


def test_straight_line_vs_reference_dag(vamp, oracle):
    fx = host_fixture("panda_table_pick_problems.npz", oracle)
    same = same_rsqrt_host(oracle, fx)
    got, ref, keep = [], [], []
    for k in range(1, int(fx["n_problems"]) + 1):
        o, s, g = problem(oracle, fx, k)
        ok, n, _ = vamp.panda_0_0.cpu_validate_batch(s[None], g[None], gpu_env_from_oracle(vamp, o))
        ook, on = oracle.validate_motions(o, s[None], g[None], (0, 0, 0))
        assert ok[0] == ook[0] and n[0] == on[0] == fx[f"p{k}_n"][0]
        got.append(ok[0])
        ref.append(fx[f"p{k}_ok"][0])
        keep.append(stable(fx[f"p{k}_test_margin"], fx[f"p{k}_cull_margin"], same)[0])
    fixture_check("panda table_pick start->goal (CPU rake)", np.array(got), np.array(ref), np.array(keep), same, 0.5)


def test_table_pick_scene_fixture(vamp, oracle):
    """configs[1]'s MBM run: per-configuration masks and edges on
    table_pick scene0001 vs the reference DAG."""
    from test_oracle_robots import scene_env
    fx = host_fixture("panda_table_pick.npz", oracle)
    oenv = scene_env(oracle, fx)
    env = gpu_env_from_oracle(vamp, oenv)
    same = same_rsqrt_host(oracle, fx)
    got = vamp.panda_0_0.cpu_fkcc_batch(fx["q"], env)
    assert np.array_equal(got, oracle.fkcc_threads(oenv, fx["q"], (0, 0, 0)))
    fixture_check("panda fkcc table_pick (CPU rake)", got, fx["valid"], stable(fx["test_margin"], fx["cull_margin"],
                                                                                  same), same)
    ok, n, _ = vamp.panda_0_0.cpu_validate_batch(fx["starts"], fx["goals"], env)
    rok, rn = oracle.validate_motions(oenv, fx["starts"], fx["goals"], (0, 0, 0))
    assert np.array_equal(ok, rok) and np.array_equal(n, rn) and np.array_equal(n, fx["n"])
    fixture_check("panda validate_motion table_pick (CPU rake)", ok, fx["ok"],
                  stable(fx["edge_test_margin"], fx["edge_cull_margin"], same), same, EDGE_MIN_COVERAGE)


@pytest.mark.parametrize("k,base", [(1, (0, 0, 0)), (1, (200, 200, 0)), (2, (0, 0, 0)), (3, (0, 0, 0)),
                                    (4, (0, 0, 0)), (5, (0, 0, 0)), (6, (0, 0, 0))])
def test_rrtc_matches_restatement(vamp, oracle, k, base):
    fx = host_fixture("panda_table_pick_problems.npz", oracle)
    o, s, g = problem(oracle, fx, k)
    env = gpu_env_from_oracle(vamp, o)
    robot = vamp.PandaBase(*base)
    rng = robot.halton()
    res = robot.rrtc(s, g, env, vamp.RRTCSettings(**SETTINGS), rng)
    p, cost, it, sizes, idx = rrtc_py.rrtc("panda", o, s, g, SETTINGS, 1, base)
    assert res.solved and len(p)
    assert res.iterations == it and res.size == sizes and rng.index == idx
    assert np.array_equal(res.path.view(np.uint32), p.view(np.uint32))
    assert np.float32(res.cost).view(np.uint32) == np.float32(cost).view(np.uint32)
    # the ends are the start and goal, or the connect step's last increment onto them (rrtc.hh:213-221
    # walks the other tree from the nearest node's parent)
    assert np.abs(res.path[0] - s).max() <= 1e-5 and np.abs(res.path[-1] - g).max() <= 1e-5
    # segments: collision-free under the planner's own checks (validate_vector with the planner's
    # vector and distance); validate_motion recomputes both from the endpoints, which rakes slightly
    # different interpolants -- so a disagreement is only admissible on a segment that grazes an
    # obstacle.  Counted exactly: every failing segment must have an interpolant within the fixture
    # margin band (MARGIN_TEST) of a contact; on the host the fixtures were made on: exactly 0.
    ok, n = oracle.validate_motions(o, res.path[:-1], res.path[1:], base)
    bad = np.nonzero(~ok.astype(bool))[0]
    for i in bad:
        a, b = res.path[i].astype(np.float64), res.path[i + 1].astype(np.float64)
        t = np.arange(1, 8 * int(n[i]) + 1) / (8.0 * int(n[i]))
        q = (a[None] + (b - a)[None] * t[:, None]).astype(F)
        _, tm, _, _ = oracle.fkcc(o, q, base, stats=True)
        assert np.abs(tm).min() <= MARGIN_TEST, f"segment {i} invalid far from any contact: {np.abs(tm).min()}"
    if same_rsqrt_host(oracle, fx):
        assert len(bad) == 0, f"{len(bad)} near-boundary segment disagreements: {bad}"


def test_rrtc_rng_and_settings(vamp, oracle):
    """a second solve continues the sampler (evaluate_mbm runs trials without reset); max_iterations
    bounds the search; an unsolvable problem reports solved = False."""
    fx = host_fixture("panda_table_pick_problems.npz", oracle)
    o, s, g = problem(oracle, fx, 2)
    env = gpu_env_from_oracle(vamp, o)
    robot = vamp.panda_0_0
    rng = robot.halton()
    r1 = robot.rrtc(s, g, env, vamp.RRTCSettings(**SETTINGS), rng)
    i1 = rng.index
    r2 = robot.rrtc(s, g, env, vamp.RRTCSettings(**SETTINGS), rng)
    p, _, it, _, idx = rrtc_py.rrtc("panda", o, s, g, SETTINGS, i1)
    assert r2.iterations == it and rng.index == idx and np.array_equal(r2.path, p)
    assert r1.solved and r2.solved
    capped = robot.rrtc(s, g, env, vamp.RRTCSettings(range=1.0, max_iterations=3, max_samples=1000), robot.halton())
    assert capped.iterations <= 4
    # the goal inside an obstacle: no path within the iteration budget
    blocked = vamp.Environment()
    blocked.add_sphere(vamp.Sphere([0.0, 0.0, 0.4], 0.6))
    r = robot.rrtc(s, g, blocked, vamp.RRTCSettings(range=1.0, max_iterations=200, max_samples=1000), robot.halton())
    assert not r.solved and r.path.shape == (0, 7) and r.iterations == 201


# ---- the case table of tests/rrtc_cases.py: every setting at which the GPU batch is compared with this planner --------
def planner_run(vamp, env, start, goals, settings, first, base=(0, 0, 0)):
    robot = vamp.PandaBase(*base)
    rng = robot.halton()
    rng.skip(int(first) - 1)
    return robot.rrtc(start, goals, env, vamp.RRTCSettings(**settings), rng), rng.index


def same_as_restatement(res, idx, ref, tag):
    """path and cost bit for bit, iterations, tree sizes, solved and the advanced sampler index; a search that ends
    unsolved (at a bound) is compared like a solved one"""
    p, cost, it, sizes, widx = ref
    assert (res.solved, res.iterations, tuple(res.size), idx) == (len(p) > 0, it, sizes, widx), \
        (tag, res.solved, res.iterations, res.size, idx, len(p), it, sizes, widx)
    assert res.path.shape == p.shape, (tag, res.path.shape, p.shape)
    assert np.array_equal(res.path.view(np.uint32), p.view(np.uint32)), tag
    assert np.float32(res.cost).view(np.uint32) == np.float32(cost).view(np.uint32), (tag, res.cost, cost)


@pytest.mark.parametrize("name", list(rc.CASES))
def test_planner_matches_restatement_on_case(vamp, oracle, name):
    case = rc.CASES[name]
    want, _ = rc.restated(name)
    for b in range(len(case.batches)):
        k, starts, goals, firsts = case.arrays(b)
        env = rc.vamp_env(vamp, k, case.cloud)
        for i in range(len(starts)):
            res, idx = planner_run(vamp, env, starts[i], goals[i], case.settings, firsts[i], case.base)
            same_as_restatement(res, idx, want[b][i], (name, k, i))


def test_case_table_reaches_every_branch(oracle):
    """Conditions of the case table, read from the restatement's trace alone: the table takes every branch the
    GPU planner distinguishes -- block counts per segment that leave rake groups idle (3, 5, 6, 7), fill a pass
    (8), need two passes (9 .. 16) and three (17, 18), packed connects over several passes, failures at the
    head of a pass and behind valid segments, every dynamic-domain branch, both path orientations, trees wider
    than a wave.  Not counted: a failure in the second or later pass of one segment (the oracle's
    validate_vector does not report the failing block)."""
    t = {}
    for name in rc.CASES:
        for key, v in rc.restated(name)[1].items():
            t[key] = t.get(key, 0) + v
    print("merged trace:", sorted(t.items()))
    known = {e for e in rc.EVENTS if "=" not in e}
    assert all(key in known or key.split("=")[0] in ("ext_n", "con_n") for key in t), sorted(t)
    for key in ("dd_reject", "dd_first_shrink", "dd_shrink", "dd_clamp", "dd_grow"):
        assert t.get(key, 0) >= 10, (key, t.get(key, 0))
    for key in ("ext_reach", "ext_clip", "con_multi_pass_packed", "con_fail_first_in_pass", "con_fail_later_in_pass",
                "con_cut_by_cap", "solved_flip", "solved_noflip", "len_b_0", "len_b_pos", "nn_over_64",
                "nn_winner_over_64"):
        assert t.get(key, 0) >= 1, key
    ext = {int(key[6:]) for key in t if key.startswith("ext_n=")}
    con = {int(key[6:]) for key in t if key.startswith("con_n=")}
    assert {1, 2, 3, 4, 6, 9} <= ext and max(ext) >= 17, sorted(ext)
    assert set(range(1, 10)) <= con and con & set(range(10, 17)), sorted(con)
    assert "con_n_ext_0" not in t  # a new node bitwise equal to a node of the other tree: not constructed


@pytest.mark.parametrize("name", list(rc.LIMITS))
def test_exact_limits(vamp, oracle, name):
    """the sample limit at the node count N of a solved search and one below: the planner equals the restatement
    at both; N solves, N - 1 stops in the last connect -- in `packed` between two segments of one pass"""
    settings, k, first = rc.LIMITS[name]
    o, s, g = rc.scene(k)
    env = rc.vamp_env(vamp, k)
    free, idx = planner_run(vamp, env, s, g, settings, first)
    assert free.solved
    same_as_restatement(free, idx, rrtc_py.rrtc("panda", o, s, g, settings, first), (name, "free"))
    N = sum(free.size)
    for limit in (N, N - 1):
        cut = dict(settings, max_samples=limit)
        trace = {}
        want = rrtc_py.rrtc("panda", o, s, g, cut, first, trace=trace)
        res, idx = planner_run(vamp, env, s, g, cut, first)
        same_as_restatement(res, idx, want, (name, limit))
        assert res.solved == (limit == N) and sum(res.size) == limit
        if limit == N:
            assert res.path.tobytes() == free.path.tobytes() and res.iterations == free.iterations
        else:
            assert trace.get("con_cut_by_cap") == 1
            if name == "packed":
                assert trace.get("con_cut_inside_pass") == 1


# ---- the nearest-neighbour tie rule -------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["adjacent", "adjacent-rev", "stride", "stride-rev"])
def test_nearest_tie_takes_the_earliest_node(vamp, oracle, layout):
    """Two goals at bitwise equal distance from the first sample (rrtc_cases.tie_layouts): the planner takes the
    earliest-inserted one, as the restatement's argmin does, and the search depends on it -- the restatement
    with the opposite rule (tie_last) takes another course."""
    goals = rc.tie_layouts()[layout]
    _, s, _ = rc.scene(rc.TIE_PROBLEM)
    want, trace = rc.tie_restated(layout)
    other, _ = rc.tie_restated(layout, True)
    assert trace.get("tie", 0) >= 1
    assert want[2] > 1 and other[2] > 1  # no goal connects to the start directly
    assert (want[2], want[0].tobytes()) != (other[2], other[0].tobytes())
    res, idx = planner_run(vamp, rc.vamp_env(vamp, rc.TIE_PROBLEM), s, goals, rc.TIE_SETTINGS, 1)
    same_as_restatement(res, idx, want, layout)


# ---- BASELINE configs[4]'s planner half: RRT-Connect on the two-Panda composite -------------------------------
PAIR_BASES = ((0, 0, 0), (100, 0, 0))  # vamp_amd.panda_pair: arm A at the origin, arm B 1 m along x


def pair_problems(oracle, n, seed=41):
    """configs[4]'s scene (oracle_py.pair_scene: a table under both arms, three spheres between them) and n
    start/goal composite configurations, collision-free, whose straight validate_motion FAILS (so the planner
    has to search), from seeded uniform draws -- no reference counterpart (SURVEY §0 finding 10): the anchor is
    rrtc.hh:33-248 over the composed validity"""
    o = oracle.pair_scene()
    rng = np.random.default_rng(seed)
    q = oracle.pair_scale(rng.random((40 * n, 14), dtype=F))
    q = q[oracle.pair_fkcc_threads(o, q, *PAIR_BASES)]
    s, g = q[0::2][:8 * n], q[1::2][:8 * n]
    m = min(len(s), len(g))
    ok, _ = oracle.pair_validate_motions(o, s[:m], g[:m], *PAIR_BASES)
    hard = np.nonzero(~ok.astype(bool))[0][:n]
    assert len(hard) == n
    return o, s[hard], g[hard]


@pytest.mark.parametrize("k", range(6))
def test_pair_rrtc_matches_restatement(vamp, oracle, k):
    """vamp_amd.panda_pair.rrtc == the Python restatement over the oracle's composite validate_vector
    (oracle vo_pair_validate_vector), Halton<14> and the two-register l2_norm: path bit for bit, cost,
    iterations, tree sizes, sampler index; every segment of the path passes the oracle's validate_motion."""
    o, S, G = pair_problems(oracle, 6)
    env = gpu_env_from_oracle(vamp, o)
    robot = vamp.panda_pair
    rng = robot.halton()
    res = robot.rrtc(S[k], G[k], env, vamp.RRTCSettings(**SETTINGS), rng)
    p, cost, it, sizes, idx = rrtc_py.rrtc("pair", o, S[k], G[k], SETTINGS, 1, PAIR_BASES)
    assert res.solved and len(p) > 2
    assert res.iterations == it and res.size == sizes and rng.index == idx
    assert np.array_equal(res.path.view(np.uint32), p.view(np.uint32))
    assert np.float32(res.cost).view(np.uint32) == np.float32(cost).view(np.uint32)
    ok, _ = oracle.pair_validate_motions(o, res.path[:-1], res.path[1:], *PAIR_BASES)
    assert ok.all(), np.nonzero(~ok.astype(bool))[0]
