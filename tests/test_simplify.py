"""Path simplification on the CPU rake (mr-vamp_amd/csrc/cpu/vcpu_simplify.cpp) against a Python restatement of
planning/simplify.hh:192-260 written here: float32 numpy, unfused a + (b - a) * t, the library's vgpu_l2_norm
for distances and the C oracle's validate_motion for every edge.  Nothing but the final comparison calls the
code under test.  Equality is bit for bit: waypoints, length, iterations (and status under a length limit).

The seeded cage paths are also the batched GPU path's cases (tests/test_gpu_simplify.py imports them); the
restatement's trace proves that they exercise a shortcut hit short of the last waypoint, a row without any
valid candidate, accepted and rejected B-spline midpoints, growth beyond twice the input and both outcomes of
the straight-line test -- otherwise the test fails as "inputs too easy".

Section 5 runs the shared case table tests/simplify_cases.py (constructed shortcut rows, long B-spline steps,
exact result lengths, batches of more than 1024 paths, the Fetch, the UR5 and the Baxter) the same way; the trace's
CHUNK_EVENTS prove that those cases reach the second 64-lane chunk of each GPU kernel loop."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_py as op
from conftest import host_fixture
from test_gpu_parity import gpu_env_from_oracle
from test_rrtc import PAIR_BASES, SETTINGS, pair_problems, problem

F = np.float32
BSPLINE, REDUCE, SHORTCUT, PERTURB = 0, 1, 2, 3
LENGTHS = (2, 3, 4, 9, 33, 65, 66, 67)  # 66 and 67: first rows of 64 and 65 candidates (one wave and one more)
BASES = ((0, 0, 0), (200, 200, 0))
SEED = 7


@pytest.fixture(scope="module")
def vamp():
    import vamp_amd
    return vamp_amd


# ---- the restatement ---------------------------------------------------------------------------------------
def l2(v):
    """FloatVector::l2_norm through the library's routine (include/vamp_gpu.h vgpu_l2_norm)"""
    from vamp_amd import _lib
    v = np.ascontiguousarray(v, F)
    return F(_lib.load().vgpu_l2_norm(v.ctypes.data_as(_lib.F32P), v.shape[0]))


def interpolate(a, b, t):
    """interface.hh:422-425: a + (b - a) * t, every operation rounded to float32"""
    return (a + ((b - a).astype(F) * F(t)).astype(F)).astype(F)


def path_cost(p):
    """Path::cost (plan.hh:13-32)"""
    if len(p) < 2:
        return F(np.inf)
    if len(p) == 2:
        return l2((p[1] - p[0]).astype(F))
    c = F(0)
    for i in range(len(p) - 1):
        c = F(c + l2((p[i + 1] - p[i]).astype(F)))
    return c


# what simplify_py counts beyond the original eight keys: the second-chunk branches of the GPU kernels, which
# work in 64-lane chunks with a carry from one chunk to the next (tests/simplify_cases.py states which case
# group has to show which of them)
CHUNK_EVENTS = ("hit_k>=64", "hit_k>=128", "hit_nearest_long", "row_none_over_64", "bs_even_over_64",
                "bs_cand_slot>=64", "bs_accept_slot>=64", "bs_reject_slot>=64", "bs_gap_before_64")


def new_trace():
    """edges: the motions the sequential walk validates; edges_whole: the motions of whole rounds (every
    candidate of a shortcut row, both edges of every B-spline candidate), what a lockstep batch validates;
    rounds: straight-line tests + shortcut rows + B-spline steps; cost_segments: len(result) - 1 of every run"""
    T = dict(hit_inner=0, row_none=0, accepted=0, rejected=0, grew=0, straight_ok=0, straight_fail=0, edges=0,
             edges_whole=0, rounds=0, cost_segments=set())
    T.update({k: 0 for k in CHUNK_EVENTS})
    return T


def merge_trace(into, t):
    for k, v in t.items():
        into[k] = into[k] | v if isinstance(v, set) else into[k] + v
    return into


def simplify_py(path, validate, trace=None, max_iterations=5, operations=(SHORTCUT, BSPLINE), max_steps=1,
                min_change=0.1, midpoint=0.5, max_path_len=0):
    """simplify<Robot, 8, resolution> (simplify.hh:192-260) with shortcut_path (:116-141) and smooth_bspline
    (:14-53).  validate(starts, goals) -> bool array is validate_motion of each edge.  Returns (path, iterations,
    status); trace counts what happened and the edges the sequential walk validates."""
    T = trace if trace is not None else new_trace()
    p = np.ascontiguousarray(path, F).copy()
    n_in = len(p)
    status = 0

    def first_valid(starts, goals):
        """index of the first valid edge in order (the walk stops there), or None"""
        ok = np.asarray(validate(np.asarray(starts, F), np.asarray(goals, F)), bool)
        hit = np.nonzero(ok)[0]
        T["edges"] += int(hit[0]) + 1 if len(hit) else len(ok)
        T["edges_whole"] += len(ok)
        return int(hit[0]) if len(hit) else None

    def shortcut():
        nonlocal p
        if len(p) < 3:
            return False
        result = False
        i = 0
        while i < len(p) - 2:
            js = list(range(len(p) - 1, i + 1, -1))
            k = first_valid([p[i]] * len(js), [p[j] for j in js])
            T["rounds"] += 1
            if k is None:
                T["row_none"] += 1
                T["row_none_over_64"] += len(js) > 64
            else:
                T["hit_inner"] += js[k] != len(p) - 1
                T["hit_k>=64"] += k >= 64
                T["hit_k>=128"] += k >= 128
                # the erase moves the (len - j) waypoints from j on down by j - i - 1 waypoints: by one, and more
                # than a chunk of floats, source and destination overlap inside every chunk
                T["hit_nearest_long"] += js[k] == i + 2 and (len(p) - js[k]) * p.shape[1] > 64
                p = np.concatenate([p[:i + 1], p[js[k]:]])
                result = True
            i += 1
        return result

    def bspline():
        nonlocal p, status
        if len(p) < 3:
            return False
        changed = False
        for _ in range(max_steps):
            if max_path_len and 2 * len(p) - 1 > max_path_len:
                status = 1
                return changed
            q = np.empty((2 * len(p) - 1, p.shape[1]), F)  # Path::subdivide (plan.hh:34-49)
            q[0::2] = p
            for i in range(len(p) - 1):
                q[2 * i + 1] = interpolate(p[i], p[i + 1], 0.5)
            p = q
            updated = False
            T["rounds"] += 1
            evens = range(2, len(p) - 1, 2)
            T["bs_even_over_64"] += len(evens) > 64
            slot, gap_before_64, cand_past_64 = 0, False, False  # slot: the candidate's place in the compact list
            for t, index in enumerate(evens):
                t1 = interpolate(p[index], p[index - 1], midpoint)
                t2 = interpolate(p[index], p[index + 1], midpoint)
                mid = interpolate(t1, t2, 0.5)
                if not l2((mid - p[index]).astype(F)) > F(min_change):
                    gap_before_64 |= t < 64
                    continue
                cand_past_64 |= t >= 64
                ok = np.asarray(validate(np.stack([p[index - 1], mid]), np.stack([mid, p[index + 1]])), bool)
                T["edges"] += 2 if ok[0] else 1
                T["edges_whole"] += 2
                T["bs_cand_slot>=64"] += slot >= 64
                if ok[0] and ok[1]:
                    p[index] = mid
                    changed = updated = True
                    T["accepted"] += 1
                    T["bs_accept_slot>=64"] += slot >= 64
                else:
                    T["rejected"] += 1
                    T["bs_reject_slot>=64"] += slot >= 64
                slot += 1
            T["bs_gap_before_64"] += gap_before_64 and cand_past_64
            if not updated:
                break
        return changed

    iterations = 0
    straight = len(p) == 2
    if len(p) > 2:
        straight = bool(np.asarray(validate(p[:1], p[-1:]), bool)[0])
        T["edges"] += 1
        T["edges_whole"] += 1
        T["rounds"] += 1
        T["straight_ok" if straight else "straight_fail"] += 1
    if straight:
        p = np.stack([p[0], p[-1]])
    elif len(p) > 2:
        run = {SHORTCUT: shortcut, BSPLINE: bspline}
        for _ in range(max_iterations):
            iterations += 1
            any_ = False
            for o in operations:
                any_ |= run[o]()
                if status:
                    break
            if not any_ or status:
                break
    T["grew"] += len(p) > 2 * n_in
    T["cost_segments"].add(len(p) - 1)
    return p, iterations, status


# ---- inputs ----------------------------------------------------------------------------------------------------
def panda_validate(oenv, base):
    return lambda s, g: op.validate_motions(oenv, s, g, base)[0]


def pair_validate(oenv):
    return lambda s, g: op.pair_validate_motions(oenv, s, g, *PAIR_BASES)[0]


@functools.lru_cache(maxsize=None)
def cage_paths(base):
    """Seeded cage-valid Panda paths of every LENGTHS entry: raw uniform configurations, and the same draws
    with each waypoint pulled to within distance 1.0 of its predecessor (kept when still cage-valid).
    Returns [(name, path)]."""
    op.build()
    oenv = op.sphere_cage_env()
    rng = np.random.default_rng(SEED)
    q = op.scale(rng.random((6000, 7), dtype=F))
    q = q[op.fkcc_threads(oenv, q, base)]
    out, at = [], 0
    for n in LENGTHS:
        out.append((f"raw{n}", q[at:at + n].copy()))
        at += n
        w = [q[at]]
        at += 1
        while len(w) < n:
            d = l2((q[at] - w[-1]).astype(F))
            c = interpolate(w[-1], q[at], min(F(1.0), F(1.0) / d)) if d > 0 else q[at]
            at += 1
            if op.fkcc_threads(oenv, c[None], base)[0]:
                w.append(c)
        out.append((f"cap{n}", np.stack(w).astype(F)))
    return out


@functools.lru_cache(maxsize=None)
def cage_expected(base):
    """the restatement's result of every cage path under the default settings: {name: (path, iterations)}, and
    the summed trace"""
    oenv = op.sphere_cage_env()
    T = new_trace()
    exp = {}
    for name, p in cage_paths(base):
        r, it, st = simplify_py(p, panda_validate(oenv, base), T)
        assert st == 0
        exp[name] = (r, it)
    return exp, T


def same_path(got, want):
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def cage_env(vamp):
    return gpu_env_from_oracle(vamp, op.sphere_cage_env())


# ---- 1. the cage paths -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", BASES, ids=["base0", "base200"])
def test_cage_paths_match_restatement(vamp, oracle, base):
    exp, T = cage_expected(base)
    print("trace", base, T)
    # at base (200, 200, 0) the arm stands clear of the cage (every straight line is valid): the conditions are
    # asserted over the whole case set, both bases together
    seen = {k: sum(cage_expected(b)[1][k] for b in BASES) for k in T if k != "cost_segments"}
    easy = [k for k in ("hit_inner", "row_none", "accepted", "rejected", "grew", "straight_ok", "straight_fail")
            if not seen[k]]
    assert not easy, f"inputs too easy: never seen {easy} ({seen})"
    robot = vamp.PandaBase(*base)
    env = cage_env(vamp)
    edges = 0
    for name, p in cage_paths(base):
        res = robot.simplify(p, env, vamp.SimplifySettings(), robot.halton())
        want, it = exp[name]
        assert len(res.path) == len(want) and res.iterations == it, (name, len(res.path), len(want), res.iterations, it)
        assert same_path(res.path, want), name
        assert res.status == 0 and res.solved
        assert np.float32(res.cost).view(np.uint32) == path_cost(want).view(np.uint32), name
        assert np.array_equal(res.path[0], p[0]) and np.array_equal(res.path[-1], p[-1])
        edges += res.validated_edges
    assert edges == T["edges"]  # the walk validates exactly the edges the sequential algorithm does


# ---- 2. planner paths ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table_pick_paths(n_problems=16):
    """the RRT-Connect path of every table_pick problem (each in its own scene): [(oracle env, path)]"""
    import vamp_amd as vamp
    op.build()
    fx = host_fixture("panda_table_pick_problems.npz", op)
    out = []
    for k in range(1, min(int(fx["n_problems"]), n_problems) + 1):
        o, s, g = problem(op, fx, k)
        res = vamp.panda_0_0.rrtc(s, g, gpu_env_from_oracle(vamp, o), vamp.RRTCSettings(**SETTINGS),
                                  vamp.panda_0_0.halton())
        assert res.solved
        out.append((o, res.path))
    return out


def test_table_pick_rrtc_paths(vamp, oracle):
    paths = table_pick_paths()
    assert len(paths) == 16
    for k, (o, p) in enumerate(paths):
        want, it, _ = simplify_py(p, panda_validate(o, (0, 0, 0)))
        res = vamp.panda_0_0.simplify(p, gpu_env_from_oracle(vamp, o))
        assert res.iterations == it and same_path(res.path, want), k
        assert np.array_equal(res.path[0], p[0]) and np.array_equal(res.path[-1], p[-1])


@functools.lru_cache(maxsize=None)
def pair_paths(n=2):
    import vamp_amd as vamp
    op.build()
    o, S, G = pair_problems(op, 6)
    env = gpu_env_from_oracle(vamp, o)
    return o, [vamp.panda_pair.rrtc(S[k], G[k], env, vamp.RRTCSettings(**SETTINGS), vamp.panda_pair.halton()).path
               for k in range(n)]


def test_composite_rrtc_paths(vamp, oracle):
    o, paths = pair_paths()
    env = gpu_env_from_oracle(vamp, o)
    for p in paths:
        assert p.shape[1] == 14 and len(p) > 2
        want, it, _ = simplify_py(p, pair_validate(o))
        res = vamp.panda_pair.simplify(p, env)
        assert res.iterations == it and same_path(res.path, want)
        assert np.float32(res.cost).view(np.uint32) == path_cost(want).view(np.uint32)


# ---- 3. settings ----------------------------------------------------------------------------------------------------
def settings_variants(vamp):
    """(id, SimplifySettings keywords incl. bspline fields, the restatement's keywords)"""
    return [
        ("bspline_first", dict(operations=[BSPLINE, SHORTCUT]), dict(operations=(BSPLINE, SHORTCUT))),
        ("shortcut_only", dict(operations=[SHORTCUT]), dict(operations=(SHORTCUT,))),
        ("bspline_only", dict(operations=[BSPLINE]), dict(operations=(BSPLINE,))),
        ("no_operations", dict(operations=[]), dict(operations=())),
        ("iterations0", dict(max_iterations=0), dict(max_iterations=0)),
        ("iterations1", dict(max_iterations=1), dict(max_iterations=1)),
        ("steps2", dict(max_steps=2), dict(max_steps=2)),
        ("min_change_huge", dict(min_change=1e9), dict(min_change=1e9)),
        ("limit40", dict(max_path_len=40), dict(max_path_len=40)),
    ]


def make_settings(vamp, kw):
    s = vamp.SimplifySettings()
    for k, v in kw.items():
        if k in ("max_steps", "min_change", "midpoint_interpolation"):
            setattr(s.bspline, k, v)
        else:
            setattr(s, k, v)
    return s


def settings_paths():
    """the cage paths the settings variants run on: one that the shortcut collapses and ones that grow"""
    return [(n, p) for n, p in cage_paths((0, 0, 0)) if n in ("raw33", "cap9", "cap33")]


@functools.lru_cache(maxsize=None)
def settings_expected(variant):
    kw = {v[0]: v[2] for v in settings_variants(None)}[variant]
    oenv = op.sphere_cage_env()
    return {n: simplify_py(p, panda_validate(oenv, (0, 0, 0)), **kw) for n, p in settings_paths()}


@pytest.mark.parametrize("variant", [v[0] for v in settings_variants(None)])
def test_settings(vamp, oracle, variant):
    kw = {v[0]: v[1] for v in settings_variants(vamp)}[variant]
    env = cage_env(vamp)
    exp = settings_expected(variant)
    statuses = set()
    for name, p in settings_paths():
        res = vamp.panda_0_0.simplify(p, env, make_settings(vamp, kw))
        want, it, st = exp[name]
        assert (res.iterations, res.status) == (it, st), (name, res.iterations, it, res.status, st)
        assert same_path(res.path, want), name
        statuses.add(st)
        straight = it == 0 and len(want) == 2  # the straight-line test passed: no iteration runs
        if variant == "iterations0":
            assert it == 0 and (straight or same_path(res.path, p))
        if variant == "no_operations":
            assert straight or (it == 1 and same_path(res.path, p))
            statuses.add("looped" if it else "straight")
    if variant == "min_change_huge":
        # nothing is a candidate: the B-spline only subdivides, no midpoint is ever tested against the environment
        T = new_trace()
        for _, p in settings_paths():
            simplify_py(p, panda_validate(op.sphere_cage_env(), (0, 0, 0)), T, min_change=1e9)
        assert T["accepted"] == 0 and T["rejected"] == 0 and T["straight_fail"] > 0
    if variant == "no_operations":
        assert "looped" in statuses
    if variant == "limit40":
        assert statuses == {0, 1}, "the limit must stop a growing path and leave a short one alone"


# ---- 4. unsupported inputs and defaults --------------------------------------------------------------------------------
def test_unsupported_and_defaults(vamp, oracle):
    from vamp_amd import _lib
    lib = _lib.load()
    s = _lib.VgpuSimplifySettings()
    assert lib.vgpu_simplify_settings_default(C.byref(s)) == 0
    assert (s.max_iterations, s.interpolate, s.n_operations, list(s.operations)[:2]) == (5, 0, 2, [SHORTCUT, BSPLINE])
    assert (s.bspline_max_steps, s.max_path_len) == (1, 0)
    assert F(s.bspline_min_change) == F(0.1) and F(s.bspline_midpoint_interpolation) == F(0.5)
    d = vamp.SimplifySettings().c()
    assert bytes(d) == bytes(s)
    assert (vamp.SimplifyRoutine.BSPLINE, vamp.SimplifyRoutine.REDUCE, vamp.SimplifyRoutine.SHORTCUT,
            vamp.SimplifyRoutine.PERTURB) == (0, 1, 2, 3)
    env = cage_env(vamp)
    p = cage_paths((0, 0, 0))[6][1]
    for kw, field in ((dict(operations=[REDUCE]), "REDUCE"), (dict(operations=[SHORTCUT, PERTURB]), "PERTURB"),
                      (dict(interpolate=64), "interpolate")):
        st = make_settings(vamp, kw)
        cs = st.c()
        res = _lib.VgpuPlanResult()
        out = np.empty((64, 7), F)
        rc = lib.vgpu_cpu_simplify(C.byref(vamp.panda_0_0.c_robot), env.host_handle(), p.ctypes.data_as(_lib.F32P),
                                   len(p), C.byref(cs), out.ctypes.data_as(_lib.F32P), 64, C.byref(res), None)
        assert rc == -4
        with pytest.raises(vamp.VgpuError, match=field):
            vamp.panda_0_0.simplify(p, env, st)
    # short inputs come back as they are; the output capacity is reported like vgpu_cpu_rrtc's
    for n in (0, 1, 2):
        res = vamp.panda_0_0.simplify(p[:n], env)
        assert res.iterations == 0 and same_path(res.path, p[:n])
        assert np.float32(res.cost).view(np.uint32) == path_cost(p[:n]).view(np.uint32)
    cs = vamp.SimplifySettings().c()
    res = _lib.VgpuPlanResult()
    exp = cage_expected((0, 0, 0))[0]
    name = max(exp, key=lambda k: len(exp[k][0]))  # the longest result
    assert len(exp[name][0]) > 4
    long = dict(cage_paths((0, 0, 0)))[name]
    rc = lib.vgpu_cpu_simplify(C.byref(vamp.panda_0_0.c_robot), env.host_handle(), long.ctypes.data_as(_lib.F32P),
                               len(long), C.byref(cs), np.empty((4, 7), F).ctypes.data_as(_lib.F32P), 4, C.byref(res),
                               None)
    assert rc == -1 and res.path_len == len(exp[name][0])


# ---- 5. the shared case table (tests/simplify_cases.py): the settings, robots and chunk-boundary paths at which
# tests/test_gpu_simplify.py compares the batch with this function --------------------------------------------------
import simplify_cases as sc  # noqa: E402  (it imports the restatement above)


@pytest.mark.parametrize("group", sc.GROUPS)
def test_case_group_shows_its_events(oracle, group):
    assert {c.group for c in sc.cases().values()} == set(sc.GROUPS)
    print("seen", group, sc.check_group(group))


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_case_table_matches_restatement(vamp, oracle, name):
    case = sc.cases()[name]
    runs, T = sc.restated(name)
    robot, env = sc.product(vamp, case)
    settings = make_settings(vamp, case.cpu_keywords())
    edges = 0
    for (pname, p), (want, it, st, _) in zip(case.paths, runs):
        res = robot.simplify(p, env, settings)
        assert (len(res.path), res.iterations, res.status) == (len(want), it, st), \
            (pname, len(res.path), len(want), res.iterations, it, res.status, st)
        assert same_path(res.path, want), pname
        assert np.float32(res.cost).view(np.uint32) == path_cost(want).view(np.uint32), pname
        edges += res.validated_edges
    assert edges == T["edges"]
