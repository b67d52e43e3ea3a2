"""Path-simplification cases shared by tests/test_simplify.py (Robot.simplify on the CPU against the restatement
simplify_py) and tests/test_gpu_simplify.py (simplify_batch against Robot.simplify), so that every setting at
which the GPU is compared with the CPU function is one at which the CPU function is pinned to the restatement.

Plain numpy and the oracle; nothing here needs a GPU.  The kernels of vgpu_simplify.hip work in 64-lane chunks
with a carry from one chunk to the next; the cases are built so that the second chunk of each of them runs, and
the restatement's trace (test_simplify.CHUNK_EVENTS) proves that it did: check_group(group) fails as "inputs too
easy" when a group never showed an event it exists for.

A Case is a name, its group, a robot, a base, the SimplifySettings keywords (as test_simplify.make_settings takes
them), the waypoint capacity of the batch call (None: Robot.simplify_capacity's default; otherwise the CPU
function and the restatement run under max_path_len = capacity, where the batch stops a path) and paths
[(name, [n, dim] float32)].  One case is one batch: its paths finish in different rounds.

    rows       Panda in the 14-sphere cage, SHORTCUT only.  A is a cage-valid waypoint, `good` / `bad` the
               cage-valid draws q whose motion A -> q is valid / invalid.
               first{k}   [A, x, g, b_k-1 .. b_0]: row 0 has k + 1 candidates, the first k invalid, the last one
                          (j = i + 2) valid: found = k = cnt - 1 -- the nearest-only row of k + 1 candidates, whose
                          erase moves (k + 1) * 7 floats down by one waypoint.  k = 0, 1, 63, 64, 65, 127, 128:
                          rows of 64, 65 and 129 candidates are first63, first64 and first128.  (first0's only
                          candidate is the straight-line test's edge, so it ends there.)
               far{k}     [A, x, g', x', g, b_k-1 .. b_0]: first valid candidate at k with a valid and an invalid
                          one after it in the same ballot; k = 1, 63, 64, 65
               none{c}    [A, b_c .. b_0]: row 0 has c candidates, none valid; c = 64, 65, 129
    bspline    Panda cage; BSPLINE only, and BSPLINE then SHORTCUT with max_steps 1 and 2; capacity 517.  Paths
               of 67, 70 and 130 waypoints at most 1.0 apart, some waypoints three times in a row (the middle
               one's midpoint change is exactly 0: a non-candidate, after which compact slots differ from
               even-index numbers), two of those among the first 64 even indices.
    cost       results of 64, 65, 66, 128 and 129 waypoints for the chunked cost sum: max_iterations = 0 passes
               64, 66 and 128 waypoints through, min_change = 1e9 BSPLINE-only subdivides 33 and 65 once.
    many       1023, 1024, 1025 and 2049 paths under the default settings, capacity 259: windows of 3 to 9
               waypoints of the seeded cage paths, every 11th cut to 0, 1 or 2 waypoints; first128 at index 1024
               and none129 at the last index (first128 where they coincide).
    fetch, ur5, baxter   the table_pick / bookshelf scenes of tests/golden: seeded raw and pulled-together paths of
               3, 9, 33 and 67 valid configurations whose straight line is blocked, default settings and BSPLINE only,
               capacity 259.
"""
import functools

import numpy as np

KS = (0, 1, 63, 64, 65, 127, 128)
FAR_KS = (1, 63, 64, 65)
NONE_ROWS = (64, 65, 129)
BS_LENGTHS = (67, 70, 130)
BS_CAPACITY = 2 * 259 - 1
BS_SEED = 11  # checked on the CPU: with it the restatement alone accepts and rejects candidates at slots >= 64
MANY = (1023, 1024, 1025, 2049)
MANY_CAPACITY = 259
ROBOT_LENGTHS = (3, 9, 33, 67)
ROBOT_CAPACITY = 259
ROBOT_FIXTURES = {"fetch": "fetch_table_pick.npz", "ur5": "ur5_table_pick.npz", "baxter": "baxter_bookshelf.npz"}
ROBOT_SEEDS = {"fetch": 21, "ur5": 22, "baxter": 23}

# the events each group exists for; check_group asserts every one of them was seen
GROUP_EVENTS = {
    "rows": ("hit_k>=64", "hit_k>=128", "hit_nearest_long", "row_none_over_64", "hit_inner", "row_none",
             "straight_ok", "straight_fail"),
    "bspline": ("bs_even_over_64", "bs_cand_slot>=64", "bs_accept_slot>=64", "bs_reject_slot>=64",
                "bs_gap_before_64", "accepted", "rejected", "hit_inner", "hit_k>=64", "capacity_stop"),
    "cost": ("cost_63", "cost_64", "cost_65", "cost_127", "cost_128"),
    "many": ("straight_ok", "straight_fail", "hit_inner", "row_none", "accepted", "rejected", "hit_k>=128",
             "row_none_over_64", "past_1024_idle", "past_1024_working"),
    "fetch": ("straight_fail", "row_none", "accepted", "rejected", "bs_even_over_64", "bs_cand_slot>=64",
              "capacity_stop"),
    "ur5": ("straight_fail", "row_none", "accepted", "rejected", "bs_even_over_64", "bs_cand_slot>=64",
            "capacity_stop"),
    "baxter": ("straight_fail", "row_none", "accepted", "rejected", "bs_even_over_64", "bs_cand_slot>=64",
               "capacity_stop"),
}

CASE_NAMES = ("rows", "bspline_only", "bspline_first-steps1", "bspline_first-steps2", "cost_pass", "cost_subdivide",
              *(f"many{n}" for n in MANY), *(f"{r}-{s}" for r in ROBOT_FIXTURES for s in ("default", "bspline")))
GROUPS = tuple(GROUP_EVENTS)

# test_simplify imports this module for the names above (its parametrised tests), so they come first
import oracle_py as op  # noqa: E402
from test_simplify import (BSPLINE, F, SEED, SHORTCUT, cage_paths, interpolate, l2, merge_trace,  # noqa: E402
                           new_trace, simplify_py)


class Case:
    def __init__(self, name, group, robot, settings, paths, capacity=None, base=(0, 0, 0)):
        self.name, self.group, self.robot, self.base = name, group, robot, tuple(base)
        self.settings, self.capacity = dict(settings), capacity
        self.paths = [(n, np.ascontiguousarray(p, F)) for n, p in paths]
        for _, p in self.paths:
            p.setflags(write=False)

    def py_keywords(self):
        """simplify_py's keywords of this case's settings"""
        kw = dict(self.settings)
        if "operations" in kw:
            kw["operations"] = tuple(kw["operations"])
        if "midpoint_interpolation" in kw:
            kw["midpoint"] = kw.pop("midpoint_interpolation")
        kw["max_path_len"] = self.capacity or 0
        return kw

    def cpu_keywords(self):
        """make_settings' keywords of the CPU run the batch is compared with"""
        return dict(self.settings, max_path_len=self.capacity or 0)


# ---- environments and validity -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_env(robot):
    op.build()
    if robot == "panda":
        return op.sphere_cage_env()
    from conftest import host_fixture
    from test_oracle_robots import scene_env
    return scene_env(op, host_fixture(ROBOT_FIXTURES[robot], op))


def product(vamp, case):
    """(the product's robot, its environment) of a case"""
    from test_gpu_parity import gpu_env_from_oracle
    robot = vamp.PandaBase(*case.base) if case.robot == "panda" else getattr(vamp, case.robot)
    return robot, gpu_env_from_oracle(vamp, oracle_env(case.robot))


def configs_valid(robot, q, base=(0, 0, 0)):
    return op.robot_fkcc_threads(robot, oracle_env(robot), q, base)


def edges_valid(robot, base=(0, 0, 0)):
    """validate(starts, goals) of simplify_py: the oracle's validate_motion of each edge"""
    oenv = oracle_env(robot)
    if robot == "panda":
        return lambda s, g: op.validate_motions(oenv, s, g, base)[0]
    return lambda s, g: op.robot_validate_motions(robot, oenv, s, g, base)[0]


def draws(robot, seed, n):
    """seeded uniform configurations that are valid in the robot's scene"""
    dim = op.ROBOTS[robot][1]
    q = op.robot_scale(robot, np.random.default_rng(seed).random((n, dim), dtype=F))
    return q[configs_valid(robot, q)]


def pulled(robot, q, n):
    """n waypoints from the draws q, each pulled to within distance 1.0 of its predecessor and kept when still
    valid (the "cap" paths of test_simplify.cage_paths); returns (path, draws used)"""
    w, at = [q[0]], 1
    while len(w) < n:
        d = l2((q[at] - w[-1]).astype(F))
        c = interpolate(w[-1], q[at], min(F(1.0), F(1.0) / d)) if d > 0 else q[at]
        at += 1
        if configs_valid(robot, c[None])[0]:
            w.append(c)
    return np.stack(w).astype(F), at


# ---- the groups --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def row_paths():
    """{name: path} of the constructed shortcut rows"""
    q = op.scale(np.random.default_rng(SEED).random((6000, 7), dtype=F))
    q = q[configs_valid("panda", q)]
    A, rest = q[0], q[1:]
    ok = edges_valid("panda")(np.repeat(A[None], len(rest), 0), rest)
    good, bad = rest[ok], rest[~ok]
    assert len(good) >= 8 and len(bad) >= 600, (len(good), len(bad))
    out, at = {}, 0

    def bads(n):  # fresh ones for every path
        nonlocal at
        at += n
        return bad[at - n:at]

    for i, k in enumerate(KS):
        out[f"first{k}"] = np.stack([A, bad[-1 - i], good[i % len(good)], *bads(k)])
    for i, k in enumerate(FAR_KS):
        out[f"far{k}"] = np.stack([A, bad[-20 - i], good[(i + 1) % len(good)], bad[-30 - i], good[i % len(good)],
                                   *bads(k)])
    for c in NONE_ROWS:
        out[f"none{c}"] = np.stack([A, *bads(c + 1)])
    assert at <= len(bad) - 40
    return out


def blocked(robot, a, b):
    """the motion a -> b is invalid: a path from a to b does not end at the straight-line test"""
    return not edges_valid(robot)(a[None], b[None])[0]


def blocked_pulled(robot, q, n):
    """pulled() paths from successive draws until one's front -> back motion is invalid"""
    at = 0
    while True:
        w, used = pulled(robot, q[at:], n)
        at += used
        if blocked(robot, w[0], w[-1]):
            return w, at


def pulled_to_blocked(robot, q, n):
    """a pulled() path of n - 1 waypoints and then, unpulled, the first draw that its front cannot reach by a
    valid motion (for scenes that leave most motions valid)"""
    w, at = pulled(robot, q, n - 1)
    while not blocked(robot, w[0], q[at]):
        at += 1
    return np.concatenate([w, q[at][None]]), at + 1


def blocked_raw(robot, q, n):
    """n draws, the last one replaced by later draws until the front -> back motion is invalid"""
    w, at = q[:n].copy(), n
    while not blocked(robot, w[0], w[-1]):
        w[-1] = q[at]
        at += 1
    return w, at


@functools.lru_cache(maxsize=None)
def bspline_paths():
    """[(name, path)]: pulled-together cage paths of BS_LENGTHS waypoints whose straight line is blocked, three of
    the waypoints tripled"""
    q = draws("panda", BS_SEED, 30000)
    out, at = [], 0
    for n in BS_LENGTHS:
        w, used = blocked_pulled("panda", q[at:], n - 6)
        at += used
        triple = {4, 21, len(w) - 3}  # waypoints 5 .. 7 and 24 .. 26 of the result lie among the first 64
        out.append((f"bs{n}", np.stack([x for i, x in enumerate(w) for _ in range(3 if i in triple else 1)])))
        assert len(out[-1][1]) == n
    return out


MANY_WINDOWS = 257


@functools.lru_cache(maxsize=None)
def many_paths(n):
    """n short paths: the 257 windows of test_many_short_paths over and over (257 is odd, so a window's copies
    sit in different lanes and waves of the scan), every 11th path cut to 0, 1 or 2 waypoints, and the two
    129-candidate rows at index 1024 and at the end (first128 where the two coincide)"""
    src = [p for _, p in cage_paths((0, 0, 0)) if len(p) >= 33]
    rows = row_paths()
    out = []
    for i in range(n):
        k = i % MANY_WINDOWS
        p = src[k % len(src)]
        m = 3 + k % 7
        at = (5 * k) % (len(p) - m)
        w = p[at:at + m]
        out.append((f"w{k}", w[:(i // 11) % 3].copy() if i % 11 == 0 else w.copy()))
    out[-1] = ("none129", rows["none129"])
    if n > 1024:
        out[1024] = ("first128", rows["first128"])
    return out


@functools.lru_cache(maxsize=None)
def robot_paths(robot):
    """[(name, path)]: raw draws and pulled-together paths (the last waypoint a free draw) of ROBOT_LENGTHS
    waypoints, valid in the robot's scene, front -> back blocked"""
    q = draws(robot, ROBOT_SEEDS[robot], 6000)
    out, at = [], 0
    for n in ROBOT_LENGTHS:
        for name, make in (("raw", blocked_raw), ("cap", pulled_to_blocked)):
            w, used = make(robot, q[at:], n)
            at += used
            out.append((f"{name}{n}", w))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """{name: Case}"""
    out = []
    out.append(Case("rows", "rows", "panda", dict(operations=[SHORTCUT]), list(row_paths().items())))
    bs = bspline_paths()
    out.append(Case("bspline_only", "bspline", "panda", dict(operations=[BSPLINE]), bs, BS_CAPACITY))
    for steps in (1, 2):
        out.append(Case(f"bspline_first-steps{steps}", "bspline", "panda",
                        dict(operations=[BSPLINE, SHORTCUT], max_steps=steps), bs, BS_CAPACITY))
    raw = draws("panda", SEED + 1, 4000)
    assert len(raw) >= 356
    out.append(Case("cost_pass", "cost", "panda", dict(max_iterations=0),
                    [("raw64", raw[:64]), ("raw66", raw[64:130]), ("raw128", raw[130:258])]))
    out.append(Case("cost_subdivide", "cost", "panda", dict(operations=[BSPLINE], min_change=1e9),
                    [("raw33", raw[258:291]), ("raw65", raw[291:356])]))
    for n in MANY:
        out.append(Case(f"many{n}", "many", "panda", {}, many_paths(n), MANY_CAPACITY))
    for robot in ROBOT_FIXTURES:
        out.append(Case(f"{robot}-default", robot, robot, {}, robot_paths(robot), ROBOT_CAPACITY))
        out.append(Case(f"{robot}-bspline", robot, robot, dict(operations=[BSPLINE]), robot_paths(robot),
                        ROBOT_CAPACITY))
    assert tuple(c.name for c in out) == CASE_NAMES
    return {c.name: c for c in out}




def group_cases(group):
    return [c for c in cases().values() if c.group == group]


# ---- the restatement, once per distinct run ------------------------------------------------------------------------
_RUNS = {}


def _run(case, path):
    kw = case.py_keywords()
    key = (case.robot, case.base, repr(sorted(kw.items())), path.shape, path.tobytes())
    if key not in _RUNS:
        t = new_trace()
        r, it, st = simplify_py(path, edges_valid(case.robot, case.base), t, **kw)
        r.setflags(write=False)
        _RUNS[key] = (r, it, st, t)
    return _RUNS[key]


@functools.lru_cache(maxsize=None)
def restated(name):
    """([per path (result, iterations, status, that run's trace)], the case's summed trace); computed once and
    shared, nobody writes to it"""
    case = cases()[name]
    runs = [_run(case, p) for _, p in case.paths]
    T = new_trace()
    for *_, t in runs:
        merge_trace(T, t)
    return runs, T


@functools.lru_cache(maxsize=None)
def group_seen(group):
    """event -> count over the group's cases, the derived events included"""
    seen = {k: 0 for k in GROUP_EVENTS[group]}
    for c in group_cases(group):
        runs, T = restated(c.name)
        for k in seen:
            if k in T and k != "cost_segments":
                seen[k] += int(T[k])
            elif k.startswith("cost_"):
                seen[k] += int(k[5:]) in T["cost_segments"]
        if "capacity_stop" in seen:
            seen["capacity_stop"] += sum(st == 1 for _, _, st, _ in runs)
        # a path past the scan's first block of 1024 that never works (no round at all) and one that works for
        # several rounds
        if "past_1024_idle" in seen:
            seen["past_1024_idle"] += sum(t["rounds"] == 0 for *_, t in runs[1025:])
            seen["past_1024_working"] += sum(t["rounds"] > 2 for *_, t in runs[1025:])
    return seen


def check_group(group):
    seen = group_seen(group)
    easy = [k for k in GROUP_EVENTS[group] if not seen[k]]
    assert not easy, f"inputs too easy: never seen {easy} ({seen})"
    return seen


def slowest(name):
    """index of the case's path with the most rounds in the restatement"""
    runs, _ = restated(name)
    return max(range(len(runs)), key=lambda i: runs[i][3]["rounds"])
