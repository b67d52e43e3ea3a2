"""RRT-Connect cases shared by tests/test_rrtc.py (the CPU planner against the restatement tests/rrtc_py.py)
and tests/test_gpu_rrtc_batch.py (the GPU batch against the CPU planner), so that every setting at which the
GPU is compared with the CPU planner is also one at which the CPU planner is pinned to the restatement.

Plain numpy and the oracle; nothing here needs a GPU.  All problems are the 16 table_pick problems of
tests/golden/panda_table_pick_problems.npz, each with its own scene.

A Case is a name, RRTCSettings keywords, a base, whether the scene gets the point cloud, and batches: a batch is
one scene (a problem number) and items (pair, goals, rng_first) -- the start of problem `pair`, the goals of the
problems `goals` in that order, the sampler's first draw.  A GPU call runs one batch; items of a batch have the
same number of goals.

    default, default-base200   range 1.0, no bounds: all 16 problems, offsets 1 and 1001
    ragged32, ragged257        all 16 start/goal pairs in problem 4's scene under an iteration bound
    wide                       range 0.1 and 200 samples: trees wider than a wave, packed connects cut by the cap
    iter40                     the iteration bound
    no_dynamic_domain, no_balance, goal_tree_first, small_domain, goal_first_no_balance
    clamp_domain               radius 4, min_radius 3, alpha 0.25: first shrink, shrink, clamp and growth
    range-{0.4,0.75,1.5,2.25,4.5}, range-2.25-base200   2 .. 18 rake blocks per segment
    base5                      the arm 5 cm off the scene's origin: searches with a non-zero base
    tree_ratio-{0.5,2.0}
    two_goals, three_goals     the other goals are other problems', in two orders
    pointcloud                 the scene plus a point cloud

EVENTS lists the trace events of rrtc_py.rrtc(trace=...); restated(name) runs the restatement once per case and
keeps results and trace for every test that needs them.  tie_layouts() constructs goals at bitwise equal
distance from the first sample (the nearest-neighbour tie rule)."""
import functools

import numpy as np

F = np.float32
BIG = 1000000
DEFAULT = dict(range=1.0, max_iterations=BIG, max_samples=BIG)
BOUNDED = dict(max_iterations=400, max_samples=512)  # the new cases' budget: a few hundred iterations at most
K3 = (4, 8, 14)
OFFSETS = (1, 1001)
WIDE = (2, 3, 5, 8, 11, 14)

# what rrtc_py.rrtc counts into `trace`; n stands for a block count
EVENTS = ("ext_reach", "ext_clip", "ext_n=n", "con_n=n", "dd_reject", "dd_first_shrink", "dd_shrink", "dd_clamp",
          "dd_grow", "con_multi_pass_packed", "con_cut_by_cap", "con_cut_inside_pass", "con_fail_first_in_pass",
          "con_fail_later_in_pass",
          "con_n_ext_0", "solved_flip", "solved_noflip", "len_b_0", "len_b_pos", "nn_over_64", "nn_winner_over_64",
          "tie")


def _oracle():
    import oracle_py
    oracle_py.build()
    return oracle_py


def problem(oracle, fx, k):
    o = oracle.Env()
    for key in ("spheres", "capsules", "zcapsules", "cuboids", "zcuboids"):
        setattr(o, key, [list(r) for r in fx[f"p{k}_env_{key}"]])
    return o, fx[f"p{k}_start"], fx[f"p{k}_goal"]


@functools.lru_cache(maxsize=None)
def _fixture():
    from conftest import host_fixture
    fx = host_fixture("panda_table_pick_problems.npz", _oracle())
    assert int(fx["n_problems"]) == 16
    return fx


def cloud_points():
    """300 points in a 24 cm cube in front of the arm"""
    rng = np.random.default_rng(7)
    return (np.array([0.35, 0.0, 0.9], F) + rng.uniform(-0.12, 0.12, (300, 3))).astype(F)


@functools.lru_cache(maxsize=None)
def scene(k, cloud=False):
    """problem k -> (oracle environment, start, goal); nobody writes to them"""
    o, s, g = problem(_oracle(), _fixture(), k)
    if cloud:
        from scenes import R_MAX, R_MIN, R_POINT
        o.add_pointcloud(cloud_points(), R_MIN, R_MAX, R_POINT)
    s, g = s.astype(F), g.astype(F)
    s.setflags(write=False)
    g.setflags(write=False)
    return o, s, g


def vamp_env(vamp, k, cloud=False):
    """the product's environment of scene(k, cloud)"""
    from test_gpu_parity import gpu_env_from_oracle
    env = gpu_env_from_oracle(vamp, scene(k)[0])
    if cloud:
        from scenes import R_MAX, R_MIN, R_POINT
        env.add_pointcloud(cloud_points(), R_MIN, R_MAX, R_POINT)
    return env


class Case:
    def __init__(self, name, settings, batches, base=(0, 0, 0), cloud=False, **gpu):
        self.name, self.settings, self.base, self.cloud = name, dict(settings), tuple(base), cloud
        self.batches = [(int(k), [(int(p), tuple(gs), int(f)) for p, gs, f in items]) for k, items in batches]
        for _, items in self.batches:
            assert len({len(gs) for _, gs, _ in items}) == 1
        # the GPU call's keywords: the arena holds every case's max_samples or more, so no case stops at it
        self.gpu = dict(node_cap=512, path_cap=128)
        self.gpu.update(gpu)

    def arrays(self, batch):
        """(scene, starts [n, 7], goals [n, n_goals, 7], rng_first uint64 [n]) of batch number `batch`"""
        k, items = self.batches[batch]
        starts = np.stack([scene(p)[1] for p, _, _ in items])
        goals = np.stack([np.stack([scene(q)[2] for q in gs]) for _, gs, _ in items])
        return k, starts, goals, np.array([f for _, _, f in items], np.uint64)


def own(problems, offsets=OFFSETS):
    """every problem in its own scene, once per sampler offset"""
    return [(k, [(k, (k,), f) for f in offsets]) for k in problems]


def _cases():
    out = []

    def add(name, settings, batches=None, **kw):
        out.append(Case(name, settings, own(K3) if batches is None else batches, **kw))

    add("default", DEFAULT, own(range(1, 17)), node_cap=256, path_cap=64)
    add("default-base200", DEFAULT, own(range(1, 17)), base=(200, 200, 0), node_cap=256, path_cap=64)
    add("ragged32", dict(range=1.0, max_iterations=300, max_samples=BIG),
        [(4, [(p, (p,), f) for f in OFFSETS for p in range(1, 17)])], path_cap=64)
    add("ragged257", dict(range=1.0, max_iterations=60, max_samples=BIG),
        [(4, [(1 + p % 16, (1 + p % 16,), 1 + 97 * p) for p in range(257)])], node_cap=128, path_cap=32, slice=16)
    add("wide", dict(range=0.1, max_samples=200, max_iterations=BIG), own(WIDE), node_cap=256, path_cap=256)
    add("iter40", dict(range=1.0, max_iterations=40, max_samples=BIG), own((5, 8, 11)), node_cap=256, path_cap=64)
    for name, kw in (("no_dynamic_domain", dict(dynamic_domain=False)), ("no_balance", dict(balance=False)),
                     ("goal_tree_first", dict(start_tree_first=False)),
                     ("small_domain", dict(radius=0.5, min_radius=0.2, alpha=0.25)),
                     ("goal_first_no_balance", dict(start_tree_first=False, balance=False)),
                     ("clamp_domain", dict(radius=4.0, min_radius=3.0, alpha=0.25)),
                     ("tree_ratio-0.5", dict(tree_ratio=0.5)), ("tree_ratio-2.0", dict(tree_ratio=2.0))):
        add(name, dict(range=1.0, **BOUNDED, **kw))
    for r in (0.4, 0.75, 1.5, 2.25, 4.5):
        add(f"range-{r}", dict(range=r, **BOUNDED))
    add("range-2.25-base200", dict(range=2.25, **BOUNDED), base=(200, 200, 0))
    # base (200, 200, 0) is clear of every scene, so those searches connect at once; 5 cm off, the scene is still
    # in reach: problem 14 solves, 4 and 8 search to the bound
    add("base5", dict(range=1.0, **BOUNDED), base=(5, 0, 0))
    bounded = dict(range=1.0, max_iterations=400, max_samples=BIG)
    add("two_goals", bounded, [(k, [(k, (k, o), 1), (k, (o, k), 1), (k, (k, o), 1001)])
                               for k, o in ((4, 7), (8, 14), (1, 2))], path_cap=64)
    add("three_goals", dict(range=1.0, **BOUNDED),
        [(k, [(k, gs, f) for gs in ((k, a, b), (b, a, k)) for f in OFFSETS]) for k, a, b in ((4, 7, 11), (8, 14, 2),
                                                                                            (14, 4, 5))])
    add("pointcloud", bounded, own((1, 4, 8, 14), (1,)), cloud=True, path_cap=64)
    return {c.name: c for c in out}


CASES = _cases()


@functools.lru_cache(maxsize=None)
def restated(name):
    """the restatement on every item of the case: ([per batch [per item (path, cost, iterations, sizes, index)]],
    the case's merged trace).  Computed once and shared; nobody writes to it."""
    import rrtc_py
    case = CASES[name]
    trace, out = {}, []
    for b in range(len(case.batches)):
        k, starts, goals, firsts = case.arrays(b)
        o = scene(k, case.cloud)[0]
        out.append([rrtc_py.rrtc("panda", o, starts[i], goals[i], case.settings, int(firsts[i]), case.base, trace=trace)
                    for i in range(len(starts))])
    return out, trace


# ---- exact limits ----------------------------------------------------------------------------------------------
# name -> (settings without bounds, problem, rng_first): searches that solve; the tests take the path length L and
# the node count N from the CPU planner and set path_cap to L and L - 1, the sample limit to N and N - 1.  In
# `packed` (range 0.1: one block per segment, 8 segments per pass) the limit N - 1 cuts the last connect between
# two segments of one pass (con_cut_inside_pass; tests/test_rrtc.py asserts it).
UNBOUNDED_01 = dict(range=0.1, max_iterations=BIG, max_samples=BIG)
LIMITS = {"default-1": (DEFAULT, 4, 1), "default-1001": (DEFAULT, 4, 1001), "packed": (UNBOUNDED_01, 2, 1)}


# ---- the nearest-neighbour tie ---------------------------------------------------------------------------------
# problem 4's scene and start; the goal tree is searched in iteration 1 (the start tree is tree_a at the top of
# the loop and balance = 0 always swaps), so the first sample's nearest node is chosen among the goals
TIE_PROBLEM = 4
TIE_SETTINGS = dict(range=1.0, max_iterations=400, max_samples=2048, start_tree_first=False, balance=False)


def _dist(temp, g):
    import rrtc_py
    return rrtc_py.l2_rows((temp - g).astype(F)[None])[0]


@functools.lru_cache(maxsize=None)
def tie_layouts():
    """{layout: goals [n, 7]}: g1 = problem 4's goal and g2, a point towards problem 7's goal moved float by
    float until its float32 l2_norm distance from the first sample (Halton draw 1, scaled) equals g1's bit for
    bit.  adjacent / adjacent-rev: [g1, g2] and [g2, g1], arena nodes 1 and 2, neighbouring lanes of the GPU's
    scan.  stride / stride-rev: 63 strictly farther fillers between them, arena nodes 1 and 65, one lane's
    consecutive visits."""
    op = _oracle()
    temp = op.robot_scale("panda", op.halton(7, [1]))[0]
    g1 = scene(TIE_PROBLEM)[2]
    d1 = _dist(temp, g1)
    away = (scene(7)[2] - temp).astype(np.float64)
    g2 = (temp + away * (float(d1) / np.linalg.norm(away))).astype(F)
    rng = np.random.default_rng(4)
    for _ in range(20000):
        d = _dist(temp, g2)
        if d == d1:
            break
        j = int(rng.integers(7))
        outward = np.sign(g2[j] - temp[j]) * (1 if d < d1 else -1)
        g2[j] = np.nextafter(g2[j], F(np.inf) * F(outward if outward else 1))
    assert _dist(temp, g2).view(np.uint32) == d1.view(np.uint32) and g2.tobytes() != g1.tobytes()
    fill = (temp + 1.5 * (g1 - temp) + np.random.default_rng(5).uniform(-0.05, 0.05, (63, 7))).astype(F)
    assert all(_dist(temp, f) > d1 for f in fill)
    out = {"adjacent": np.stack([g1, g2]), "adjacent-rev": np.stack([g2, g1]),
           "stride": np.stack([g1, *fill, g2]), "stride-rev": np.stack([g2, *fill, g1])}
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def tie_restated(layout, tie_last=False):
    """((path, cost, iterations, sizes, index), trace) of the restatement on a tie layout, sampler at 1"""
    import rrtc_py
    o, s, _ = scene(TIE_PROBLEM)
    trace = {}
    return rrtc_py.rrtc("panda", o, s, tie_layouts()[layout], TIE_SETTINGS, 1, trace=trace, tie_last=tie_last), trace
