"""Timing of batched path simplification (vgpu_simplify.hip) against a loop of the CPU function.

P RRT-Connect paths on one MotionBenchMaker table_pick scene (problem 2 of tests/golden: its straight line is
blocked, so the planner searches), one per Halton offset (robot.halton().skip(k)), simplified with the default
settings: once as one simplify_batch call (host arrays in and out, so the copies are included) and once as P
calls of Robot.simplify on the CPU rake (one core).  Prints paths/s of both, the batch's rounds, validate calls and edges validated, and the over-evaluation
ratio: edges validated by the batch / edges the sequential walk validates (the batch validates a whole shortcut
row where the walk stops at its first valid edge, and both edges of a B-spline candidate where the walk skips
the second after an invalid first).
Usage: python tools/bench_simplify.py [n_paths] [reps]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mr-vamp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vamp_amd as vamp  # noqa: E402


def scene():
    """table_pick problem 2: its obstacles, start and goal (tests/golden/panda_table_pick_problems.npz)"""
    fx = np.load(os.path.join(ROOT, "tests", "golden", "panda_table_pick_problems.npz"), allow_pickle=False)
    env = vamp.Environment()
    for x, y, z, r, _ in fx["p2_env_spheres"]:
        env.add_sphere(vamp.Sphere([x, y, z], r))
    for key in ("cuboids", "zcuboids"):
        for row in fx[f"p2_env_{key}"]:
            env.add_cuboid(vamp.Cuboid.from_axes(row[0:3], row[3:6], row[6:9], row[9:12], row[12:15]))
    for key in ("capsules", "zcapsules"):
        for row in fx[f"p2_env_{key}"]:
            p1 = np.array(row[0:3], np.float32)
            env.add_capsule(vamp.Cylinder(p1, (p1 + np.array(row[3:6], np.float32)).astype(np.float32), row[6]))
    return env, fx["p2_start"], fx["p2_goal"]


def main():
    n_paths = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    robot = vamp.panda_0_0
    env, start, goal = scene()
    settings = vamp.RRTCSettings(range=1.0, max_iterations=1000000, max_samples=1000000)
    paths = []
    for k in range(n_paths):
        rng = robot.halton()
        rng.skip(k)
        res = robot.rrtc(start, goal, env, settings, rng)
        if res.solved:
            paths.append(res.path)
    simp = vamp.SimplifySettings()
    ctx = vamp.context(0)

    robot.simplify_batch(paths, env, simp, ctx)  # warm-up: uploads the environment, sizes the workspaces
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        got, status = robot.simplify_batch(paths, env, simp, ctx)
        times.append(time.perf_counter() - t0)
    stats = robot.simplify_stats(ctx)
    batch_s = float(np.median(times))

    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        want = [robot.simplify(p, env, simp) for p in paths]
        times.append(time.perf_counter() - t0)
    seq_edges = sum(w.validated_edges for w in want)
    loop_s = float(np.median(times))
    parity = all(g.path.tobytes() == w.path.tobytes() and g.iterations == w.iterations for g, w in zip(got, want))
    line = {"workload": "simplify table_pick", "paths": len(paths), "reps": reps,
            "mean_len_in": float(np.mean([len(p) for p in paths])),
            "mean_len_out": float(np.mean([len(g.path) for g in got])), "parity": bool(parity),
            "batch_ms": 1e3 * batch_s, "batch_paths_per_s": len(paths) / batch_s,
            "loop_ms": 1e3 * loop_s, "loop_paths_per_s": len(paths) / loop_s, "loop_cores": 1,
            "rounds": stats["rounds"], "validate_calls": stats["validate_calls"], "batch_edges": stats["edges"],
            "sequential_edges": int(seq_edges), "over_evaluation": stats["edges"] / max(seq_edges, 1),
            "capacity_stops": int(np.count_nonzero(status))}
    print(json.dumps(line))
    return 0 if parity else 1


if __name__ == "__main__":
    sys.exit(main())
