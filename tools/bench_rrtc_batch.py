"""Timing of batched RRT-Connect (vgpu_rrtc.hip: one wave per problem) against a loop of the CPU planner.

P problems from the 16 MotionBenchMaker table_pick problems of tests/golden, each with P / 16 Halton offsets
(rng_first = 1, 1001, 2001, ...), range 1.0.  Every problem of the fixture has its own scene, so the batch runs
in two modes: 16 rrtc_batch calls of P / 16 problems each, one per scene ("batch_*"), and ONE rrtc_batch_scenes
call of all P problems, each naming its scene ("scenes_*") -- host arrays in and out in both, so the copies are
included.  The CPU side is P calls of Robot.rrtc on the CPU rake, on one core and on 16 threads (the calls release
the GIL).  Prints problems/s of all of them, each mode's launches, the iterations and the straggler ratio: the
largest iteration count of one problem over the mean -- a launch lasts as long as its slowest wave.  Both modes are
compared with the CPU loop bit for bit ("parity", "scenes_parity").
Usage: python tools/bench_rrtc_batch.py [n_problems] [reps] [node_cap]
"""
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mr-vamp_amd"))

import vamp_amd as vamp  # noqa: E402


def scene(fx, k):
    """table_pick problem k: its obstacles, start and goal (tests/golden/panda_table_pick_problems.npz)"""
    env = vamp.Environment()
    for x, y, z, r, _ in fx[f"p{k}_env_spheres"]:
        env.add_sphere(vamp.Sphere([x, y, z], r))
    for key in ("cuboids", "zcuboids"):
        for row in fx[f"p{k}_env_{key}"]:
            env.add_cuboid(vamp.Cuboid.from_axes(row[0:3], row[3:6], row[6:9], row[9:12], row[12:15]))
    for key in ("capsules", "zcapsules"):
        for row in fx[f"p{k}_env_{key}"]:
            p1 = np.array(row[0:3], np.float32)
            env.add_capsule(vamp.Cylinder(p1, (p1 + np.array(row[3:6], np.float32)).astype(np.float32), row[6]))
    return env, fx[f"p{k}_start"].astype(np.float32), fx[f"p{k}_goal"].astype(np.float32)


def main():
    P = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    node_cap = int(sys.argv[3]) if len(sys.argv) > 3 else 64
    robot = vamp.panda_0_0
    fx = np.load(os.path.join(ROOT, "tests", "golden", "panda_table_pick_problems.npz"), allow_pickle=False)
    n = int(fx["n_problems"])
    per = max(P // n, 1)
    scenes = [scene(fx, k) for k in range(1, n + 1)]
    firsts = (1 + 1000 * np.arange(per)).astype(np.uint64)
    settings = vamp.RRTCSettings(range=1.0, max_iterations=1000000, max_samples=1000000)
    ctx = vamp.context(0)

    def batch():
        out, launches, iterations, most = [], 0, 0, 0
        for env, s, g in scenes:
            got, status, idx = robot.rrtc_batch(np.tile(s, (per, 1)), np.tile(g, (per, 1)), env, settings, firsts,
                                                node_cap, 32, ctx)
            stats = robot.rrtc_stats(ctx)
            launches += stats["launches"]
            iterations += stats["iterations"]
            most = max(most, stats["max_iterations"])
            out += list(zip(got, status, idx))
        return out, launches, iterations, most

    # the same problems in the same order as one multi-scene call
    envs = [env for env, _, _ in scenes]
    all_s = np.concatenate([np.tile(s, (per, 1)) for _, s, _ in scenes])
    all_g = np.concatenate([np.tile(g, (per, 1)) for _, _, g in scenes])
    all_e = np.repeat(np.arange(n, dtype=np.uint32), per)
    all_f = np.tile(firsts, n)

    def one_call():
        got, status, idx = robot.rrtc_batch_scenes(all_s, all_g, envs, all_e, settings, all_f, node_cap, 32, ctx)
        return list(zip(got, status, idx)), robot.rrtc_stats(ctx)

    batch()  # warm-up: uploads the environments, sizes the arena
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        got, launches, iterations, most = batch()
        times.append(time.perf_counter() - t0)
    batch_s = float(np.median(times))

    # the C call alone (copies in, launches, copies out) on the same arrays, without the Python result objects
    import ctypes as C
    from vamp_amd import _lib
    paths = np.zeros((per, 32, 7), np.float32)
    ln, st = np.zeros(per, np.uint32), np.zeros(per, np.uint8)
    res = (_lib.VgpuPlanResult * per)()
    cs = settings.c()
    tiled = [(env, np.tile(s, (per, 1)), np.tile(g, (per, 1))) for env, s, g in scenes]
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for env, s, g in tiled:
            idx = firsts.copy()
            _lib.check(_lib.load().vgpu_rrtc_batch_host(
                ctx.h, C.byref(robot.c_robot), env.handle(ctx), s.ctypes.data_as(_lib.F32P), g.ctypes.data_as(_lib.F32P),
                1, per, C.byref(cs), idx.ctypes.data_as(_lib.U64P), node_cap, paths.ctypes.data_as(_lib.F32P), 32,
                ln.ctypes.data_as(_lib.U32P), res, st.ctypes.data_as(_lib.U8P)), ctx.h)
        times.append(time.perf_counter() - t0)
    call_s = float(np.median(times))

    one_call()  # warm-up: the arena for all P problems, the view table
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        sgot, sstats = one_call()
        times.append(time.perf_counter() - t0)
    scenes_s = float(np.median(times))
    total = n * per
    paths = np.zeros((total, 32, 7), np.float32)
    ln, st = np.zeros(total, np.uint32), np.zeros(total, np.uint8)
    res = (_lib.VgpuPlanResult * total)()
    handles = (C.c_void_p * n)(*[env.handle(ctx) for env in envs])
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        idx = all_f.copy()
        _lib.check(_lib.load().vgpu_rrtc_batch_scenes_host(
            ctx.h, C.byref(robot.c_robot), handles, n, all_e.ctypes.data_as(_lib.U32P), all_s.ctypes.data_as(_lib.F32P),
            all_g.ctypes.data_as(_lib.F32P), 1, total, C.byref(cs), idx.ctypes.data_as(_lib.U64P), node_cap,
            paths.ctypes.data_as(_lib.F32P), 32, ln.ctypes.data_as(_lib.U32P), res, st.ctypes.data_as(_lib.U8P)), ctx.h)
        times.append(time.perf_counter() - t0)
    scenes_call_s = float(np.median(times))

    jobs = [(j, k) for j in range(n) for k in range(per)]  # the batch's order

    def one(job):
        env, s, g = scenes[job[0]]
        rng = robot.halton()
        rng.skip(int(firsts[job[1]]) - 1)
        return robot.rrtc(s, g, env, settings, rng), rng.index

    for j in range(n):
        one((j, 0))  # the host environments
    t0 = time.perf_counter()
    want = [one(job) for job in jobs]
    loop_s = time.perf_counter() - t0
    with ThreadPoolExecutor(16) as pool:
        t0 = time.perf_counter()
        list(pool.map(one, jobs, chunksize=max(len(jobs) // 256, 1)))
        loop16_s = time.perf_counter() - t0
    planner_ns = sum(w.nanoseconds for w, _ in want)  # the searches alone, without the Python call around them
    def same(results):
        return len(results) == len(want) and all(
            st != 0 or (a.path.tobytes() == w.path.tobytes() and a.iterations == w.iterations and int(i) == wi)
            for (a, st, i), (w, wi) in zip(results, want))

    parity, scenes_parity = same(got), same(sgot)
    scenes_parity = scenes_parity and [st for _, st, _ in sgot] == [st for _, st, _ in got]
    its = np.array([w.iterations for w, _ in want], np.float64)
    total = len(jobs)
    line = {"workload": "rrtc_batch table_pick", "problems": total, "calls": n, "reps": reps, "node_cap": node_cap,
            "parity": bool(parity), "stopped_at_capacity": int(sum(st != 0 for _, st, _ in got)),
            "solved": int(sum(a.solved for a, _, _ in got)),
            "batch_ms": 1e3 * batch_s, "batch_problems_per_s": total / batch_s,
            "batch_c_call_ms": 1e3 * call_s, "batch_c_call_problems_per_s": total / call_s,
            "loop_ms": 1e3 * loop_s, "loop_problems_per_s": total / loop_s, "loop_planner_ms": planner_ns / 1e6,
            "loop16_ms": 1e3 * loop16_s, "loop16_problems_per_s": total / loop16_s,
            "scenes_parity": bool(scenes_parity), "scenes_ms": 1e3 * scenes_s,
            "scenes_problems_per_s": total / scenes_s, "scenes_c_call_ms": 1e3 * scenes_call_s,
            "scenes_c_call_problems_per_s": total / scenes_call_s, "scenes_launches": sstats["launches"],
            "launches": launches, "iterations": iterations, "max_iterations": most,
            "mean_iterations": float(its.mean()), "straggler_ratio": float(its.max() / max(its.mean(), 1e-9))}
    print(json.dumps(line))
    return 0 if parity and scenes_parity else 1


if __name__ == "__main__":
    sys.exit(main())
