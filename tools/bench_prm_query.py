"""Timing of the batched roadmap search (vgpu_roadmap_query.hip) against the CPU function on the same graph.

One Panda roadmap on the MotionBenchMaker table_pick scene (problem 2 of tests/golden, as tools/bench_simplify.py)
built by Robot.roadmap from `draws` Halton draws, cut at `max_samples` vertices.  For S in {1, 8, 64}: S sources
drawn from the start's component, searched as ONE vgpu_roadmap_sssp call (g, hops and parent; device arrays, the
call's own host reads included), against vgpu_cpu_roadmap_sssp looped over the same sources on one core and
spread over 16 threads (one search per task).  Prints one JSON line per S: ms per search of the three, the
GPU call's rounds, and relaxed slots / reachable directed slots (1.0 = every slot relaxed once; above it, slots
relaxed again after their vertex's g fell a second time).  The S = 8 batch is also compared with the CPU result bit for bit.
Usage: python tools/bench_prm_query.py [draws] [max_samples] [reps]
"""
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mr-vamp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import vamp_amd as vamp  # noqa: E402
from bench_simplify import scene  # noqa: E402
from vamp_amd import roadmap  # noqa: E402


def main():
    draws = int(sys.argv[1]) if len(sys.argv) > 1 else 1500000
    max_samples = int(sys.argv[2]) if len(sys.argv) > 2 else 300000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    import torch
    robot = vamp.panda_0_0
    env, start, goal = scene()
    ctx = vamp.context(0)
    settings = vamp.PRMSettings(vamp.PRMNeighborParams(robot.dimension(), robot.space_measure()))
    settings.max_iterations, settings.max_samples = draws, max_samples
    t0 = time.perf_counter()
    rm = robot.roadmap(start, goal, env, settings, robot.halton(), ctx)
    build_s = time.perf_counter() - t0
    n, n_adj = len(rm), len(rm.adj)
    t0 = time.perf_counter()
    w = rm.weights
    weights_ms = 1e3 * (time.perf_counter() - t0)  # upload + vgpu_roadmap_edge_weights + read-back
    _, graph = rm._device(ctx)
    off = rm.offsets.astype(np.uint64)
    deg = np.diff(rm.offsets)
    home = np.nonzero(rm.component == rm.component[0])[0]
    rng = np.random.default_rng(0)
    at = rm.connect_index(0, 1, ctx)
    print(json.dumps({"workload": "prm query table_pick", "vertices": n, "directed_slots": n_adj,
                      "mean_degree": n_adj / max(n, 1), "max_degree": int(deg.max()), "start_component": len(home),
                      "build_s": build_s, "weights_ms": weights_ms, "connect_index": at}))
    ok = True
    for S in (1, 8, 64):
        sources = rng.choice(home, S).astype(np.uint32)
        roadmap.sssp_device(torch, graph, sources, None, ctx)  # warm-up: sizes the workspace
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            g, hops, parent = roadmap.sssp_device(torch, graph, sources, None, ctx)
            times.append(time.perf_counter() - t0)
        stats = roadmap.sssp_stats(ctx)
        gpu_s = float(np.median(times))
        reach = int((torch.isfinite(g).to(torch.int64) * torch.from_numpy(deg).to(g.device)[None, :]).sum().item())
        t0 = time.perf_counter()
        want = [roadmap.cpu_sssp(off, rm.adj, w, [s]) for s in sources]
        cpu1_s = time.perf_counter() - t0
        with ThreadPoolExecutor(16) as pool:
            t0 = time.perf_counter()
            list(pool.map(lambda s: roadmap.cpu_sssp(off, rm.adj, w, [s]), sources))
            cpu16_s = time.perf_counter() - t0
        parity = None
        if S == 8:
            gg, hh, pp = g.cpu().numpy(), hops.cpu().numpy().view(np.uint32), parent.cpu().numpy().view(np.uint32)
            parity = all(gg[i].tobytes() == want[i][0].tobytes() and np.array_equal(hh[i], want[i][1][0]) and
                         np.array_equal(pp[i], want[i][2][0]) for i in range(S))
            ok = ok and parity
        print(json.dumps({"S": S, "gpu_ms_per_search": 1e3 * gpu_s / S, "cpu_1core_ms_per_search": 1e3 * cpu1_s / S,
                          "cpu_16threads_ms_per_search": 1e3 * cpu16_s / S, "gpu_call_ms": 1e3 * gpu_s,
                          "rounds": stats["rounds"], "host_reads": stats["host_reads"],
                          "relaxed_slots": stats["relaxed_slots"], "reachable_slots": reach,
                          "relaxed_per_reachable": stats["relaxed_slots"] / max(reach, 1), "parity": parity}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
