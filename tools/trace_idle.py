#!/usr/bin/env python3
"""Per-step dispatch count, busy time (union of kernel intervals) and idle share of a validate step, from a
rocprofv3 --kernel-trace run of tools/pmc_drive.py (run --workload validate): the dispatches between the two
spin_kernel markers, cut into steps at lead_kernel; the first step is the warm-up and is dropped.

    python3 tools/trace_idle.py DIR TAG [DIR TAG ...] > trace_idle.json    (one record per TAG; profiles/r07_trace_idle.json: parent, lean)"""
import csv
import glob
import json
import sys


def analyse(d, tag):
    path = [p for p in glob.glob(d + "/**/*kernel_trace.csv", recursive=True)][0]
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    spins = [i for i, r in enumerate(rows) if "spin_kernel" in r[2]]
    rows = rows[spins[0] + 1:spins[-1]]
    starts = [i for i, r in enumerate(rows) if "lead_kernel" in r[2]]
    steps = [rows[a:b] for a, b in zip(starts, starts[1:] + [len(rows)])][1:]
    out = {"tag": tag, "steps": []}
    names = {}
    for st in steps:
        span = max(e for _, e, _ in st) - st[0][0]
        busy, cur_s, cur_e = 0, None, None
        for s, e, _ in st:
            if cur_e is None or s > cur_e:
                if cur_e is not None:
                    busy += cur_e - cur_s
                cur_s, cur_e = s, e
            else:
                cur_e = max(cur_e, e)
        busy += cur_e - cur_s
        out["steps"].append({"dispatches": len(st), "span_us": span / 1e3, "busy_us": busy / 1e3,
                             "idle_us": (span - busy) / 1e3, "idle_share": (span - busy) / span,
                             "sum_durations_us": sum(e - s for s, e, _ in st) / 1e3})
        for s, e, n in st:
            k = n.split("(")[0][-90:]
            a = names.setdefault(k, [0, 0])
            a[0] += 1
            a[1] += e - s
    out["per_step_by_kernel"] = {k: {"calls_per_step": v[0] / len(steps), "us_per_step": v[1] / 1e3 / len(steps)}
                                 for k, v in sorted(names.items(), key=lambda kv: -kv[1][1])}
    return out


print(json.dumps({tag: analyse(d, tag) for d, tag in zip(sys.argv[1::2], sys.argv[2::2])}, indent=1))
