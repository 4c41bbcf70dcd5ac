#!/usr/bin/env python3
"""Where a bench step's time goes outside its kernels, from ONE rocprofv3 trace without counters:

    rocprofv3 --kernel-trace --memory-copy-trace --hip-runtime-trace --output-format csv -d DIR -- \\
        python3 bench.py --steps 5 --warmup 2 --no-cpu-baseline
    python3 tools/step_timeline.py DIR [--steps 5] [--json profiles/rNN_step_timeline.json]

A step is one k_skm_scatter dispatch with the device activity around it (fill / upload in front, regroup and union
behind, read-back at the end); the last --steps of them are the timed ones.  Per step, in microseconds:
  idle_before_first   GPU idle from the previous step's last device activity to this step's first
  front               first device activity -> the scatter's start, and its parts (each op's duration, each gap)
  scatter_to_regroup, regroup_to_union   gaps between the kernels
  union_to_sync_return   the union's end -> hipStreamSynchronize returns (read-back and wake-up)
  host_before_first_launch   the call's first HIP API (hipSetDevice at the top of kh_exp1_run) -> its first enqueue
  host_submit         first enqueue -> the synchronise is entered
  between_calls       the synchronise's return -> the next call's first HIP API: the native tail (replica sums, fold),
                      the Python binding both ways and bench.py's loop
  api                 host time inside named HIP calls of the step (sum of their durations, count)"""
import argparse
import csv
import glob
import json
import os
import statistics


def rows(d, suffix):
    f = glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True)
    if not f:
        raise SystemExit(f"no *{suffix} under {d}")
    return list(csv.DictReader(open(f[0])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--json")
    a = ap.parse_args()
    dev = []   # (start, end, what)
    for r in rows(a.dir, "kernel_trace.csv"):
        n = r["Kernel_Name"]
        what = ("scatter" if "_scatter" in n else "regroup" if "_regroup" in n else "union" if "_union" in n else
                "fill" if "fillBuffer" in n else "ws_init" if "ws_init" in n else "ws_down" if "ws_down" in n else "kernel:" + n[:24])
        dev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), what))
    for r in rows(a.dir, "memory_copy_trace.csv"):
        dev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "h2d" if "HOST_TO_DEVICE" in r["Direction"] else "d2h"))
    dev.sort()
    api = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Function"]) for r in rows(a.dir, "hip_api_trace.csv"))
    scat = [i for i, e in enumerate(dev) if e[2] == "scatter"]
    if len(scat) < a.steps + 1:
        raise SystemExit(f"{len(scat)} scatter dispatches: fewer than --steps + 1")
    ENQ = ("hipMemsetAsync", "hipMemcpyAsync", "hipLaunchKernel", "hipModuleLaunchKernel", "hipExtLaunchKernel")
    us = lambda ns: round(ns / 1e3, 2)
    steps = []
    for si in scat[-a.steps:]:
        # the step's device activity: back from the scatter to the op after the previous union's read-back, forward to
        # the last op before the next step's first
        lo = si
        while lo > 0 and dev[lo - 1][2] in ("fill", "h2d", "ws_init"):
            lo -= 1
        hi = si
        while hi + 1 < len(dev) and dev[hi + 1][2] not in ("fill", "h2d", "ws_init", "scatter"):
            hi += 1
        ops = dev[lo:hi + 1]
        byname = {o[2]: o for o in ops}
        st = {"idle_before_first": us(ops[0][0] - dev[lo - 1][1]) if lo else None,
              "front": us(dev[si][0] - ops[0][0]), "front_parts": []}
        for j in range(lo, si):
            st["front_parts"].append([dev[j][2], us(dev[j][1] - dev[j][0]), "gap", us(dev[j + 1][0] - dev[j][1])])
        st["scatter_to_regroup"] = us(byname["regroup"][0] - byname["scatter"][1])
        st["regroup_to_union"] = us(byname["union"][0] - byname["regroup"][1])
        st["behind_union"] = [[o[2], "gap", us(o[0] - p[1]), us(o[1] - o[0])] for p, o in zip(ops, ops[1:]) if p[0] >= byname["union"][0]]
        # the host side: the synchronise that covers the union's end, the call's APIs back to the previous synchronise
        uend = byname["union"][1]
        sync = next(x for x in api if x[2] == "hipStreamSynchronize" and x[1] >= uend)
        prev = max((x for x in api if x[2] == "hipStreamSynchronize" and x[1] < sync[0]), key=lambda x: x[1])
        call = [x for x in api if prev[1] <= x[0] <= sync[0]]
        first_enq = next(x for x in call if x[2] in ENQ)
        st["union_to_sync_return"] = us(sync[1] - uend)
        st["last_device_op_to_sync_return"] = us(sync[1] - ops[-1][1])
        st["host_before_first_launch"] = us(first_enq[0] - call[0][0])
        st["host_submit"] = us(sync[0] - first_enq[0])
        st["between_calls"] = us(call[0][0] - prev[1])
        st["first_launch_to_device_start"] = us(ops[0][0] - first_enq[0])
        per = {}
        for x in call:
            d = per.setdefault(x[2], [0, 0])
            d[0] += x[1] - x[0]
            d[1] += 1
        st["api"] = {k: [us(v[0]), v[1]] for k, v in sorted(per.items())}
        st["kernels"] = {n: us(byname[n][1] - byname[n][0]) for n in ("scatter", "regroup", "union")}
        steps.append(st)
    keys = ("idle_before_first", "front", "scatter_to_regroup", "regroup_to_union", "union_to_sync_return",
            "last_device_op_to_sync_return", "host_before_first_launch", "host_submit", "between_calls", "first_launch_to_device_start")
    med = {k: statistics.median(s[k] for s in steps) for k in keys}
    for i, s in enumerate(steps):
        print(f"step {i}: " + "  ".join(f"{k} {s[k]}" for k in keys))
        print("   front:", s["front_parts"], " behind the union:", s["behind_union"])
    print("median: " + "  ".join(f"{k} {med[k]}" for k in keys))
    print("api of the last step (us, calls):", steps[-1]["api"])
    if a.json:
        json.dump({"unit": "us", "source": "rocprofv3 --kernel-trace --memory-copy-trace --hip-runtime-trace, bench.py --steps 5 --warmup 2 --no-cpu-baseline",
                   "median": med, "steps": steps}, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
