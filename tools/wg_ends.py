#!/usr/bin/env python
"""When do the workgroups of the persistent union end their walk?

Reads what a -DKH_STAMPS -DKH_STAMPS_WG build (tools/build_diag.sh wg) appended to $KHOICE_WG_DUMP, one line per
workgroup and call: call, workgroup, hardware id, XCC, shader clock at the beginning and the end of the walk,
constant-rate clock at the beginning and the end.  Prints, for the last call of the file (or --call N):
  - the distribution of (workgroup end - kernel start) / (last end - kernel start), on the constant-rate clock that all
    XCCs share: minimum, quartiles, the share of workgroups that end before 0.9;
  - the workgroups that shared a CU (same XCC, shader engine, shader array and CU in the hardware id), in dispatch
    order: how far apart they end, and whether the one dispatched first ends first.

    python tools/wg_ends.py wg_k31.txt [--call N] [--json out.json]
"""
import argparse
import json
from collections import defaultdict

import numpy as np


def analyse(rows):
    rows = rows[np.argsort(rows[:, 1])]
    b, hwid, xcc = rows[:, 1], rows[:, 2], rows[:, 3] & 0xF
    out = {"workgroups": int(len(b))}
    for name, c0, c1 in (("constant_clock", 6, 7), ("shader_clock", 4, 5)):
        start, end = rows[:, c0].astype(np.float64), rows[:, c1].astype(np.float64)
        t0 = start.min()
        span = end.max() - t0
        frac = (end - t0) / span
        q = np.quantile(frac, [0.0, 0.25, 0.5, 0.75, 1.0])
        out[name] = {"span_ticks": float(span), "start_spread": float((start.max() - t0) / span),
                     "min": float(q[0]), "q1": float(q[1]), "median": float(q[2]), "q3": float(q[3]),
                     "share_before_0.9": float((frac < 0.9).mean()), "share_before_0.95": float((frac < 0.95).mean()),
                     "share_before_0.99": float((frac < 0.99).mean()), "mean": float(frac.mean())}
        if name != "constant_clock":
            continue
        cus = defaultdict(list)
        for i in range(len(b)):
            cus[(int(xcc[i]), int(hwid[i] >> 8) & 0xFF)].append(i)     # (XCC, SE / SH / CU bits); i ascends with blockIdx
        gaps, first_first, sizes = [], 0, defaultdict(int)
        for members in cus.values():
            sizes[len(members)] += 1
            if len(members) < 2:
                continue
            f = frac[members]
            gaps.append(float(f.max() - f.min()))
            first_first += int(np.argmin(f) == 0)
        rng = np.random.default_rng(1)
        perm = rng.permutation(len(b))
        rnd = np.abs(frac[perm[0::2][: len(b) // 2]] - frac[perm[1::2][: len(b) // 2]])
        half = len(b) // 2
        out["pairs"] = {"cus": len(cus), "workgroups_per_cu": {str(k): v for k, v in sorted(sizes.items())},
                        "mean_gap_inside_a_cu": float(np.mean(gaps)) if gaps else None,
                        "mean_gap_of_random_pairs": float(rnd.mean()),
                        "first_dispatched_ends_first": first_first / max(1, len(gaps)),
                        "corr_b_vs_b_plus_half_grid": float(np.corrcoef(frac[:half], frac[half:2 * half])[0, 1]),
                        "mean_end_first_half_of_grid": float(frac[:half].mean()),
                        "mean_end_second_half_of_grid": float(frac[half:].mean())}
    return out


def occupancy(rows, resident):
    """A launch of more workgroups than the chip holds (k_skm_scatter, $KHOICE_WG_DUMP_SCATTER): the filled share of the
    `resident` workgroup places over the launch (sum of the workgroups' lives / (resident x span)), the mean
    concurrency in every tenth of the span, and when the workgroups end."""
    start, end = rows[:, 6].astype(np.float64), rows[:, 7].astype(np.float64)
    t0, span = start.min(), end.max() - start.min()
    edges = t0 + span * np.linspace(0.0, 1.0, 11)
    conc = [float(np.clip(np.minimum(end, hi) - np.maximum(start, lo), 0, None).sum() / (hi - lo)) for lo, hi in zip(edges, edges[1:])]
    frac = (end - t0) / span
    q = np.quantile(frac, [0.0, 0.25, 0.5, 0.75, 1.0])
    life = end - start
    return {"workgroups": int(len(rows)), "resident": int(resident), "span_ticks": float(span),
            "filled_share": float(life.sum() / (resident * span)), "mean_concurrency": float(life.sum() / span),
            "concurrency_by_tenth": [round(c, 1) for c in conc],
            "life_ticks": {"mean": float(life.mean()), "min": float(life.min()), "max": float(life.max())},
            "end": {"min": float(q[0]), "q1": float(q[1]), "median": float(q[2]), "q3": float(q[3]),
                    "share_before_0.9": float((frac < 0.9).mean())}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dump")
    ap.add_argument("--call", type=int, default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--resident", type=int, default=0, help="a scatter dump: workgroups the chip holds at a time")
    a = ap.parse_args()
    rows = np.loadtxt(a.dump, dtype=np.uint64, ndmin=2)
    calls = np.unique(rows[:, 0])
    call = calls[-1] if a.call is None else a.call
    if a.resident:
        res = {"dump": a.dump, "calls_in_file": int(len(calls)), "call": int(call), **occupancy(rows[rows[:, 0] == call], a.resident)}
        res["last_calls_filled_share"] = [round(occupancy(rows[rows[:, 0] == c], a.resident)["filled_share"], 4) for c in calls[-5:]]
        print(json.dumps(res, indent=1))
        if a.json:
            with open(a.json, "w") as fh:
                json.dump(res, fh, indent=1)
        return
    res = {"dump": a.dump, "calls_in_file": int(len(calls)), "call": int(call), **analyse(rows[rows[:, 0] == call])}
    # how stable the picture is: the share before 0.9 and the idle wave-slot share (1 - mean end) of every call
    per_call = [analyse(rows[rows[:, 0] == c])["constant_clock"] for c in calls[-5:]]
    res["last_calls_mean_end"] = [round(p["mean"], 4) for p in per_call]
    res["last_calls_min_end"] = [round(p["min"], 4) for p in per_call]
    print(json.dumps(res, indent=1))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
