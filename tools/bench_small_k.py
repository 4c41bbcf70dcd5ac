#!/usr/bin/env python3
"""Small-k sweep of the headline shape: bench.py at k = 7 .. 16, this tree against a built checkout of another commit.

    python tools/bench_small_k.py --parent DIR [--runs 3] [--k-min 7 --k-max 16] [--steps 20 --warmup 3] [--out FILE]

For every k the two trees are run in turn (parent, new, parent, new, ...), `--runs` times each, so that drift of the
machine shows up in both columns and the run-to-run spread is known.  Every run is a fresh child process under its own
time limit (`timeout -k 10`): python bench.py --k K --no-cpu-baseline --dump-outputs DIR, started in the tree it measures.
The sweep stops at the first child that does not exit with 0.  The arrays the two trees dump at a k must be identical.
Without --parent only this tree is measured.

Output (default profiles/small_k_sweep.json): per k the ms_per_step of every run, their median and spread
((max - min) / median) for both trees, kernel_ms_per_step of the last run of each, and outputs_identical;
_source_sha is bench.source_hash() of this tree."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NAMES = ("within_hist", "across_hist", "distinct_per_seq")


def bench_once(tree, k, steps, warmup, dump, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, "bench.py", "--gpus", "1", "--k", str(k), "--steps", str(steps),
           "--warmup", str(warmup), "--no-cpu-baseline", "--dump-outputs", dump]
    p = subprocess.run(cmd, cwd=tree, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        return p.returncode, None
    return 0, json.loads(p.stdout.strip().splitlines()[-1])


def column(runs):
    ms = [r["ms_per_step"] for r in runs]
    med = statistics.median(ms)
    return {"ms_per_step": ms, "median_ms": round(med, 4), "spread": round((max(ms) - min(ms)) / med, 4),
            "kernel_ms_per_step": {n: v for n, v in runs[-1]["kernel_ms_per_step"].items() if v},
            "replans": runs[-1]["replans"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the commit to compare against")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--k-min", type=int, default=7)
    ap.add_argument("--k-max", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=180, help="seconds a child may run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "small_k_sweep.json"))
    args = ap.parse_args()
    import bench
    trees = ([("parent", os.path.abspath(args.parent))] if args.parent else []) + [("new", ROOT)]
    out = {"_source_sha": bench.source_hash(), "shape": "10 species x 5 genomes x 5 Mbp", "steps": args.steps,
           "warmup": args.warmup, "runs": args.runs, "k": {}}
    rc = 0
    with tempfile.TemporaryDirectory() as tmp:
        for k in range(args.k_min, args.k_max + 1):
            got = {name: [] for name, _ in trees}
            for r in range(args.runs):
                for name, tree in trees:
                    rc, res = bench_once(tree, k, args.steps, args.warmup, os.path.join(tmp, f"{name}_{k}"), args.limit)
                    if rc != 0:
                        print(f"k={k} {name} run {r}: exit {rc}; stopping", flush=True)
                        break
                    got[name].append(res)
                    print(f"k={k} {name} run {r}: {res['ms_per_step']} ms", flush=True)
                if rc != 0:
                    break
            if rc != 0:
                break
            row = {name: column(runs) for name, runs in got.items()}
            if args.parent:
                row["outputs_identical"] = all(
                    np.array_equal(np.load(os.path.join(tmp, f"parent_{k}", n + ".npy")), np.load(os.path.join(tmp, f"new_{k}", n + ".npy")))
                    for n in NAMES)
                row["speedup"] = round(row["parent"]["median_ms"] / row["new"]["median_ms"], 3)
            out["k"][str(k)] = row
            with open(args.out, "w") as fh:          # after every k: a sweep that stops early keeps what it measured
                json.dump(out, fh, indent=1)
                fh.write("\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
