#!/usr/bin/env python3
"""Experiment type 3 above the bitmaps: Engine.exp3_run with KHOICE_EXP3_SKM=1 (k_skm_cross over super-k-mer records)
against the same call with the switch unset (the set form inside the library).  Both sides are this tree.

    python tools/bench_exp3_skm.py [--runs 3] [--steps 10] [--k 17,21,31,41,63] [--out FILE]

Shape: that of tools/bench_exp3_small_k.py — 10 groups x 4 genomes x 5 Mbp and 20 pivots, two read sets of a fifth
genome of every group's ancestor (10 000 reads of 150 bases, 10 000 reads of 200 to 8 000 bases): 60 operands, one pass;
texts resident on the device.  Per k both sides first answer once (the warm-up) and their outputs must be identical;
then they are timed in turn (sets, skm, sets, skm, ...), `--runs` times each, `--steps` calls per run, with a host
clock around calls that end in a device synchronise.  One further call with the switch set under the profiler gives
the kernel times of skm_scatter, skm_regroup and skm_cross, and the statistics say which form answered.

Output (default profiles/exp3_skm.json): per k the ms per call of every run, median and spread ((max - min) / median)
of both sides, speedup, outputs_identical, the form, its kernel times and slot statistics, and `passes`: the
super-k-mer form is faster by more than twice the larger spread."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIELDS = ("inter_hist", "distinct_per_seq", "distinct_per_pivot")
KERNELS = ("copy_in", "skm_scatter", "skm_regroup", "skm_cross")
COUNTERS = ("retries", "big_slots", "cross_multi_slots", "skm_records", "setops")
SWITCH = "KHOICE_EXP3_SKM"


def column(ms):
    med = statistics.median(ms)
    return {"ms_per_call": [round(v, 3) for v in ms], "median_ms": round(med, 3), "spread": round((max(ms) - min(ms)) / med, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--k", default="17,21,31,41,63")
    ap.add_argument("--species", type=int, default=10)
    ap.add_argument("--genomes", type=int, default=4)
    ap.add_argument("--length", type=int, default=5_000_000)
    ap.add_argument("--reads", type=int, default=10_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exp3_skm.json"))
    args = ap.parse_args()
    import torch
    from khoice_amd import build as kbuild
    from khoice_amd import engine as E
    from khoice_amd import synth
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured without one")
    kbuild.build_library()
    hosts, owner, short, long_ = [], [], [], []
    for s in range(1, args.species + 1):
        anc = synth.ancestor(s, args.length)
        for g in range(args.genomes):
            hosts.append(synth.clean_text(synth.genome_records(s, g, args.length, anc)))
            owner.append(s - 1)
        codes = synth.genome_codes(s, args.genomes, args.length, anc)
        short.append(b"\n".join(synth.simulated_reads(codes, args.reads, 150, 0.002, 2 * s)))
        long_.append(b"\n".join(synth.simulated_reads(codes, args.reads, 8_000, 0.05, 2 * s + 1, min_len=200)))
    phosts = short + long_
    dev = [torch.from_numpy(np.frombuffer(t, dtype=np.uint8).copy()).cuda() for t in hosts + phosts]
    torch.cuda.synchronize()
    texts = [(d.data_ptr(), d.numel()) for d in dev]
    seqs, pivots = texts[:len(hosts)], texts[len(hosts):]
    cs, hist_len = 5000, 5001
    out = {"shape": f"{args.species} groups x {args.genomes} genomes x {args.length} bp + {len(phosts)} pivots "
                    f"({args.species} x {args.reads} reads of 150, {args.species} x {args.reads} reads of 200..8000)",
           "pivot_bases": sum(len(t) for t in phosts), "genome_bases": sum(len(t) for t in hosts),
           "runs": args.runs, "steps": args.steps, "k": {}}
    with E.Engine(0) as eng:
        def side(on):
            def call(k):
                if on:
                    os.environ[SWITCH] = "1"
                else:
                    os.environ.pop(SWITCH, None)
                return eng.exp3_run(seqs, owner, pivots, k, cs=cs, hist_len=hist_len)
            return call
        sides = {"sets": side(False), "skm": side(True)}
        for k in (int(x) for x in args.k.split(",")):
            first = {name: fn(k) for name, fn in sides.items()}          # the warm-up, and the two answers
            for f in FIELDS:
                assert np.array_equal(first["sets"][f], first["skm"][f]), (k, f)
            ms = {name: [] for name in sides}
            for _ in range(args.runs):
                for name, fn in sides.items():
                    eng.sync()
                    t0 = time.perf_counter()
                    for _ in range(args.steps):
                        fn(k)
                    eng.sync()
                    ms[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
            eng.profile(True)
            st0 = eng.stats()
            sides["skm"](k)
            st1 = eng.stats()
            eng.profile(False)
            kern = {n: round(st1["kernels"][n]["ms"] - st0["kernels"][n]["ms"], 4) for n in KERNELS
                    if st1["kernels"][n]["launches"] > st0["kernels"][n]["launches"]}
            row = {name: column(v) for name, v in ms.items()}
            row["outputs_identical"] = True
            row["form"] = "skm_cross" if "skm_cross" in kern and st1["retries"] == st0["retries"] else "sets"
            row["kernel_ms"] = kern
            row["cross_launches"] = st1["kernels"]["skm_cross"]["launches"] - st0["kernels"]["skm_cross"]["launches"]
            row["stats"] = {n: st1[n] - st0[n] for n in COUNTERS}
            row["speedup"] = round(row["sets"]["median_ms"] / row["skm"]["median_ms"], 3)
            margin = 2 * max(row["sets"]["spread"], row["skm"]["spread"])
            row["passes"] = row["skm"]["median_ms"] < row["sets"]["median_ms"] * (1 - margin)
            out["k"][str(k)] = row
            print(f"k={k} {json.dumps(row)}", flush=True)
            with open(args.out, "w") as fh:                              # after every k: a run that stops early keeps what it measured
                json.dump(out, fh, indent=1)
                fh.write("\n")
    os.environ.pop(SWITCH, None)
    return 0


if __name__ == "__main__":
    sys.exit(main())
