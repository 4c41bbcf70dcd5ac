#!/usr/bin/env python3
"""Experiment type 6 at small k: Engine.exp6_run by its bitmap form against the same call by its set form.

    python tools/bench_exp6_small_k.py [--runs 3] [--steps 1] [--k-min 7 --k-max 13] [--reads 10000] [--out FILE]

Shape: 10 groups x 5 genomes x 5 Mbp, texts resident on the device; per pivot (one per group) 10 000 reads, once of 150
bases and once of 10 kb, cut from a sixth genome of the group's ancestor (its bytes outside ACGT left out), resident as
well.  The ruler is the path of the commit before the bitmap form, which is not the code under test.  It can be reached
in two ways: that commit's library built aside, or this tree under KHOICE_NO_BMP=1, whose set form the bitmap form left
as it was.  This tool takes the second (`ruler` in the output says so).  Per k and read length both sides first answer
once (the warm-up) and their outputs must be identical; then they are timed in turn (sets, bitmaps, sets, bitmaps, ...),
`--runs` times each, `--steps` calls per run, with a host clock around calls that end in a device synchronise.  k = 13
is the control: there exp6_run takes the set form on both sides.  A last call under the profiler gives the kernel times
of bmp_build, bmp_present, bmp_group_masks, read_lookup and read_fold.

Output (default profiles/exp6_small_k.json): per k and read length the ms per call of every run, median and spread
((max - min) / median) of both sides, speedup, outputs_identical, and `passes`: the bitmap form is faster by more than
twice the larger spread."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIELDS = ("within_hist", "distinct_per_seq")
KERNELS = ("bmp_build", "bmp_present", "bmp_group_masks", "read_lookup", "read_fold")
READ_LENGTHS = (150, 10_000)


def column(ms):
    med = statistics.median(ms)
    return {"ms_per_call": [round(v, 3) for v in ms], "median_ms": round(med, 3), "spread": round((max(ms) - min(ms)) / med, 4)}


def cut_reads(text, nreads, length, seed):
    """(text of nreads reads of `length` bases, one line each; offsets) cut at random from the ACGT bytes of `text`."""
    src = np.frombuffer(text, dtype=np.uint8)
    src = src[np.isin(src, np.frombuffer(b"ACGT", dtype=np.uint8))]
    starts = np.random.default_rng(seed).integers(0, src.size - length, size=nreads)
    lines = np.empty((nreads, length + 1), dtype=np.uint8)
    lines[:, :length] = src[starts[:, None] + np.arange(length)[None, :]]
    lines[:, length] = ord("\n")
    return lines.reshape(-1), np.arange(nreads + 1, dtype=np.uint64) * np.uint64(length + 1)


def identical(a, b):
    return all(np.array_equal(a[f], b[f]) for f in FIELDS) and all(
        np.array_equal(x, y) for f in ("tie_masks", "unmatched") for x, y in zip(a[f], b[f]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--k-min", type=int, default=7)
    ap.add_argument("--k-max", type=int, default=13)
    ap.add_argument("--species", type=int, default=10)
    ap.add_argument("--genomes", type=int, default=5)
    ap.add_argument("--length", type=int, default=5_000_000)
    ap.add_argument("--reads", type=int, default=10_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exp6_small_k.json"))
    args = ap.parse_args()
    import torch
    from khoice_amd import build as kbuild
    from khoice_amd import engine as E
    from khoice_amd import synth
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured without one")
    kbuild.build_library()
    os.environ.pop("KHOICE_NO_BMP", None)
    hosts, owner, keep, pivot_reads = [], [], [], {n: [] for n in READ_LENGTHS}
    for s in range(1, args.species + 1):
        anc = synth.ancestor(s, args.length)
        for g in range(args.genomes + 1):
            text = synth.clean_text(synth.genome_records(s, g, args.length, anc))
            if g < args.genomes:
                hosts.append(text)
                owner.append(s - 1)
                continue
            for n in READ_LENGTHS:
                lines, off = cut_reads(text, args.reads, n, 1000 * s + n)
                keep.append(torch.from_numpy(lines).cuda())
                pivot_reads[n].append(((keep[-1].data_ptr(), keep[-1].numel()), off))
    dev = [torch.from_numpy(np.frombuffer(t, dtype=np.uint8).copy()).cuda() for t in hosts]
    torch.cuda.synchronize()
    seqs = [(d.data_ptr(), d.numel()) for d in dev]
    cs, hist_len = 5000, 5001
    out = {"shape": f"{args.species} groups x {args.genomes} genomes x {args.length} bp + {args.species} pivots x {args.reads} reads",
           "ruler": "this tree under KHOICE_NO_BMP=1 (the set form, which the bitmap form left as it was)",
           "runs": args.runs, "steps": args.steps, "k": {}}
    with E.Engine(0) as eng:
        def call(k, n, no_bmp):
            if no_bmp:
                os.environ["KHOICE_NO_BMP"] = "1"
            try:
                return eng.exp6_run(seqs, owner, pivot_reads[n], k, cs=cs, hist_len=hist_len)
            finally:
                os.environ.pop("KHOICE_NO_BMP", None)

        sides = {"sets": lambda k, n: call(k, n, True), "bitmaps": lambda k, n: call(k, n, False)}
        for k in range(args.k_min, args.k_max + 1):
            out["k"][str(k)] = {}
            for n in READ_LENGTHS:
                first = {name: fn(k, n) for name, fn in sides.items()}       # the warm-up, and the two answers
                assert identical(first["sets"], first["bitmaps"]), (k, n)
                ms = {name: [] for name in sides}
                for _ in range(args.runs):
                    for name, fn in sides.items():
                        eng.sync()
                        t0 = time.perf_counter()
                        for _ in range(args.steps):
                            fn(k, n)
                        eng.sync()
                        ms[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
                eng.profile(True)
                st0 = eng.stats()
                sides["bitmaps"](k, n)
                st1 = eng.stats()
                eng.profile(False)
                kern = {c: round(st1["kernels"][c]["ms"] - st0["kernels"][c]["ms"], 4) for c in KERNELS
                        if st1["kernels"][c]["launches"] > st0["kernels"][c]["launches"]}
                row = {name: column(v) for name, v in ms.items()}
                row["outputs_identical"] = True
                row["form"] = "bitmaps" if "bmp_build" in kern else "sets"
                row["kernel_ms"] = kern
                row["speedup"] = round(row["sets"]["median_ms"] / row["bitmaps"]["median_ms"], 3)
                margin = 2 * max(row["sets"]["spread"], row["bitmaps"]["spread"])
                row["passes"] = row["bitmaps"]["median_ms"] < row["sets"]["median_ms"] * (1 - margin)
                out["k"][str(k)][str(n)] = row
                print(f"k={k} reads of {n}: {json.dumps(row)}", flush=True)
                with open(args.out, "w") as fh:                              # after every row: a run that stops early keeps what it measured
                    json.dump(out, fh, indent=1)
                    fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
