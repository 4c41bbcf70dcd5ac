#!/usr/bin/env python3
"""Experiment type 6 above k = 12: Engine.exp6_run by its index form against the same call by its set form.

    python tools/bench_exp6_index.py [--runs 3] [--ks 13,21,31,41,63] [--reads 10000] [--read-lengths 150,10000]
                                       [--sweep 100,1000,10000] [--species 10 --genomes 5 --length 5000000] [--out FILE]

Shape: 10 groups x 5 genomes x 5 Mbp, texts resident on the device; per pivot (one per group) 10 000 reads, once of 150
bases and once of 10 kb, cut from a sixth genome of the group's ancestor (its bytes outside ACGT left out), resident as
well: the shape of tools/bench_exp6_small_k.py.  The sides are KHOICE_EXP6_INDEX=1 (the merged mask index of
kh_index.hip) and KHOICE_EXP6_INDEX=0 (the set form of the same tree, which the index form leaves as it was).  Per point
both sides first answer once (the warm-up) and their outputs must be identical; then they are timed in turn (sets,
index, sets, index, ...), `--runs` times each, one call per run, with a host clock around calls that end in a device
synchronise.  A last call under the profiler gives the kernel times of the index form's classes, and a MaskIndex built
over the same group sets gives the index's n and bytes.  For the break-even the sweep repeats k = 31 with 150-base
reads at `--sweep` reads per pivot.

Output (default profiles/exp6_index.json): per point the ms per call of every run, median and spread ((max - min) /
median) of both sides, speedup, `ratio` = windows * ngroups / sum |sets|, and `wins`: "index" or "sets" when that
side's median beats the other's by more than twice the larger spread, else "none".  `R` is the smallest measured
ratio from which the index wins every measured point at that ratio and above (0: it wins everywhere; null: it does not
win at the largest ratio)."""
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
KERNELS = ("extract_hist", "bucket_plan", "extract_scatter", "bucket_sort_rle", "range_bounds", "setop", "index_dir",
           "index_tag", "read_index", "read_masks", "read_fold")


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


def winner(row):
    margin = 2 * max(row["sets"]["spread"], row["index"]["spread"])
    s, i = row["sets"]["median_ms"], row["index"]["median_ms"]
    return "index" if i < s * (1 - margin) else "sets" if s < i * (1 - margin) else "none"


def break_even(points):
    """R from [(ratio, wins)]: the smallest measured ratio from which the index wins every point at that ratio and above."""
    pts = sorted(points)
    if all(w == "index" for _, w in pts):
        return 0
    r = None
    for ratio, w in reversed(pts):
        if w != "index":
            break
        r = ratio
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--ks", default="13,21,31,41,63")
    ap.add_argument("--species", type=int, default=10)
    ap.add_argument("--genomes", type=int, default=5)
    ap.add_argument("--length", type=int, default=5_000_000)
    ap.add_argument("--reads", type=int, default=10_000)
    ap.add_argument("--read-lengths", default="150,10000")
    ap.add_argument("--sweep", default="100,1000,10000")
    ap.add_argument("--sweep-k", type=int, default=31)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exp6_index.json"))
    args = ap.parse_args()
    import torch
    from khoice_amd import build as kbuild
    from khoice_amd import engine as E
    from khoice_amd import synth
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured without one")
    kbuild.build_library()
    ks = [int(k) for k in args.ks.split(",") if k]
    sweep = [int(n) for n in args.sweep.split(",") if n]
    read_lengths = [int(n) for n in args.read_lengths.split(",") if n]
    hosts, owner, keep, pivot_reads = [], [], [], {}
    shapes = [(n, args.reads) for n in read_lengths] + [(150, n) for n in sweep if n != args.reads]
    for s in range(1, args.species + 1):
        anc = synth.ancestor(s, args.length)
        for g in range(args.genomes + 1):
            text = synth.clean_text(synth.genome_records(s, g, args.length, anc))
            if g < args.genomes:
                hosts.append(text)
                owner.append(s - 1)
                continue
            for length, nreads in shapes:
                lines, off = cut_reads(text, nreads, length, 1000 * s + length)
                keep.append(torch.from_numpy(lines).cuda())
                pivot_reads.setdefault((length, nreads), []).append(((keep[-1].data_ptr(), keep[-1].numel()), off))
    dev = [torch.from_numpy(np.frombuffer(t, dtype=np.uint8).copy()).cuda() for t in hosts]
    torch.cuda.synchronize()
    seqs = [(d.data_ptr(), d.numel()) for d in dev]
    cs, hist_len = 5000, 5001
    out = {"shape": f"{args.species} groups x {args.genomes} genomes x {args.length} bp + {args.species} pivots x reads",
           "ruler": "this tree under KHOICE_EXP6_INDEX=0 (the set form, which the index form left as it was)",
           "runs": args.runs, "points": [], "R": None}
    with E.Engine(0) as eng:
        def call(k, shape, index):
            os.environ["KHOICE_EXP6_INDEX"] = "1" if index else "0"
            try:
                return eng.exp6_run(seqs, owner, pivot_reads[shape], k, cs=cs, hist_len=hist_len)
            finally:
                os.environ.pop("KHOICE_EXP6_INDEX", None)

        sides = {"sets": lambda k, shape: call(k, shape, False), "index": lambda k, shape: call(k, shape, True)}
        sizes = {}

        def index_size(k):
            """{n, bytes, sum_sets} of the index over the groups' sets at k (the sets of group_unions, built here)."""
            if k not in sizes:
                plain = eng.build_batch(seqs, k, with_counts=False)
                groups = [eng.union_sum([p for p, o in zip(plain, owner) if o == g], cs) for g in range(args.species)]
                with eng.mask_index(groups) as ix:
                    i = ix.info()
                w = 1 if k <= 32 else 2
                sizes[k] = {"n": i["n"], "sum_sets": int(sum(len(g) for g in groups)),
                            "bytes": i["n"] * 8 * (w + i["mask_words"]) + 8 * (i["buckets"] + 1)}
                for s in plain + groups:
                    s.free()
            return sizes[k]

        points = [(k, (length, args.reads)) for k in ks for length in read_lengths]
        points += [(args.sweep_k, (150, n)) for n in sweep if (args.sweep_k, (150, n)) not in
                   [(k, s) for k, s in points]]
        for k, shape in points:
            length, nreads = shape
            first = {name: fn(k, shape) for name, fn in sides.items()}       # the warm-up, and the two answers
            assert identical(first["sets"], first["index"]), (k, shape)
            ms = {name: [] for name in sides}
            for _ in range(args.runs):
                for name, fn in sides.items():
                    eng.sync()
                    t0 = time.perf_counter()
                    fn(k, shape)
                    eng.sync()
                    ms[name].append((time.perf_counter() - t0) * 1e3)
            eng.profile(True)
            st0 = eng.stats()
            sides["index"](k, shape)
            st1 = eng.stats()
            eng.profile(False)
            kern = {c: round(st1["kernels"][c]["ms"] - st0["kernels"][c]["ms"], 4) for c in KERNELS
                    if st1["kernels"][c]["launches"] > st0["kernels"][c]["launches"]}
            size = index_size(k)
            windows = args.species * nreads * max(0, length - k + 1)
            row = {"k": k, "read_length": length, "reads_per_pivot": nreads}
            row.update({name: column(v) for name, v in ms.items()})
            row["outputs_identical"] = True
            row["form"] = "index" if "read_index" in kern else "sets"
            row["kernel_ms"] = kern
            row["index_n"], row["index_bytes"], row["sum_sets"] = size["n"], size["bytes"], size["sum_sets"]
            row["ratio"] = round(windows * args.species / size["sum_sets"], 4)
            row["speedup"] = round(row["sets"]["median_ms"] / row["index"]["median_ms"], 3)
            row["wins"] = winner(row)
            out["points"].append(row)
            out["R"] = break_even([(p["ratio"], p["wins"]) for p in out["points"]])
            print(json.dumps(row), flush=True)
            with open(args.out, "w") as fh:                                  # after every row: a run that stops early keeps what it measured
                json.dump(out, fh, indent=1)
                fh.write("\n")
    print(json.dumps({"R": out["R"]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
