#!/usr/bin/env python3
"""Read-level votes (experiment type 6): Engine.read_votes on two read sets, with kh_membership as a ruler.

    python tools/bench_read_votes.py [--runs 5] [--species 10] [--genomes 4] [--length 5000000] [--out FILE]

Shape: 10 datasets x 4 genomes x 5 Mbp at k = 31; the sets are the `set_counts 1` unions of the datasets.  The reads
are cut from a fifth genome of dataset 1 (cuts that hold an N or a contig break are drawn again): 2*10^5 reads of 150
bases and 2*10^3 reads of 10^4 bases, resident on the device.  Per read set one warm-up call, then `--runs` timed calls
(host clock around a call that ends in a device synchronise), then `--runs` calls under the profiler for the split
between k_read_masks and k_read_fold (kh_stats).  The ruler: kh_confusion_row of the same pivot genome's distinct
k-mers against the same sets, its k_membership time from kh_stats, in lookups (k-mer x set) per second.

Output (default profiles/read_votes.json): medians and spreads ((max - min) / median) of the ms per call, of both
kernels, windows per second, and the searches per second of k_read_masks next to k_membership's."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K = 31


def column(ms):
    med = statistics.median(ms)
    return {"ms": [round(v, 3) for v in ms], "median_ms": round(med, 3), "spread": round((max(ms) - min(ms)) / med, 4)}


def cut_reads(text: bytes, n_reads: int, length: int, seed: int):
    """(buffer uint8, offsets uint64) of n_reads cuts of `length` bases in the layout of Engine.read_votes."""
    rng = np.random.default_rng(seed)
    t = np.frombuffer(text, dtype=np.uint8)
    ok = np.zeros(256, dtype=bool)
    ok[list(b"ACGT")] = True
    rows = np.zeros((0, length), dtype=np.uint8)
    while rows.shape[0] < n_reads:
        starts = rng.integers(0, t.size - length, size=n_reads - rows.shape[0])
        cand = t[starts[:, None] + np.arange(length)[None, :]]
        rows = np.concatenate([rows, cand[ok[cand].all(axis=1)]])
    buf = np.concatenate([rows, np.full((n_reads, 1), 10, dtype=np.uint8)], axis=1).reshape(-1)
    return buf, np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(length + 1)


def kernel_ms(st0, st1, name):
    return st1["kernels"][name]["ms"] - st0["kernels"][name]["ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--species", type=int, default=10)
    ap.add_argument("--genomes", type=int, default=4)
    ap.add_argument("--length", type=int, default=5_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "read_votes.json"))
    args = ap.parse_args()
    import torch
    from khoice_amd import build as kbuild
    from khoice_amd import engine as E
    from khoice_amd import synth
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured without one")
    kbuild.build_library()
    hosts, owner, pivot = [], [], None
    for s in range(1, args.species + 1):
        anc = synth.ancestor(s, args.length)
        for g in range(args.genomes + (s == 1)):
            text = synth.clean_text(synth.genome_records(s, g, args.length, anc))
            if g == args.genomes:
                pivot = text
            else:
                hosts.append(text)
                owner.append(s - 1)
    read_sets = {"150b_x_200000": cut_reads(pivot, 200_000, 150, 1), "10kb_x_2000": cut_reads(pivot, 2_000, 10_000, 2)}
    dev = [torch.from_numpy(np.frombuffer(t, dtype=np.uint8).copy()).cuda() for t in hosts + [pivot]]
    dev_reads = {n: torch.from_numpy(b).cuda() for n, (b, _) in read_sets.items()}
    torch.cuda.synchronize()
    texts = [(d.data_ptr(), d.numel()) for d in dev]
    out = {"shape": f"{args.species} datasets x {args.genomes} genomes x {args.length} bp, k = {K}", "runs": args.runs,
           "reads": {}}
    with E.Engine(0) as eng:
        plain = eng.build_batch(texts[:-1], K, ci=1, with_counts=False)
        sets = []
        for g in range(args.species):
            union = eng.union_sum([s for s, o in zip(plain, owner) if o == g], 5000)
            sets.append(union.set_counts(1))
            union.free()
        for s in plain:
            s.free()
        out["set_kmers"] = [len(s) for s in sets]
        for name, (buf, off) in read_sets.items():
            reads = (dev_reads[name].data_ptr(), buf.size)
            windows = int(((off[1:] - off[:-1]).astype(np.int64) - K).clip(0).sum())
            eng.read_votes(reads, off, K, sets)                                   # warm-up
            ms = []
            for _ in range(args.runs):
                eng.sync()
                t0 = time.perf_counter()
                eng.read_votes(reads, off, K, sets)
                ms.append((time.perf_counter() - t0) * 1e3)
            eng.profile(True)
            masks, fold = [], []
            for _ in range(args.runs):
                st0 = eng.stats()
                eng.read_votes(reads, off, K, sets)
                st1 = eng.stats()
                masks.append(kernel_ms(st0, st1, "read_masks"))
                fold.append(kernel_ms(st0, st1, "read_fold"))
            eng.profile(False)
            row = {"reads": off.size - 1, "windows": windows, "call": column(ms), "k_read_masks": column(masks),
                   "k_read_fold": column(fold)}
            row["windows_per_s"] = round(windows / (row["call"]["median_ms"] * 1e-3))
            row["masks_lookups_per_s"] = round(windows * len(sets) / (row["k_read_masks"]["median_ms"] * 1e-3))
            out["reads"][name] = row
            print(name, json.dumps(row), flush=True)
        pv = eng.build(texts[-1], K, ci=1, with_counts=True)                      # the ruler
        eng.confusion_row(pv, sets)
        eng.profile(True)
        mem = []
        for _ in range(args.runs):
            st0 = eng.stats()
            eng.confusion_row(pv, sets)
            mem.append(kernel_ms(st0, eng.stats(), "setop"))
        eng.profile(False)
        out["k_membership"] = dict(column(mem), pivot_kmers=len(pv))
        out["k_membership"]["lookups_per_s"] = round(len(pv) * len(sets) / (out["k_membership"]["median_ms"] * 1e-3))
        print("k_membership", json.dumps(out["k_membership"]), flush=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
