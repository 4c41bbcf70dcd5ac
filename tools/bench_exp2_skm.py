#!/usr/bin/env python3
"""Experiment type 2 above the bitmaps: Engine.exp2_run with KHOICE_EXP2_SKM=1 (the own-group read-out of k_skm_cross
over super-k-mer records) against the set form inside the library — of this tree, or with --parent-lib of another build
of the library (the parent commit's), which is the comparison that counts.

    python tools/bench_exp2_skm.py [--runs 3] [--steps 5] [--k 17,21,31,41,63] [--parent-lib FILE] [--exp3-ab 31,41] [--out FILE]

Shape: that of tools/bench_exp2_small_k.py — 10 groups x 5 genomes x 5 Mbp and one pivot of 5 Mbp per group (a sixth
genome of the group's ancestor): 60 operands and 160 bins, one pass; texts resident on the device.

This process never opens the GPU.  It writes the texts to a temporary file once and starts one WORKER process per run
and side, the sides in turn (sets, skm, sets, skm, ...), each under `timeout`; a worker that fails ends the measurement
(nothing more is started) and what was measured so far is kept.  A worker loads the library of its side
(KHOICE_HIP_LIB), uploads the texts and, per k, answers once (the warm-up, hashed), times `--steps` calls with a host
clock around calls that end in a device synchronise, and answers once more under the profiler: kernel times, and from
the statistics which form answered.

--exp3-ab K,K: type 3 must not pay for the shared body.  tools/bench_exp3_skm.py --k K,K is run `--runs` times per
library, parent and this tree in turn, each under `timeout`; its skm side is compared.

Output (default profiles/exp2_skm.json): per k the ms per call of every run, median and spread ((max - min) / median) of
both sides, speedup, outputs_identical (the hashes of all runs of both sides agree), the form that answered
(`skm_cross`, or `sets` where the form declined or retried), its kernel times and slot statistics; under `exp3_ab` per k
the same columns for the two libraries and `within_parent_spread`: this tree's median <= the parent's median + the
parent's max - min."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIELDS = ("within_hist", "across_hist", "within_only", "across_only", "distinct_per_seq", "distinct_per_pivot")
KERNELS = ("copy_in", "skm_scatter", "skm_regroup", "skm_cross")
COUNTERS = ("retries", "big_slots", "cross_multi_slots", "skm_records", "setops")
SWITCH = "KHOICE_EXP2_SKM"


def column(ms):
    med = statistics.median(ms)
    return {"ms_per_call": [round(v, 3) for v in ms], "median_ms": round(med, 3), "spread": round((max(ms) - min(ms)) / med, 4)}


def make_texts(args, path):
    from khoice_amd import synth
    texts, owner, pivots = [], [], []
    for s in range(1, args.species + 1):
        anc = synth.ancestor(s, args.length)
        for g in range(args.genomes + 1):
            text = synth.clean_text(synth.genome_records(s, g, args.length, anc))
            if g == args.genomes:
                pivots.append(text)
            else:
                texts.append(text)
                owner.append(s - 1)
    lens = np.array([len(t) for t in texts + pivots], dtype=np.int64)
    np.savez(path, blob=np.frombuffer(b"".join(texts + pivots), dtype=np.uint8), lens=lens, owner=np.array(owner), npivots=len(pivots))


def worker(args):
    """One run of one side: every k in one process.  Prints one JSON line per k."""
    import torch
    from khoice_amd import engine as E
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured without one")
    z = np.load(args.texts)
    owner, npiv = [int(g) for g in z["owner"]], int(z["npivots"])
    ends = np.cumsum(z["lens"])
    dev = [torch.from_numpy(z["blob"][e - n:e].copy()).cuda() for e, n in zip(ends, z["lens"])]
    torch.cuda.synchronize()
    texts = [(d.data_ptr(), d.numel()) for d in dev]
    seqs, pivots = texts[:len(texts) - npiv], texts[len(texts) - npiv:]
    pivot_group = list(range(npiv))
    if args.worker == "skm":
        os.environ[SWITCH] = "1"
    else:
        os.environ.pop(SWITCH, None)
    with E.Engine(0) as eng:
        call = lambda k: eng.exp2_run(seqs, owner, pivots, pivot_group, k, cs=5000, hist_len=5001)
        for k in (int(x) for x in args.k.split(",")):
            first = call(k)
            digest = hashlib.sha256(b"".join(np.ascontiguousarray(first[f]).tobytes() for f in FIELDS)).hexdigest()[:16]
            eng.sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                call(k)
            eng.sync()
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            eng.profile(True)
            st0 = eng.stats()
            call(k)
            st1 = eng.stats()
            eng.profile(False)
            kern = {n: round(st1["kernels"][n]["ms"] - st0["kernels"][n]["ms"], 4) for n in KERNELS
                    if st1["kernels"][n]["launches"] > st0["kernels"][n]["launches"]}
            print(json.dumps({"k": k, "ms": ms, "digest": digest, "kernel_ms": kern,
                              "form": "skm_cross" if "skm_cross" in kern and st1["retries"] == st0["retries"] else "sets",
                              "cross_launches": st1["kernels"]["skm_cross"]["launches"] - st0["kernels"]["skm_cross"]["launches"],
                              "stats": {n: st1[n] - st0[n] for n in COUNTERS}}), flush=True)
    return 0


def start(cmd, env, limit):
    """A child under `timeout`; its output, or None when it failed (the caller starts nothing more)."""
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, env=env, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        print(f"exit {r.returncode}: {' '.join(cmd)}", file=sys.stderr, flush=True)
        return None
    return r.stdout


def save(out, path):
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--k", default="17,21,31,41,63")
    ap.add_argument("--species", type=int, default=10)
    ap.add_argument("--genomes", type=int, default=5)
    ap.add_argument("--length", type=int, default=5_000_000)
    ap.add_argument("--parent-lib", default=None, help="the library whose set form is the other side (default: this tree's)")
    ap.add_argument("--exp3-ab", default="", help="k values of the type-3 comparison of the two libraries")
    ap.add_argument("--limit", type=int, default=300, help="seconds a child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exp2_skm.json"))
    ap.add_argument("--worker", choices=("sets", "skm"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--texts", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    from khoice_amd import build as kbuild
    lib = kbuild.build_library()
    libs = {"sets": os.path.abspath(args.parent_lib) if args.parent_lib else lib, "skm": lib}
    out = {"shape": f"{args.species} groups x {args.genomes} genomes x {args.length} bp + {args.species} pivots",
           "runs": args.runs, "steps": args.steps,
           "sets_library": "parent commit" if args.parent_lib else "this tree", "k": {}}
    ks = [int(x) for x in args.k.split(",")]
    rows = {k: {"sets": [], "skm": []} for k in ks}
    ok = True
    with tempfile.TemporaryDirectory() as tmp:
        texts = os.path.join(tmp, "texts.npz")
        make_texts(args, texts)
        for _ in range(args.runs):
            for side in ("sets", "skm"):
                env = dict(os.environ, KHOICE_HIP_LIB=libs[side])
                env.pop(SWITCH, None)
                got = ok and start([sys.executable, os.path.abspath(__file__), "--worker", side, "--texts", texts, "--k", args.k,
                                    "--steps", str(args.steps)], env, args.limit)
                if not got:
                    ok = False
                    break
                for line in got.splitlines():
                    if line.startswith("{"):
                        r = json.loads(line)
                        rows[r["k"]][side].append(r)
            if not ok:
                break
    for k in ks:
        sets, skm = rows[k]["sets"], rows[k]["skm"]
        if not sets or not skm:
            continue
        row = {"sets": column([r["ms"] for r in sets]), "skm": column([r["ms"] for r in skm])}
        row["outputs_identical"] = len({r["digest"] for r in sets + skm}) == 1
        row["form"] = skm[-1]["form"] if len({r["form"] for r in skm}) == 1 else "mixed"
        row["kernel_ms"], row["cross_launches"], row["stats"] = skm[-1]["kernel_ms"], skm[-1]["cross_launches"], skm[-1]["stats"]
        row["speedup"] = round(row["sets"]["median_ms"] / row["skm"]["median_ms"], 3)
        margin = 2 * max(row["sets"]["spread"], row["skm"]["spread"])
        row["passes"] = row["form"] == "skm_cross" and row["skm"]["median_ms"] < row["sets"]["median_ms"] * (1 - margin)
        out["k"][str(k)] = row
        print(f"k={k} {json.dumps(row)}", flush=True)
    out["complete"] = ok
    save(out, args.out)
    if ok and args.exp3_ab and args.parent_lib:
        ab = {"tool": f"tools/bench_exp3_skm.py --runs 1 --steps {args.steps} --k {args.exp3_ab}, its skm side; one process per run, "
                      "parent and this tree in turn", "k": {}}
        ms = {}
        with tempfile.TemporaryDirectory() as tmp:
            for i in range(args.runs):
                for side, path in (("parent", libs["sets"]), ("this_tree", lib)):
                    part = os.path.join(tmp, f"{side}{i}.json")
                    got = ok and start([sys.executable, os.path.join(ROOT, "tools", "bench_exp3_skm.py"), "--runs", "1", "--steps", str(args.steps),
                                        "--k", args.exp3_ab, "--out", part], dict(os.environ, KHOICE_HIP_LIB=path), args.limit)
                    if got is None or got is False:
                        ok = False
                        break
                    for k, row in json.load(open(part))["k"].items():
                        assert row["form"] == "skm_cross" and row["outputs_identical"], (side, k, row)
                        ms.setdefault(k, {"parent": [], "this_tree": []})[side] += row["skm"]["ms_per_call"]
                if not ok:
                    break
        for k, m in ms.items():
            if m["parent"] and m["this_tree"]:
                row = {side: column(v) for side, v in m.items()}
                row["within_parent_spread"] = statistics.median(m["this_tree"]) <= statistics.median(m["parent"]) + max(m["parent"]) - min(m["parent"])
                ab["k"][k] = row
                print(f"exp3 k={k} {json.dumps(row)}", flush=True)
        ab["complete"] = ok
        out["exp3_ab"] = ab
        save(out, args.out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
