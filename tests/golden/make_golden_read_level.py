"""Golden outputs of the reference's read-level analysis (src/merge_lists.py with -r), recorded under a seed.

Run on the CPU with the reference checked out at REF (the only file of the read-level tests that reads it):

    python tests/golden/make_golden_read_level.py

Writes tests/golden/merge_lists_read_level.json — data only: per case the genomes, the reads files, the text dumps the
reference read, the seed, and the three output texts it wrote after `random.seed(seed)`.
"""
import argparse
import importlib.util
import json
import os
import random
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden import REF                              # noqa: E402  (where the reference is checked out)

from oracle import kmer_oracle as O                      # noqa: E402
from tests import read_level_oracle as RL                # noqa: E402

CASES = [(2, 5, 260), (3, 11, 320), (4, 21, 360), (3, 33, 360), (5, 7, 260)]     # (num_datasets, k, genome length)
READS_PER_PIVOT = 22


def load_reference():
    spec = importlib.util.spec_from_file_location("ref_merge_lists", f"{REF}/src/merge_lists.py")
    ml = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ml)
    return ml


def _mutate(rng, seq, rate):
    t = list(seq)
    for i in range(len(t)):
        if rng.random() < rate:
            t[i] = rng.choice("ACGT")
    return "".join(t)


def _rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def make_reads(rng, pivot, k):
    """Reads cut from the pivot with lengths that straddle k, some of random sequence, blank lines."""
    lengths = [0, k - 1, k, k + 1, 2 * k, 2 * k + 3]
    reads = []
    for i in range(READS_PER_PIVOT):
        n = lengths[i] if i < len(lengths) else rng.randrange(max(1, k - 2), 3 * k + 8)
        if i % 5 == 4:
            reads.append(_rand(rng, n))
        else:
            at = rng.randrange(0, len(pivot) - n + 1)
            reads.append(pivot[at:at + n])
    reads.insert(rng.randrange(1, len(reads)), "")        # a blank line inside the file
    return reads


def reads_file(rng, reads, p):
    """FASTA text: a header line in front of every read; the last file lacks its final newline."""
    lines = []
    for i, r in enumerate(reads):
        lines.append(f">pivot_{p + 1}_read_{i}")
        lines.append(r)
    text = "\n".join(lines)
    return text if p % 2 else text + "\n"


def gen_case(ml, rng, num_datasets, k, length, seed):
    shared = _rand(rng, length // 8)
    pivots, rests = [], []
    for d in range(num_datasets):
        anc = shared + _rand(rng, length - len(shared))
        rests.append([_mutate(rng, anc, 0.01) for _ in range(2)])
        pivots.append(_mutate(rng, anc, 0.015))
    rests[1][1] = rests[0][0]                               # two datasets share a genome
    reads = [make_reads(rng, pivots[p], k) for p in range(num_datasets)]
    files = [reads_file(rng, reads[p], p) for p in range(num_datasets)]
    pivot_dbs = [O.count_records(reads[p], k) for p in range(num_datasets)]           # kmc -ci1 on the reads
    unions = [O.set_counts(O.union_sum([O.set_counts(O.count_records([g], k), 1) for g in gs], 5000), 1) for gs in rests]
    ties = total = 0
    for p in range(num_datasets):
        sets = [{O.decode(c, k) for c in O.intersect(unions[d], pivot_dbs[p], "sum", 255)} for d in range(num_datasets)]
        for _, tie, _ in RL.reads_votes(RL.file_reads(files[p]), k, sets, {O.decode(c, k) for c in pivot_dbs[p]}):
            ties += len(tie) > 1
            total += 1
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(f"{tmp}/out/confusion_matrix")
        os.makedirs(f"{tmp}/out/values")
        os.makedirs(f"{tmp}/reads")
        pivot_paths, inter_paths, pivot_txt, inter_txt = [], [], [], []
        for p in range(num_datasets):
            open(f"{tmp}/reads/pivot_{p + 1}.fa", "w").write(files[p])
            path = f"{tmp}/pivot_{p + 1}.txt"
            txt = O.dump_sorted_text(pivot_dbs[p], k)
            open(path, "w").write(txt)
            pivot_paths.append(path)
            pivot_txt.append(txt)
            for d in range(num_datasets):
                ipath = f"{tmp}/pivot_{p + 1}_intersect_dataset_{d + 1}.txt"
                itxt = O.dump_sorted_text(O.intersect(unions[d], pivot_dbs[p], "sum", 255), k)
                open(ipath, "w").write(itxt)
                inter_paths.append(ipath)
                inter_txt.append(itxt)
        open(f"{tmp}/pivots.txt", "w").write("".join(x + "\n" for x in pivot_paths))
        open(f"{tmp}/inters.txt", "w").write("".join(x + "\n" for x in inter_paths))
        ns = argparse.Namespace(num_datasets=num_datasets, pivot_filelist=f"{tmp}/pivots.txt",
                                intersect_list=f"{tmp}/inters.txt", output_path=f"{tmp}/out/",
                                k=str(k), read_level=[f"{tmp}/reads/"])
        ml.args = ns            # calculate_accuracy_values reads the module-level `args`
        random.seed(seed)
        ml.main(ns)
        outs = {name: open(f"{tmp}/out/{name}").read() for name in (
            f"confusion_matrix/k_{k}_confusion_matrix.txt",
            f"confusion_matrix/k_{k}_confusion_matrix_with_unidentified.txt",
            f"values/k_{k}_accuracy_values.csv")}
    case = {"k": k, "num_datasets": num_datasets, "seed": seed, "rest_of_set": rests, "reads_files": files,
            "pivot_dumps": pivot_txt, "intersection_dumps": inter_txt, "outputs": outs}
    return case, ties, total


def main():
    ml = load_reference()
    rng = random.Random(0x72656164)
    cases, ties, total = [], 0, 0
    for i, (n, k, length) in enumerate(CASES):
        case, t, m = gen_case(ml, rng, n, k, length, 1000 + 17 * i)
        print(f"n={n} k={k}: {t} of {m} reads have more than one tied dataset")
        cases.append(case)
        ties += t
        total += m
    # the draws must be neither trivial nor universal
    assert total / 4 <= ties <= 3 * total / 4, (ties, total)
    path = os.path.join(HERE, "merge_lists_read_level.json")
    with open(path, "w") as fh:
        json.dump({"cases": cases}, fh, separators=(",", ":"))
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f != os.path.basename(path))
    print(os.path.basename(path), os.path.getsize(path), "bytes; ties", ties, "of", total)
    assert os.path.getsize(path) < largest
    print("python", sys.version.split()[0])


if __name__ == "__main__":
    main()
