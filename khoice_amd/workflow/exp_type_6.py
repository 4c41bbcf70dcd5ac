"""Experiment type 6 of khoice (read-level confusion matrix of simulated reads), executed without Snakemake.

workflow/rules/exp_type_6.smk has the rules of type 4 up to the last one, once per read type ("illumina", "ont"): the
pivot databases are built from the reads (`exp6_input/pivot_reads_subset/{read_type}/pivot_N.fa`), and the last rule
runs src/merge_lists.py with `-r`, which classifies every read by the votes of its k-mers (src/merge_lists.py:151-183).

    prepare(...)        the directories, `complex` files and file lists of exp_type_6.smk:24-111
    run_batched(...)    the files of exp6_accuracies/ from one resident engine: one kh_exp6_run per k and read type

Simulating and subsetting the reads (exp_type_6.smk:31-60) is data management: `exp6_input/` is expected as the
reference leaves it.  The reference's tie-breaks are random; here every (k, read type) job seeds `random` with `seed`
first, as one `merge_lists -r DIR --seed N` process per job does, and then draws in the reference's order.  There is
no rule-per-process `run` for this type.
"""
from __future__ import annotations

import glob
import os
import random
from typing import List, Sequence

from .. import merge_lists
from .exp_type_1 import _ops_text

READ_TYPES = ("illumina", "ont")
CSV_HEADER = "k,pivotnum,TP,TN,FP,FN,TP-U,TN-U,FP-U,FN-U\n"


def rest_of_set(work_root: str, num: int) -> List[str]:
    """Base names of exp6_input/rest_of_set/dataset_{num}/*.fna.gz in os.listdir order (exp_type_6.smk:72-75)."""
    d = os.path.join(work_root, f"exp6_input/rest_of_set/dataset_{num}")
    return [n.split(".fna.gz")[0] for n in os.listdir(d) if n.endswith(".fna.gz")]


def prepare(work_root: str, k_values: Sequence[str], num_datasets: int, read_types: Sequence[str] = READ_TYPES) -> None:
    """exp_type_6.smk:24-27,61-111: tmp/, exp6_complex_ops/, exp6_filelists/."""
    base_dir = os.path.abspath(work_root)
    os.makedirs(os.path.join(work_root, "tmp"), exist_ok=True)
    for k in k_values:
        for num in range(1, num_datasets + 1):
            d = os.path.join(work_root, f"exp6_complex_ops/k_{k}/dataset_{num}")
            os.makedirs(d, exist_ok=True)
            ins = [f"exp6_genome_sets/rest_of_set/k_{k}/dataset_{num}/{g}.transformed" for g in rest_of_set(work_root, num)]
            with open(os.path.join(d, f"ops_{num}.txt"), "w") as fd:
                fd.write(_ops_text(ins, f"exp6_unions/rest_of_set/k_{k}/dataset_{num}/dataset_{num}.transformed.combined"))
        for read_type in read_types:
            d = os.path.join(work_root, f"exp6_filelists/k_{k}/{read_type}")
            os.makedirs(d, exist_ok=True)
            pivots, inters = [], []
            for p in range(1, num_datasets + 1):
                pivots.append(f"{base_dir}/exp6_text_dump/k_{k}/{read_type}/pivot/pivot_{p}.txt")
                for num in range(1, num_datasets + 1):
                    inters.append(f"{base_dir}/exp6_text_dump/k_{k}/{read_type}/intersection/pivot_{p}/"
                                  f"pivot_{p}_intersect_dataset_{num}.txt")
            with open(os.path.join(d, "pivots_filelist.txt"), "w") as fd:
                fd.write("".join(x + "\n" for x in pivots))
            with open(os.path.join(d, "intersections_filelist.txt"), "w") as fd:
                fd.write("".join(x + "\n" for x in inters))


def concatenate_accuracies(work_root: str, trial: int = 1) -> dict:
    """exp_type_6.smk:349-362: the header, then `cat exp6_accuracies/{read_type}/values/k_*_accuracy_values.csv` (the
    shell expands the glob in sorted order) into trial_{trial}_short_acc.csv (illumina) and _long_acc.csv (ont)."""
    out = {}
    for name, read_type in (("short", "illumina"), ("long", "ont")):
        path = os.path.join(work_root, f"exp6_accuracies/trial_{trial}_{name}_acc.csv")
        parts = sorted(glob.glob(os.path.join(work_root, f"exp6_accuracies/{read_type}/values/k_*_accuracy_values.csv")))
        with open(path, "w") as fd:
            fd.write(CSV_HEADER)
            for p in parts:
                fd.write(open(p).read())
        out[f"{name}_acc"] = path
    return out


def run_batched(work_root: str, k_values: Sequence, num_datasets: int, seed: int, read_types: Sequence[str] = READ_TYPES,
                device: int = 0, trial: int = 1):
    """The files of exp6_accuracies/{read_type}/ and the two concatenated CSVs from one resident engine.  The genome
    texts are read once; per k and read type one Engine.exp6_run (builds, unions, `set_counts 1`, the votes of every
    read; for k <= 12 the library answers the same from presence bitmaps and a mask table), then the seeded draws on the host.  The unions' histograms go where union_histogram_exp6 writes them."""
    from .. import engine as E
    from concurrent.futures import ThreadPoolExecutor
    k_values = [str(k) for k in k_values]
    prepare(work_root, k_values, num_datasets, read_types)
    with E.Engine(device) as eng:
        paths, owner = [], []
        for num in range(1, num_datasets + 1):
            for g in rest_of_set(work_root, num):
                paths.append(os.path.join(work_root, f"exp6_input/rest_of_set/dataset_{num}/{g}.fna.gz"))
                owner.append(num - 1)
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            texts = list(pool.map(eng.read_fasta, paths))
        reads = {rt: [merge_lists.read_level_reads(os.path.join(work_root, f"exp6_input/pivot_reads_subset/{rt}/pivot_{p}.fa"))
                      for p in range(1, num_datasets + 1)] for rt in read_types}
        for k in k_values:
            for rt in read_types:
                res = eng.exp6_run(texts, owner, reads[rt], int(k), cs=5000, hist_len=5001)
                for num in range(num_datasets):
                    hdir = os.path.join(work_root, f"exp6_unions/rest_of_set/k_{k}/dataset_{num + 1}")
                    os.makedirs(hdir, exist_ok=True)
                    eng.write_histogram_text(os.path.join(hdir, f"dataset_{num + 1}.hist.txt"), res["within_hist"][num], 65535)
                random.seed(seed)
                files = merge_lists.read_level_outputs(res["tie_masks"], num_datasets, k)
                out = os.path.join(os.path.abspath(work_root), f"exp6_accuracies/{rt}") + "/"
                for d in ("values", "confusion_matrix"):
                    os.makedirs(out + d, exist_ok=True)
                merge_lists.write_outputs(out, files)
    return dict(concatenate_accuracies(work_root, trial), processes=0)
