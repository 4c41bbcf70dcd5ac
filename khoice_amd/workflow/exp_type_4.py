"""Experiment type 4 of khoice (out-pivot confusion matrix), executed without Snakemake.

Mirrors workflow/rules/exp_type_4.smk rule by rule — same directories, same `complex` files and
file lists, same shell strings — so that whatever `kmc` / `kmc_tools` are first on PATH receive
the argv the reference gives KMC; the last rule calls the merge_lists drop-in
(`python3 -m khoice_amd.merge_lists`, same options as src/merge_lists.py).

    run(work_root, k_values, num_datasets)            rule-per-process
    run_batched(...)                                  same final files from one resident engine:
                                                      no text dumps, no D x D intersections
    run_fused(...)                                    the same again from one kh_exp4_run per k: no set is kept

Staging of `input_type4/` out of DATABASE_ROOT (exp_type_4.smk:31-51) is data management, not
k-mer work: both entries expect input_type4/{rest_of_set/dataset_N/*.fna.gz, pivot/pivot_N.fna.gz}.
"""
from __future__ import annotations

import glob
import os
import sys
from typing import List, Optional, Sequence

from .. import merge_lists
from .exp_type_1 import REPO_BIN, _ops_text, _Shell

REPO_ROOT = os.path.dirname(REPO_BIN)


def rest_of_set(work_root: str, num: int) -> List[str]:
    """Base names of input_type4/rest_of_set/dataset_{num}/*.fna.gz in os.listdir order
    (exp_type_4.smk:63-66,113-116)."""
    d = os.path.join(work_root, f"input_type4/rest_of_set/dataset_{num}")
    return [n.split(".fna.gz")[0] for n in os.listdir(d) if n.endswith(".fna.gz")]


def prepare(work_root: str, k_values: Sequence[str], num_datasets: int) -> None:
    """exp_type_4.smk:27-29,53-101: tmp/, complex_ops_type_4/, filelists_type_4/."""
    base_dir = os.path.abspath(work_root)
    os.makedirs(os.path.join(work_root, "tmp"), exist_ok=True)
    for k in k_values:
        for num in range(1, num_datasets + 1):
            d = os.path.join(work_root, f"complex_ops_type_4/k_{k}/dataset_{num}")
            os.makedirs(d, exist_ok=True)
            ins = [f"genome_sets_type_4/rest_of_set/k_{k}/dataset_{num}/{g}.transformed"
                   for g in rest_of_set(work_root, num)]
            with open(os.path.join(d, f"ops_{num}.txt"), "w") as fd:
                fd.write(_ops_text(ins, f"unions_type_4/rest_of_set/k_{k}/dataset_{num}/dataset_{num}.transformed.combined"))
        d = os.path.join(work_root, f"filelists_type_4/k_{k}")
        os.makedirs(d, exist_ok=True)
        pivots, inters = [], []
        for p in range(1, num_datasets + 1):
            pivots.append(f"{base_dir}/text_dump_type_4/k_{k}/pivot/pivot_{p}.txt")
            for num in range(1, num_datasets + 1):
                inters.append(f"{base_dir}/text_dump_type_4/k_{k}/intersection/pivot_{p}/pivot_{p}_intersect_dataset_{num}.txt")
        with open(os.path.join(d, "pivots_filelist.txt"), "w") as fd:
            fd.write("".join(x + "\n" for x in pivots))
        with open(os.path.join(d, "intersections_filelist.txt"), "w") as fd:
            fd.write("".join(x + "\n" for x in inters))


# --- rules (names as in exp_type_4.smk:139-294, without the `_exp_type_4` suffix) -------------
def build_kmc_database_on_genome(sh, k, num, genome):
    pre = f"step_1_type_4/rest_of_set/k_{k}/dataset_{num}/{genome}"
    sh(f"kmc -fm -m64 -k{k} -ci1 input_type4/rest_of_set/dataset_{num}/{genome}.fna.gz {pre} tmp/",
       [pre + ".kmc_pre", pre + ".kmc_suf"])


def build_kmc_database_on_pivot(sh, k, num):
    pre = f"step_1_type_4/pivot/k_{k}/dataset_{num}/pivot_{num}"
    sh(f"kmc -fm -m64 -k{k} -ci1 input_type4/pivot/pivot_{num}.fna.gz {pre} tmp/",
       [pre + ".kmc_pre", pre + ".kmc_suf"])


def transform_genome_to_set(sh, k, num, genome):
    src = f"step_1_type_4/rest_of_set/k_{k}/dataset_{num}/{genome}"
    out = f"genome_sets_type_4/rest_of_set/k_{k}/dataset_{num}/{genome}.transformed"
    sh(f"kmc_tools transform {src} set_counts 1 {out}\nrm {src}.kmc_pre {src}.kmc_suf",
       [out + ".kmc_pre", out + ".kmc_suf"])


def rest_of_set_union(sh, k, num):
    out = f"unions_type_4/rest_of_set/k_{k}/dataset_{num}/dataset_{num}.transformed.combined"
    sh(f"kmc_tools complex complex_ops_type_4/k_{k}/dataset_{num}/ops_{num}.txt", [out + ".kmc_pre", out + ".kmc_suf"])


def union_histogram(sh, k, num):
    src = f"unions_type_4/rest_of_set/k_{k}/dataset_{num}/dataset_{num}.transformed.combined"
    out = f"unions_type_4/rest_of_set/k_{k}/dataset_{num}/dataset_{num}.hist.txt"
    sh(f"kmc_tools transform {src} histogram {out}", [out])


def transform_union_to_set(sh, k, num):
    src = f"unions_type_4/rest_of_set/k_{k}/dataset_{num}/dataset_{num}.transformed.combined"
    out = f"genome_sets_type_4/unions_type_4/k_{k}/dataset_{num}/dataset_{num}.transformed.combined.transformed"
    sh(f"kmc_tools transform {src} set_counts 1 {out}\nrm {src}.kmc_pre {src}.kmc_suf",
       [out + ".kmc_pre", out + ".kmc_suf"])


def pivot_intersect(sh, k, pivot_num, num):
    a = f"genome_sets_type_4/unions_type_4/k_{k}/dataset_{num}/dataset_{num}.transformed.combined.transformed"
    b = f"step_1_type_4/pivot/k_{k}/dataset_{pivot_num}/pivot_{pivot_num}"
    out = f"intersection_results_type_4/k_{k}/pivot_{pivot_num}/pivot_{pivot_num}_intersect_dataset_{num}"
    sh(f"kmc_tools simple {a} {b} intersect {out} -ocsum", [out + ".kmc_pre", out + ".kmc_suf"])


def intersection_histogram(sh, k, pivot_num, num):
    src = f"intersection_results_type_4/k_{k}/pivot_{pivot_num}/pivot_{pivot_num}_intersect_dataset_{num}"
    sh(f"kmc_tools transform {src} histogram {src}.hist.txt", [src + ".hist.txt"])


def pivot_text_dump(sh, k, num):
    out = f"text_dump_type_4/k_{k}/pivot/pivot_{num}.txt"
    sh(f"kmc_tools transform step_1_type_4/pivot/k_{k}/dataset_{num}/pivot_{num} dump -s {out}", [out])


def intersection_text_dump(sh, k, pivot_num, num):
    src = f"intersection_results_type_4/k_{k}/pivot_{pivot_num}/pivot_{pivot_num}_intersect_dataset_{num}"
    out = f"text_dump_type_4/k_{k}/intersection/pivot_{pivot_num}/pivot_{pivot_num}_intersect_dataset_{num}.txt"
    sh(f"kmc_tools transform {src} dump -s {out}", [out])


def run_merge_list(sh, k, num_datasets, merge_cmd):
    base = os.path.abspath(sh.cwd)
    outs = [f"accuracies_type_4/values/k_{k}_accuracy_values.csv",
            f"accuracies_type_4/confusion_matrix/k_{k}_confusion_matrix.txt"]
    sh(f"{merge_cmd} -p {base}/filelists_type_4/k_{k}/pivots_filelist.txt "
       f"-i {base}/filelists_type_4/k_{k}/intersections_filelist.txt -o {base}/accuracies_type_4/ "
       f"-n {num_datasets} -k {k}\n"
       f"rm text_dump_type_4/k_{k}/intersection/pivot_*/pivot_*_intersect_dataset_*.txt\n"
       f"rm text_dump_type_4/k_{k}/pivot/pivot_*.txt", outs)


def concatenate_accuracies(work_root: str) -> str:
    """`cat accuracies_type_4/values/*.csv > accuracies_type_4/accuracy_values.csv`
    (exp_type_4.smk:296-303): the shell expands the glob in sorted order."""
    out = os.path.join(work_root, "accuracies_type_4/accuracy_values.csv")
    parts = sorted(glob.glob(os.path.join(work_root, "accuracies_type_4/values/*.csv")))
    with open(out, "w") as fd:
        for p in parts:
            fd.write(open(p).read())
    return out


def run(work_root: str, k_values: Sequence, num_datasets: int, bin_dir: Optional[str] = REPO_BIN,
        merge_cmd: Optional[str] = None):
    """Target accuracies_type_4/accuracy_values.csv, one process per rule instance."""
    k_values = [str(k) for k in k_values]
    prepare(work_root, k_values, num_datasets)
    sh = _Shell(work_root, bin_dir)
    sh.env["PYTHONPATH"] = REPO_ROOT + os.pathsep + sh.env.get("PYTHONPATH", "")
    merge_cmd = merge_cmd or f"{sys.executable} -m khoice_amd.merge_lists"
    for k in k_values:
        for num in range(1, num_datasets + 1):
            for g in rest_of_set(work_root, num):
                build_kmc_database_on_genome(sh, k, num, g)
                transform_genome_to_set(sh, k, num, g)
            build_kmc_database_on_pivot(sh, k, num)
            rest_of_set_union(sh, k, num)
            union_histogram(sh, k, num)
            transform_union_to_set(sh, k, num)
        for p in range(1, num_datasets + 1):
            pivot_text_dump(sh, k, p)
            for num in range(1, num_datasets + 1):
                pivot_intersect(sh, k, p, num)
                intersection_histogram(sh, k, p, num)
                intersection_text_dump(sh, k, p, num)
        run_merge_list(sh, k, num_datasets, merge_cmd)
    return {"accuracy_values": concatenate_accuracies(work_root), "processes": sh.launched}


def run_batched(work_root: str, k_values: Sequence, num_datasets: int, device: int = 0):
    """Same accuracies_type_4/ files from one resident engine.  Per k: one batched build of every
    rest-of-set genome and pivot, one union per dataset, then one membership search per pivot
    (kh_confusion_row) instead of D x D intersection databases and their text dumps."""
    from .. import engine as E
    from concurrent.futures import ThreadPoolExecutor
    k_values = [str(k) for k in k_values]
    prepare(work_root, k_values, num_datasets)
    for d in ("accuracies_type_4/values", "accuracies_type_4/confusion_matrix"):
        os.makedirs(os.path.join(work_root, d), exist_ok=True)
    with E.Engine(device) as eng:
        paths, owner = [], []
        for num in range(1, num_datasets + 1):
            for g in rest_of_set(work_root, num):
                paths.append(os.path.join(work_root, f"input_type4/rest_of_set/dataset_{num}/{g}.fna.gz"))
                owner.append(num - 1)
        pivot_paths = [os.path.join(work_root, f"input_type4/pivot/pivot_{num}.fna.gz")
                       for num in range(1, num_datasets + 1)]
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            texts = list(pool.map(eng.read_fasta, paths + pivot_paths))
        for k in k_values:
            ki = int(k)
            plain = eng.build_batch(texts[:len(paths)], ki, ci=1, with_counts=False)
            pivots = eng.build_batch(texts[len(paths):], ki, ci=1, with_counts=True)
            unions = []
            for num in range(num_datasets):
                members = [s for s, o in zip(plain, owner) if o == num]
                union = eng.union_sum(members, 5000)
                hdir = os.path.join(work_root, f"unions_type_4/rest_of_set/k_{k}/dataset_{num + 1}")
                os.makedirs(hdir, exist_ok=True)
                union.histogram_file(65535, os.path.join(hdir, f"dataset_{num + 1}.hist.txt"))
                unions.append(union.set_counts(1))
            files = merge_lists.confusion_from_sets(eng, pivots, [unions] * num_datasets, num_datasets, k)
            merge_lists.write_outputs(os.path.join(os.path.abspath(work_root), "accuracies_type_4") + "/", files)
    return {"accuracy_values": concatenate_accuracies(work_root), "processes": 0}


def run_fused(work_root: str, k_values: Sequence, num_datasets: int, device: int = 0):
    """The files of run_batched from one Engine.exp4_run per k (kh_exp4_run: presence bitmaps and records in code
    order for k <= 12, the set operations inside the library otherwise): the texts are read once, no set comes back
    to Python."""
    from .. import engine as E
    from concurrent.futures import ThreadPoolExecutor
    k_values = [str(k) for k in k_values]
    prepare(work_root, k_values, num_datasets)
    for d in ("accuracies_type_4/values", "accuracies_type_4/confusion_matrix"):
        os.makedirs(os.path.join(work_root, d), exist_ok=True)
    with E.Engine(device) as eng:
        paths, owner = [], []
        for num in range(1, num_datasets + 1):
            for g in rest_of_set(work_root, num):
                paths.append(os.path.join(work_root, f"input_type4/rest_of_set/dataset_{num}/{g}.fna.gz"))
                owner.append(num - 1)
        pivot_paths = [os.path.join(work_root, f"input_type4/pivot/pivot_{num}.fna.gz")
                       for num in range(1, num_datasets + 1)]
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            texts = list(pool.map(eng.read_fasta, paths + pivot_paths))
        for k in k_values:
            res = eng.exp4_run(texts[:len(paths)], owner, texts[len(paths):], int(k), cs=5000, hist_len=5001)
            for num in range(num_datasets):
                hdir = os.path.join(work_root, f"unions_type_4/rest_of_set/k_{k}/dataset_{num + 1}")
                os.makedirs(hdir, exist_ok=True)
                eng.write_histogram_text(os.path.join(hdir, f"dataset_{num + 1}.hist.txt"), res["within_hist"][num], 65535)
            files = merge_lists.confusion_from_rows(res["rows"], res["unique"], num_datasets, k)
            merge_lists.write_outputs(os.path.join(os.path.abspath(work_root), "accuracies_type_4") + "/", files)
    return {"accuracy_values": concatenate_accuracies(work_root), "processes": 0}
