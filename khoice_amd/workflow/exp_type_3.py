"""Experiment type 3 of khoice (simulated reads of every pivot vs the rest-of-set union of every dataset: the share
of the pivot's k-mers found there), executed without Snakemake.  Mirrors workflow/rules/exp_type_3.smk:176-320 rule
by rule (same directories, `complex` files and shell strings) and offers the batched and the fused form on one
resident engine.

    run(work_root, k_values, num_datasets)        rule-per-process through kmc / kmc_tools on PATH
    run_batched(...)                              same histogram files and CSV, no process launches
    run_fused(...)                                the same again from one kh_exp3_run per k: no set is kept

Inputs: input_type3/{rest_of_set/dataset_N/*.fna.gz, pivot_reads/{illumina,ont}/dataset_N/pivot_N_{read_type}_reads.fa}.
The reads are INPUTS here, plain FASTA as `seqtk seq -a` writes it (exp_type_3.smk:149-171): simulating them
(art_illumina, pbsim, :121-147) is out of scope, as is staging the genomes out of DATABASE_ROOT (:33-55).
"""
from __future__ import annotations

import os
from typing import List, Optional, Sequence

from .. import summarize
from .exp_type_1 import REPO_BIN, _ops_text, _Shell
from .exp_type_2 import _hist_lines

READ_TYPES = ("illumina", "ont")


def rest_of_set(work_root: str, num: int) -> List[str]:
    d = os.path.join(work_root, f"input_type3/rest_of_set/dataset_{num}")
    return [n.split(".fna.gz")[0] for n in os.listdir(d) if n.endswith(".fna.gz")]


def reads_path(read_type: str, num: int) -> str:
    return f"input_type3/pivot_reads/{read_type}/dataset_{num}/pivot_{num}_{read_type}_reads.fa"


def prepare(work_root: str, k_values: Sequence[str], num_datasets: int) -> None:
    """exp_type_3.smk:28-30,57-86: tmp/ and the `complex` operation file of every dataset's union."""
    os.makedirs(os.path.join(work_root, "tmp"), exist_ok=True)
    for k in k_values:
        for num in range(1, num_datasets + 1):
            d = os.path.join(work_root, f"complex_ops/within_groups/k_{k}/dataset_{num}")
            os.makedirs(d, exist_ok=True)
            ins = [f"genome_sets_type3/rest_of_set/k_{k}/dataset_{num}/{g}.transformed" for g in rest_of_set(work_root, num)]
            with open(os.path.join(d, f"within_dataset_{num}.txt"), "w") as fd:
                fd.write(_ops_text(ins, f"within_databases_type3/rest_of_set/k_{k}/dataset_{num}/dataset_{num}.transformed.combined"))


# --- rules (exp_type_3.smk:176-277, names without the `_exp_type_3` suffix) --------------------
def build_kmc_database_on_genome(sh, k, num, genome):
    pre = f"step_1_type3/rest_of_set/k_{k}/dataset_{num}/{genome}"
    sh(f"kmc -fm -m64 -k{k} -ci1 input_type3/rest_of_set/dataset_{num}/{genome}.fna.gz {pre} tmp/",
       [pre + ".kmc_pre", pre + ".kmc_suf"])


def build_kmc_database_on_pivot_reads(sh, k, read_type, num):
    pre = f"step_1_type3/pivot/{read_type}/k_{k}/dataset_{num}/pivot_{num}"
    sh(f"kmc -fm -m64 -k{k} -ci1 {reads_path(read_type, num)} {pre} tmp/", [pre + ".kmc_pre", pre + ".kmc_suf"])


def transform_genome_to_set(sh, k, num, genome):
    out = f"genome_sets_type3/rest_of_set/k_{k}/dataset_{num}/{genome}.transformed"
    sh(f"kmc_tools transform step_1_type3/rest_of_set/k_{k}/dataset_{num}/{genome} set_counts 1 {out}",
       [out + ".kmc_pre", out + ".kmc_suf"])


def _pivot_set(read_type, k, num) -> str:
    return f"genome_sets_type3/pivot/{read_type}/k_{k}/dataset_{num}/pivot_{num}.transformed"


def transform_pivot_reads_to_set(sh, k, read_type, num):
    out = _pivot_set(read_type, k, num)
    sh(f"kmc_tools transform step_1_type3/pivot/{read_type}/k_{k}/dataset_{num}/pivot_{num} set_counts 1 {out}",
       [out + ".kmc_pre", out + ".kmc_suf"])


def within_group_union(sh, k, num):
    out = f"within_databases_type3/rest_of_set/k_{k}/dataset_{num}/dataset_{num}.transformed.combined"
    sh(f"kmc_tools complex complex_ops/within_groups/k_{k}/dataset_{num}/within_dataset_{num}.txt",
       [out + ".kmc_pre", out + ".kmc_suf"])


def _intersect_prefix(read_type, pivot_num, k, num) -> str:
    return (f"within_dataset_results_type3/{read_type}/pivot_{pivot_num}/k_{k}/dataset_{num}/intersect/"
            f"dataset_{num}_pivot_intersect_group")


def pivot_intersect_within_group(sh, k, read_type, pivot_num, num):
    out = _intersect_prefix(read_type, pivot_num, k, num)
    union = f"within_databases_type3/rest_of_set/k_{k}/dataset_{num}/dataset_{num}.transformed.combined"
    sh(f"kmc_tools simple {_pivot_set(read_type, k, pivot_num)} {union} intersect {out} -ocsum",
       [out + ".kmc_pre", out + ".kmc_suf"])


def intersection_histogram(sh, k, read_type, pivot_num, num):
    src = _intersect_prefix(read_type, pivot_num, k, num)
    sh(f"kmc_tools transform {src} histogram {src}.hist.txt", [src + ".hist.txt"])


def pivot_histogram(sh, k, read_type, pivot_num):
    src = _pivot_set(read_type, k, pivot_num)
    sh(f"kmc_tools transform {src} histogram {src}.hist.txt", [src + ".hist.txt"])


def _hist_paths(k_values: Sequence[str], num_datasets: int) -> List[str]:
    """get_all_histogram_files (exp_type_3.smk:102-112): read type, pivot, k; the pivot's histogram, then one per dataset."""
    out = []
    for read_type in READ_TYPES:
        for pivot_num in range(1, num_datasets + 1):
            for k in k_values:
                out.append(_pivot_set(read_type, k, pivot_num) + ".hist.txt")
                out += [_intersect_prefix(read_type, pivot_num, k, num) + ".hist.txt" for num in range(1, num_datasets + 1)]
    return out


def _csv_stage(work_root: str, k_values: Sequence[str], num_datasets: int) -> str:
    cwd = os.getcwd()
    os.chdir(work_root)
    try:
        text = summarize.intersection_percent_csv(_hist_paths(k_values, num_datasets), num_datasets)
        os.makedirs("final_analysis_type3", exist_ok=True)
        with open("final_analysis_type3/final_analysis_type3.csv", "w") as fh:
            fh.write(text)
    finally:
        os.chdir(cwd)
    return text


def run(work_root: str, k_values: Sequence, num_datasets: int, bin_dir: Optional[str] = REPO_BIN):
    """Target final_analysis_type3/final_analysis_type3.csv, one process per rule instance."""
    k_values = [str(k) for k in k_values]
    prepare(work_root, k_values, num_datasets)
    sh = _Shell(work_root, bin_dir)
    for k in k_values:
        for num in range(1, num_datasets + 1):
            for g in rest_of_set(work_root, num):
                build_kmc_database_on_genome(sh, k, num, g)
                transform_genome_to_set(sh, k, num, g)
            within_group_union(sh, k, num)
        for read_type in READ_TYPES:
            for p in range(1, num_datasets + 1):
                build_kmc_database_on_pivot_reads(sh, k, read_type, p)
                transform_pivot_reads_to_set(sh, k, read_type, p)
                pivot_histogram(sh, k, read_type, p)
                for num in range(1, num_datasets + 1):
                    pivot_intersect_within_group(sh, k, read_type, p, num)
                    intersection_histogram(sh, k, read_type, p, num)
    return {"csv": _csv_stage(work_root, k_values, num_datasets), "processes": sh.launched}


def _read_texts(eng, work_root: str, num_datasets: int):
    """The texts of every rest-of-set genome (with its dataset, 0-based) and of every read set (read type major)."""
    from concurrent.futures import ThreadPoolExecutor
    paths, owner = [], []
    for num in range(1, num_datasets + 1):
        for g in rest_of_set(work_root, num):
            paths.append(os.path.join(work_root, f"input_type3/rest_of_set/dataset_{num}/{g}.fna.gz"))
            owner.append(num - 1)
    pivots = [(read_type, num) for read_type in READ_TYPES for num in range(1, num_datasets + 1)]
    pivot_paths = [os.path.join(work_root, reads_path(read_type, num)) for read_type, num in pivots]
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        texts = list(pool.map(eng.read_fasta, paths + pivot_paths))
    return texts[:len(paths)], owner, texts[len(paths):], pivots


def _out_path(work_root: str, rel: str) -> str:
    path = os.path.join(work_root, rel)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    return path


def run_batched(work_root: str, k_values: Sequence, num_datasets: int, device: int = 0):
    """Same *.hist.txt files and CSV from one resident engine: one batched build per k, one union per dataset and one
    intersect (-ocsum) per (read set, dataset), all on sets that never leave HBM."""
    from .. import engine as E
    k_values = [str(k) for k in k_values]
    prepare(work_root, k_values, num_datasets)
    with E.Engine(device) as eng:
        genomes, owner, reads, pivots = _read_texts(eng, work_root, num_datasets)
        for k in k_values:
            plain = eng.build_batch(genomes + reads, int(k), ci=1, with_counts=False)
            gsets, psets = plain[:len(genomes)], plain[len(genomes):]
            unions = [eng.union_sum([s for s, o in zip(gsets, owner) if o == num], 5000) for num in range(num_datasets)]
            for pset, (read_type, p) in zip(psets, pivots):
                pset.histogram_file(_hist_lines(pset.counter_max()), _out_path(work_root, _pivot_set(read_type, k, p) + ".hist.txt"))
                for num in range(num_datasets):
                    res = eng.intersect(pset, unions[num], "sum")
                    res.histogram_file(_hist_lines(res.counter_max()),
                                       _out_path(work_root, _intersect_prefix(read_type, p, k, num + 1) + ".hist.txt"))
    return {"csv": _csv_stage(work_root, k_values, num_datasets), "processes": 0}


def run_fused(work_root: str, k_values: Sequence, num_datasets: int, device: int = 0):
    """The files and CSV of run_batched from one Engine.exp3_run per k (kh_exp3_run: presence bitmaps for k <= 12, the
    set operations inside the library above): the texts are read once, the intersect histograms are the call's
    inter_hist, a pivot's own histogram its distinct count in line 1.  With KHOICE_EXP3_SKM=1 in the environment the
    library answers k = 17 .. 63 from super-k-mer records (k_skm_cross) instead — the switch is read inside
    kh_exp3_run at every call, so this runner gets the form without a change; the files are the same."""
    import numpy as np
    from .. import engine as E
    k_values = [str(k) for k in k_values]
    prepare(work_root, k_values, num_datasets)
    cs, lines = 5000, _hist_lines(5000)       # the -cs5000 unions give `simple` its counter range, as in run_batched
    with E.Engine(device) as eng:
        genomes, owner, reads, pivots = _read_texts(eng, work_root, num_datasets)
        for k in k_values:
            res = eng.exp3_run(genomes, owner, reads, int(k), cs=cs, hist_len=cs + 1)
            for i, (read_type, p) in enumerate(pivots):
                own = np.zeros(2, dtype=np.uint64)
                own[1] = res["distinct_per_pivot"][i]
                eng.write_histogram_text(_out_path(work_root, _pivot_set(read_type, k, p) + ".hist.txt"), own, _hist_lines(1))
                for num in range(num_datasets):
                    eng.write_histogram_text(_out_path(work_root, _intersect_prefix(read_type, p, k, num + 1) + ".hist.txt"),
                                             res["inter_hist"][i][num], lines)
    return {"csv": _csv_stage(work_root, k_values, num_datasets), "processes": 0}
