"""Experiment type 3 without a GPU: the inputs of tests/test_gpu_exp3.py are what they claim to be (a green GPU run
cannot be green by missing its target), workflow/exp_type_3.py::run through the oracle-backed stand-in executables
(tests/fakebin) against the oracle's direct answer, the CSV stage, and the stand-in read generator."""
import os

import numpy as np
import pytest

from khoice_amd import summarize as S
from khoice_amd import synth
from khoice_amd.workflow import exp_type_3 as W3
from oracle import kmer_oracle as O
from tests import test_gpu_exp2_bmp as X2
from tests import test_gpu_exp3 as G3

FAKE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fakebin")


# ---------------------------------------------------------------- the planted cases
@pytest.mark.parametrize("k", G3.PLANT_K)
def test_planted_codes_are_canonical_and_lie_on_the_edges(k):
    """tests/test_gpu_exp2_bmp.py proves where edge_codes lie (test_planted_codes_lie_on_the_edges); here: the planted
    case holds every one of them, each at the bit, word and range its name says."""
    seqs, group_of, pivots, plants = G3.planted_case(k)
    edges = X2.edge_codes(k)
    codes = [c for c, *_ in plants]
    assert len(set(codes)) == len(codes) and all(X2.is_canonical(c, k) for c in codes)
    by_what = {what: c for c, _, _, _, _, what in plants if what != "fill"}
    assert by_what == edges
    ncodes, rbits = 4 ** k, min(X2.RANGE_BITS, 2 * k)
    nranges = ncodes >> rbits
    assert nranges == {5: 1, 8: 1, 11: 4, 12: 16}[k]
    for r in range(nranges):                                                # the two codes either side of every range edge
        assert by_what[f"range{r}_first"] >> rbits == r == by_what[f"range{r}_last"] >> rbits
        assert not any(X2.is_canonical(c, k) for c in range(r << rbits, by_what[f"range{r}_first"]))
        assert not any(X2.is_canonical(c, k) for c in range(by_what[f"range{r}_last"] + 1, (r + 1) << rbits))
    top = by_what[f"range{nranges - 1}_last"]                               # the last word of the bitmap that holds anything
    assert top == max(c for c in range(ncodes - (1 << rbits), ncodes) if X2.is_canonical(c, k))
    assert by_what["range0_first"] == 0 and by_what["bit0"] % 64 == 0 and by_what["bit0"] > 0
    if k >= 6:
        assert by_what["bit63"] % 64 == 63
        assert by_what["wave_last_word"] // 64 == 63 and by_what["wave_first_word"] // 64 == 64
    else:
        assert ncodes // 64 == 16 and top // 64 == 15                       # k = 5: one wave of 16 words


@pytest.mark.parametrize("k", G3.PLANT_K)
def test_planted_case_holds_every_count_of_every_group_for_every_pivot(k):
    seqs, group_of, pivots, plants = G3.planted_case(k)
    ng = len(G3.PLANT_SIZES)
    assert max(len(t) for t in seqs + pivots) > 2 * G3.SPLIT and min(len(t) for t in seqs + pivots) > G3.TILE
    for gi, text in enumerate(seqs):                                        # every code in exactly the texts it was meant for
        assert set(X2.plain_set(text, k)) == {c for c, _, _, genomes, _, _ in plants if gi in genomes}
    for p, text in enumerate(pivots):
        assert set(X2.plain_set(text, k)) == {c for c, ps, *_ in plants if p in ps}
    for code, ps, vec, genomes, rc, _ in plants:
        assert [sum(group_of[gi] == g for gi in genomes) for g in range(ng)] == list(vec) and len(set(genomes)) == len(genomes)
        if rc:                                                              # the genomes spell the other strand
            other = X2.kmer_text(X2.revcomp_code(code, k), k)
            assert other != X2.kmer_text(code, k)
            for gi in genomes:
                recs = seqs[gi].decode().split("N")
                assert other in recs and X2.kmer_text(code, k) not in recs
    assert any(rc and genomes and ps for _, ps, _, genomes, rc, _ in plants)
    assert any(ps and not genomes for _, ps, _, genomes, _, _ in plants)    # held by a pivot and no group
    assert any(genomes and not ps for _, ps, _, genomes, _, _ in plants)    # held by groups and no pivot
    # a code of group g counts for every pivot that holds it: pivot 3 belongs to no group's number, pairs share codes
    assert any(len(ps) > 1 and any(vec) for _, ps, vec, *_ in plants)
    want, occ = G3.planted_answer(k)
    theirs = G3.oracle(seqs, group_of, pivots, k)
    for f in G3.FIELDS:
        assert (want[f] == theirs[f]).all(), f
    for p in range(len(pivots)):
        for g, n in enumerate(G3.PLANT_SIZES):
            assert all(occ[p][g][v] > 0 for v in range(n + 1)), (p, g)      # v = 0 .. size, every one planted
            assert all(theirs["inter_hist"][p, g, v + 1] > 0 for v in range(1, n + 1))
            assert theirs["inter_hist"][p, g].sum() == sum(occ[p][g][1:]) < theirs["distinct_per_pivot"][p]


def test_other_cases_are_what_they_claim():
    seqs, group_of, pivots = G3.walk_case(6)
    assert [group_of.count(g) for g in range(5)] == [1, 3, 4, 17, 33] == list(G3.WALK_SIZES)
    assert [n.bit_length() for n in G3.WALK_SIZES] == [1, 2, 3, 5, 6]       # the slice count changes
    assert (len(seqs) + 6) % 16 == 0 and (len(seqs) + 6) % 4 == 0
    assert all((len(seqs) + n) % 16 and (len(seqs) + n) % 4 for n in (7, 15, 5))
    assert 6 + 1 + 3 + 4 < 16 < 6 + 1 + 3 + 4 + 17                          # pivots and three groups in the first round of 16
    k = 9
    seqs, group_of, pivots, names = G3.read_shaped_case(k)
    recs = pivots[names.index("edge_records")].split(b"\n")
    assert [len(r) for r in recs[:4]] == [k - 1, k, k + 1, 0] and set(recs[4]) == set(b"N") and recs[5].islower()
    assert pivots[names.index("empty")] == b"" and 0 < len(pivots[names.index("shorter_than_k")]) < k
    assert pivots[names.index("a_genome")] == seqs[2] and group_of[2] == 1
    want = G3.oracle(seqs, group_of, pivots, k)
    p = names.index("a_genome")
    assert want["inter_hist"][p, 1].sum() == want["distinct_per_pivot"][p] > 0   # nothing of it is missing from group 1
    assert want["distinct_per_pivot"][names.index("edge_records")] > 2
    assert max(len(r) for r in pivots[names.index("reads")].split(b"\n")) > G3.TILE   # reads straddle tiles of 64
    seqs, group_of, pivots = G3.species(8_000)
    assert len(pivots) == 6 and len(seqs) == 9
    assert (40 - 9) // (9 + 1) == 3 and (19 - 9) // (9 + 1) == 1 and 2 * 9 + 1 > 18   # the budgets of test_exp3_pivot_batches


# ---------------------------------------------------------------- the rule runner through the stand-ins
def expected_type3_outputs(root, k_values, n):
    """Histogram texts of experiment type 3 from the input files by the oracle (sets as dicts), and the CSV by a
    restatement of exp_type_3.smk:286-320 on those numbers: nothing from the rule plumbing or from summarize."""
    files = {}
    rows = {}
    for k in k_values:
        unions = []
        for num in range(1, n + 1):
            sets = [O.set_counts(O.build(O.read_fasta_bytes(
                os.path.join(root, f"input_type3/rest_of_set/dataset_{num}/{g}.fna.gz")), k), 1)
                for g in W3.rest_of_set(root, num)]
            unions.append(O.union_sum(sets, 5000))
        for read_type in W3.READ_TYPES:
            for p in range(1, n + 1):
                pivot = O.set_counts(O.build(O.read_fasta_bytes(os.path.join(root, W3.reads_path(read_type, p))), k), 1)
                files[f"genome_sets_type3/pivot/{read_type}/k_{k}/dataset_{p}/pivot_{p}.transformed.hist.txt"] = \
                    O.histogram_text(pivot, 255)
                for num in range(1, n + 1):
                    # `simple` without -cs: the counter range of the -cs5000 union (two counter bytes: 65535 lines)
                    inter = O.intersect(pivot, unions[num - 1], "sum", 5000)
                    files[f"within_dataset_results_type3/{read_type}/pivot_{p}/k_{k}/dataset_{num}/intersect/"
                          f"dataset_{num}_pivot_intersect_group.hist.txt"] = O.histogram_text(inter, 65535)
                    share = round(len(inter) / len(pivot), 4)                # the percentage, restated
                    rows[(read_type, p, k, num)] = f"{read_type},{p},{k},{num},{share}\n"
    csv = "read_type,pivot_num,k,dataset_num,intersection_percent\n" + "".join(
        rows[(rt, p, k, num)] for rt in W3.READ_TYPES for p in range(1, n + 1) for k in k_values for num in range(1, n + 1))
    return files, csv


def test_exp_type_3_dag_through_standins(tmp_path):
    """exp_type_3.smk rule by rule with oracle-backed stand-ins == the oracle's direct answer."""
    root = str(tmp_path / "work")
    os.makedirs(root)
    synth.write_type3_tree(root, 3, 2, 3000, 40)
    ks, n = [9, 21], 3
    out = W3.run(root, ks, n, bin_dir=FAKE)
    # per k: build + set_counts per genome and one union per dataset; per read type and pivot build, set_counts and
    # histogram, and intersect + histogram per dataset
    assert out["processes"] == len(ks) * (n * (2 * 2 + 1) + 2 * n * (3 + 2 * n)) == 138
    files, csv = expected_type3_outputs(root, ks, n)
    assert len(files) == 2 * n * len(ks) * (1 + n)
    for rel, text in files.items():
        assert open(os.path.join(root, rel)).read() == text, rel
    assert out["csv"] == csv == open(os.path.join(root, "final_analysis_type3/final_analysis_type3.csv")).read()
    assert csv.count("\n") == 1 + 2 * n * len(ks) * n
    shares = [float(line.rsplit(",", 1)[1]) for line in csv.splitlines()[1:]]
    assert all(0 <= s <= 1 for s in shares) and len(set(shares)) > 4


def test_ops_file_matches_reference_text(tmp_path):
    """What exp_type_3.smk:77-86 writes, restated line by line."""
    root = str(tmp_path)
    synth.write_type3_tree(root, 2, 3, 400, 2)
    W3.prepare(root, ["7", "31"], 2)
    for k in ("7", "31"):
        for num in (1, 2):
            names = [f.split(".fna.gz")[0] for f in os.listdir(os.path.join(root, f"input_type3/rest_of_set/dataset_{num}"))
                     if f.endswith(".fna.gz")]
            assert sorted(names) == [f"sp{num}_g{g}" for g in range(3)]     # the pivot genome is not among them
            paths = [f"genome_sets_type3/rest_of_set/k_{k}/dataset_{num}/{b}.transformed" for b in names]
            want = "INPUT:\n"
            result = "("
            for i, path in enumerate(paths):
                want += f"set{i + 1} = {path}\n"
                result += "set{} + ".format(i + 1)
            result = result[:-2] + ")"
            want += "OUTPUT:\n"
            want += f"within_databases_type3/rest_of_set/k_{k}/dataset_{num}/dataset_{num}.transformed.combined = {result}\n"
            want += "OUTPUT_PARAMS:\n-cs5000\n"
            got = open(os.path.join(root, f"complex_ops/within_groups/k_{k}/dataset_{num}/within_dataset_{num}.txt")).read()
            assert got == want
    assert os.path.isdir(os.path.join(root, "tmp"))


# ---------------------------------------------------------------- the CSV stage
def write_hist(path, counts):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("".join(f"{c}\t{n}\n" for c, n in enumerate(counts, 1)))


def csv_tree(tmp_path, monkeypatch, totals, inter):
    """totals[(read_type, pivot, k)] and inter[(read_type, pivot, k, dataset)] (lists of line values) as files under
    tmp_path, which becomes the working directory; returns the paths in the order of get_all_histogram_files."""
    monkeypatch.chdir(tmp_path)
    for (rt, p, k), counts in totals.items():
        write_hist(W3._pivot_set(rt, k, p) + ".hist.txt", counts)
    for (rt, p, k, num), counts in inter.items():
        write_hist(W3._intersect_prefix(rt, p, k, num) + ".hist.txt", counts)


def test_intersection_percent_csv(tmp_path, monkeypatch):
    ks, n = ["9", "21"], 2
    totals, inter = {}, {}
    i = 0
    for rt in W3.READ_TYPES:
        for p in (1, 2):
            for k in ks:
                i += 1
                totals[(rt, p, k)] = [7 * i + 3, 0, 0]
                for num in (1, 2):
                    inter[(rt, p, k, num)] = [0, i, num, 1]
    inter[("ont", 2, "21", 2)] = [0, 1, 1, 0]
    totals[("ont", 2, "21")] = [3, 0, 0]                                    # 2 / 3 = 0.6667: four places
    csv_tree(tmp_path, monkeypatch, totals, inter)
    paths = W3._hist_paths(ks, n)
    assert paths[:4] == ["genome_sets_type3/pivot/illumina/k_9/dataset_1/pivot_1.transformed.hist.txt",
                         "within_dataset_results_type3/illumina/pivot_1/k_9/dataset_1/intersect/dataset_1_pivot_intersect_group.hist.txt",
                         "within_dataset_results_type3/illumina/pivot_1/k_9/dataset_2/intersect/dataset_2_pivot_intersect_group.hist.txt",
                         "genome_sets_type3/pivot/illumina/k_21/dataset_1/pivot_1.transformed.hist.txt"]
    assert len(paths) == 2 * 2 * 2 * 3 and paths[12].startswith("genome_sets_type3/pivot/ont/k_9/dataset_1/")
    text = S.intersection_percent_csv(paths, n)
    lines = text.splitlines()
    assert lines[0] == "read_type,pivot_num,k,dataset_num,intersection_percent" and len(lines) == 1 + 16
    want = []
    for rt in W3.READ_TYPES:                                                # read type, pivot, k, dataset
        for p in (1, 2):
            for k in ks:
                for num in (1, 2):
                    want.append(f"{rt},{p},{k},{num},{str(round(sum(inter[(rt, p, k, num)]) / totals[(rt, p, k)][0], 4))}")
    assert lines[1:] == want and lines[-1] == "ont,2,21,2,0.6667" and lines[1] == "illumina,1,9,1,0.3"

    bad = dict(totals)
    bad[("illumina", 1, "9")] = [10, 1, 0]                                  # a pivot set with a counter above 1
    csv_tree(tmp_path, monkeypatch, bad, inter)
    with pytest.raises(AssertionError, match="issue with pivot histogram file"):
        S.intersection_percent_csv(paths, n)
    bad_inter = dict(inter)
    bad_inter[("illumina", 1, "9", 2)] = [1, 1, 0, 0]                       # an intersect -ocsum counter of 1
    csv_tree(tmp_path, monkeypatch, totals, bad_inter)
    with pytest.raises(AssertionError, match="issue with histogram of intersection file"):
        S.intersection_percent_csv(paths, n)
    empty = dict(totals)
    empty[("ont", 1, "9")] = [0, 0, 0]                                      # a pivot without k-mers: as the reference, no guard
    csv_tree(tmp_path, monkeypatch, empty, inter)
    with pytest.raises(ZeroDivisionError):
        S.intersection_percent_csv(paths, n)


# ---------------------------------------------------------------- the stand-in read generator
def revcomp_text(t):
    return t[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def test_simulated_reads():
    codes = synth.genome_codes(2, 0, 5_000)
    genome = bytes(np.frombuffer(b"ACGTN", dtype=np.uint8)[codes])
    assert b"N" in genome
    rc = revcomp_text(genome)
    a = synth.simulated_reads(codes, 60, 150, 0.0, seed=5)
    assert a == synth.simulated_reads(codes, 60, 150, 0.0, seed=5)          # deterministic
    assert a != synth.simulated_reads(codes, 60, 150, 0.0, seed=6)
    assert len(a) == 60 and all(len(r) == 150 for r in a)
    fw = [r in genome for r in a]
    assert all(f or r in rc for f, r in zip(fw, a)) and 5 < sum(fw) < 55    # inside the genome, either strand
    b = synth.simulated_reads(codes, 60, 3_000, 0.0, seed=5, min_len=200)
    assert all(200 <= len(r) <= 3_000 and (r in genome or r in rc) for r in b) and len({len(r) for r in b}) > 20
    c = synth.simulated_reads(codes, 10, 9_000, 0.0, seed=1, min_len=200)   # never longer than the genome
    assert all(len(r) <= len(genome) and (r in genome or r in rc) for r in c)
    e = synth.simulated_reads(codes, 60, 150, 0.05, seed=5)                 # substitutions only: same places, same lengths
    assert [len(r) for r in e] == [len(r) for r in a]
    diff = sum(x != y for r, s in zip(a, e) for x, y in zip(r, s))
    assert 0.02 * 60 * 150 < diff < 0.08 * 60 * 150
    assert all((x == ord("N")) == (y == ord("N")) for r, s in zip(a, e) for x, y in zip(r, s))
    assert all(len(r) == 100 for r in synth.simulated_reads(codes[:100], 3, 150, 0.0, seed=1))


def test_write_type3_tree(tmp_path):
    root = str(tmp_path)
    synth.write_type3_tree(root, 2, 2, 3000, 25)
    for s in (1, 2):
        rest = sorted(os.listdir(os.path.join(root, f"input_type3/rest_of_set/dataset_{s}")))
        assert rest == [f"sp{s}_g0.fna.gz", f"sp{s}_g1.fna.gz"]
        pivot = O.read_fasta_bytes(os.path.join(root, f"input_type3/pivot/dataset_{s}/pivot_{s}.fna.gz"))
        assert all(O.read_fasta_bytes(os.path.join(root, f"input_type3/rest_of_set/dataset_{s}", f)) != pivot for f in rest)
        genome = "".join(O.fasta_records(pivot)).encode()
        for rt in W3.READ_TYPES:
            data = open(os.path.join(root, W3.reads_path(rt, s)), "rb").read()
            lines = data.split(b"\n")
            assert data.count(b">") == 25 and len(lines) == 51 and lines[-1] == b""    # a header and one line per read
            assert all(h.startswith(b">") and not r.startswith(b">") for h, r in zip(lines[0:50:2], lines[1:50:2]))
            lens = [len(r) for r in lines[1:50:2]]
            assert (set(lens) == {150}) if rt == "illumina" else (min(lens) >= 200 and len(set(lens)) > 5)
            assert max(lens) <= len(genome)
