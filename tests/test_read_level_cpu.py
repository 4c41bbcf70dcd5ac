"""Read-level analysis (experiment type 6), the host side: the restatement of src/merge_lists.py:160-179 plus the
seeded draws of `read_level_outputs` against texts the reference wrote, the line rules of `read_level_reads`, and the
seed switch of `-r`.  No device compute here."""
import json
import os
import random

import numpy as np
import pytest

from khoice_amd import merge_lists as ML
from tests import read_level_oracle as RL

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "merge_lists_read_level.json")))["cases"]


def dump_kmers(text):
    return {line.split()[0] for line in text.splitlines()}


def case_ties(case):
    """Per pivot the tie masks the restatement gives from the case's dumps and reads files."""
    n, k = case["num_datasets"], case["k"]
    out = []
    for p in range(n):
        pivot = dump_kmers(case["pivot_dumps"][p])
        cols = [None] * n
        for j in range(n):
            cols[(p * n + j) % n] = dump_kmers(case["intersection_dumps"][p * n + j]) & pivot
        res = RL.reads_votes(RL.file_reads(case["reads_files"][p]), k, cols, pivot)
        out.append(RL.tie_masks(res, n))
    return out


@pytest.mark.parametrize("case", GOLDEN, ids=lambda c: f"n{c['num_datasets']}_k{c['k']}")
def test_restatement_and_seeded_draws_give_the_references_files(case):
    ties = case_ties(case)
    assert any(bin(int(m[0])).count("1") > 1 for t in ties for m in t)        # there is something to draw
    random.seed(case["seed"])
    files = ML.read_level_outputs(ties, case["num_datasets"], str(case["k"]))
    assert files == case["outputs"]
    random.seed(case["seed"] + 1)                                             # and the seed matters
    assert ML.read_level_outputs(ties, case["num_datasets"], str(case["k"])) != case["outputs"]


def test_golden_cases_are_the_issues():
    assert {(c["num_datasets"], c["k"]) for c in GOLDEN} >= {(2, 5), (3, 11), (4, 21), (3, 33), (5, 7)}
    for c in GOLDEN:
        assert all("\n\n" in f for f in c["reads_files"])                     # a blank line per file
        assert any(not f.endswith("\n") for f in c["reads_files"])            # a file without its final newline


def reads_of(tmp_path, data: bytes):
    p = tmp_path / "pivot.fa"
    p.write_bytes(data)
    text, off = ML.read_level_reads(str(p))
    assert text.dtype == np.uint8 and off.dtype == np.uint64 and off[0] == 0 and off[-1] == text.size
    raw = text.tobytes()
    assert all(raw[int(off[i + 1]) - 1:int(off[i + 1])] == b"\n" for i in range(off.size - 1))
    return [raw[int(off[i]):int(off[i + 1]) - 1].decode() for i in range(off.size - 1)]


@pytest.mark.parametrize("name,data,want", [
    ("plain", b">r1\nACGT\n>r2\nGG\n", ["ACGT", "GG"]),
    ("crlf", b">r1\r\nACGT\r\n>r2\r\nGG\r\n", ["ACGT", "GG"]),
    ("blanks", b">r1\n  ACGT \t\n\tGG\n \n", ["ACGT", "GG", ""]),
    ("blank_lines", b"\n>r1\n\nAC\n\n", ["", "", "AC", ""]),
    ("gt_inside", b">r1\nAC>GT\nACGT\nA>\n", ["ACGT"]),
    ("no_final_newline", b">r1\nACGT\n>r2\nGG", ["ACGT", "GG"]),
    ("no_header", b"ACGT\nTT", ["ACGT", "TT"]),
    ("inner_blank_kept", b"AC GT\n", ["AC GT"]),
    ("empty", b"", []),
])
def test_read_level_reads_line_rules(tmp_path, name, data, want):
    assert reads_of(tmp_path, data) == want
    # the reference's own lines (:153-159) on the same file
    with open(tmp_path / "pivot.fa", "r") as fh:
        assert [line.strip() for line in fh.readlines() if ">" not in line] == want
    assert RL.file_reads(data.decode()) == want


def lists(tmp_path, with_dump=True):
    dump = tmp_path / "pivot_1.txt"
    dump.write_text("AAAAA\t1\n")
    pl, il = tmp_path / "p.txt", tmp_path / "i.txt"
    pl.write_text(str(dump) + "\n")
    il.write_text(str(dump) + "\n")
    reads = tmp_path / "reads"
    reads.mkdir()
    return ["-n", "1", "-p", str(pl), "-i", str(il), "-o", str(tmp_path) + "/", "-k", "5", "-r", str(reads) + "/"]


def test_seed_option_gets_past_the_refusal(tmp_path, capsys, monkeypatch):
    monkeypatch.delenv("KHOICE_READ_LEVEL_SEED", raising=False)
    rc = ML.main(lists(tmp_path) + ["--seed", "7"])
    err = capsys.readouterr().err
    assert rc == 1 and "pivot_1.fa" in err and "--seed" not in err            # stopped at the first missing reads file


def test_seed_from_the_environment_gets_past_the_refusal(tmp_path, capsys, monkeypatch):
    monkeypatch.setenv("KHOICE_READ_LEVEL_SEED", "7")
    rc = ML.main(lists(tmp_path))
    err = capsys.readouterr().err
    assert rc == 1 and "pivot_1.fa" in err and "--seed" not in err


def test_read_level_without_a_seed_is_still_refused(tmp_path, capsys, monkeypatch):
    monkeypatch.delenv("KHOICE_READ_LEVEL_SEED", raising=False)
    rc = ML.main(lists(tmp_path))
    err = capsys.readouterr().err
    assert rc == 1 and "read-level" in err and "--seed" in err and "pivot_1.fa" not in err


def test_seed_option_wins_over_the_environment(monkeypatch):
    monkeypatch.setenv("KHOICE_READ_LEVEL_SEED", "7")
    assert ML.read_level_seed(ML.parse_arguments(["-n", "1", "-p", "a", "-i", "b", "-o", "c", "-k", "5", "--seed", "9"])) == 9
    assert ML.read_level_seed(ML.parse_arguments(["-n", "1", "-p", "a", "-i", "b", "-o", "c", "-k", "5"])) == 7


def test_outputs_keep_int_cells_and_an_empty_last_column():
    masks = [np.array([[0b01], [0b10], [0b11], [0b11]], dtype=np.uint64), np.array([[0b10]], dtype=np.uint64)]
    random.seed(3)
    files = ML.read_level_outputs(masks, 2, "9")
    rows = [r.split(",") for r in files["confusion_matrix/k_9_confusion_matrix.txt"].splitlines()]
    assert files["confusion_matrix/k_9_confusion_matrix.txt"] == files["confusion_matrix/k_9_confusion_matrix_with_unidentified.txt"]
    assert all("." not in c for r in rows for c in r) and [r[2] for r in rows] == ["0", "0"]
    assert sum(int(c) for c in rows[0]) == 4 and rows[1] == ["0", "1", "0"]
