"""The front end of the super-k-mer form — the shared base decode (kh_device.h: decode4), the m-mer hashes and the
sliding minimum of k_skm_scatter (kh_skm.hip, kh_skm_device.h) — against the C restatement.

Decode: every byte value, between valid stretches, at each of the 16 offsets of a code word, stretches in both letter
cases, and texts of every length modulo 16; at k = 31 (super-k-mer form) and k = 15 (key arrays).
Hashing and minimum: k = 17 .. 32 (every window width, every m), the same piece of sequence at every alignment of its
first base to the code words, with poly-A, poly-T and (ACGT)n stretches: ties between the strands and m-mers that are
their own reverse complement.  The number of records the scatter writes is a function of the input and of the
minimizer order alone: it must stay what it was."""
import numpy as np
import pytest

from khoice_amd import synth
from oracle import c_oracle as CO
from tests import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from khoice_amd import build as kbuild
    from khoice_amd import engine as E
    kbuild.build_library()
    e = E.Engine(0)
    yield e
    e.close()


def exp1_records(eng, seqs, group_of, k):
    """(result, records the scatter wrote, launches of the super-k-mer union)"""
    got, did = util.exp1_run_stats(eng, seqs, group_of, k, 5000, 64, ("skm_union",), ("skm_records",))
    return got, did["skm_records"], did["skm_union"]


# ---------------------------------------------------------------- decode
def decode_case():
    """[text of all byte values, 15 short texts of length 16 n + 1 .. 16 n + 15], groups.  The oracle takes every byte
    value in a cleaned text (anything outside ACGTacgt ends a k-mer), so all 256 are used; CO.exp1 runs on it in the
    test itself."""
    rng = np.random.default_rng(2031)
    out = bytearray()
    i = 0
    for v in range(256):
        for o in range(16):
            n = 33 + (o - (len(out) + 33)) % 16            # k + 2 bases or more, then the byte at offset o of its word
            stretch = util.random_dna_np(rng, n)
            out += stretch.lower() if i & 1 else stretch
            assert len(out) % 16 == o
            out.append(v)
            i += 1
    out += util.random_dna_np(rng, 40)
    shorts = [util.random_dna_np(rng, 80 + r) for r in range(1, 16)]
    seqs = [bytes(out)] + shorts
    return seqs, [0] + [1 + (j & 1) for j in range(len(shorts))]


@pytest.mark.parametrize("k", [31, 15])
def test_decode_every_byte_every_offset(eng, k):
    seqs, group_of = decode_case()
    assert set(seqs[0]) == set(range(256)) and {len(s) % 16 for s in seqs[1:]} == set(range(1, 16))
    want = CO.exp1(seqs, group_of, k, cs=5000, hist_len=64)
    got, _, launches = exp1_records(eng, seqs, group_of, k)
    assert launches == (1 if k == 31 else 0)
    util.exp1_same(got, want)


# ---------------------------------------------------------------- hashing and sliding minimum
def frontend_case(k):
    """Four related genomes of 40 kbp and one piece of sequence (random bases around poly-A, poly-T and (ACGT)n
    stretches) sixteen times, behind 0 .. 15 other bases: every m-mer of the piece at every offset of a code word."""
    items = synth.species_set(2, 2, 40_000)
    seqs = [t for _, _, t in items]
    group_of = [s - 1 for s, _, _ in items]
    rng = np.random.default_rng(1700 + k)
    r = lambda n: util.random_dna_np(rng, n)
    piece = (r(300) + b"A" * 70 + r(150) + b"T" * 70 + r(150) + b"ACGT" * 24 + r(200) + b"A" * 40 + b"T" * 40 + r(100) +
             b"TGCA" * 12 + r(300) + b"AT" * 30 + r(100) + b"CG" * 30 + r(300))
    for a in range(16):
        seqs.append(r(a) + piece)
        group_of.append(a & 1)
    return seqs, group_of


# skm_records of frontend_case(k) as the library gave them BEFORE the hashes were computed by funnel shifts and the
# minimum by three-input steps (taken from a run of the parent commit's library on these inputs)
PARENT_RECORDS = {17: 59613, 18: 51968, 19: 46200, 20: 41826, 21: 38021, 22: 35149, 23: 32256, 24: 29989, 25: 30001, 26: 28003,
                  27: 26647, 28: 28307, 29: 26593, 30: 25117, 31: 25066, 32: 22635}


@pytest.mark.parametrize("k", list(range(17, 33)))
def test_hash_and_minimum_every_width_and_alignment(eng, k):
    seqs, group_of = frontend_case(k)
    want = CO.exp1(seqs, group_of, k, cs=5000, hist_len=64)
    got, recs, launches = exp1_records(eng, seqs, group_of, k)
    assert launches == 1, "the super-k-mer form did not run"
    util.exp1_same(got, want)
    assert recs == PARENT_RECORDS[k]
