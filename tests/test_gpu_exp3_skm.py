"""kh_exp3_run above the bitmaps through k_skm_cross (kh_skm_device.h; KHOICE_EXP3_SKM=1, k = 17 .. 63) against the
oracle of tests/test_gpu_exp3.py: the `intersect -ocsum` histograms of every pivot with every group and the distinct
counts, bit-exact; and from the statistics that the super-k-mer form alone did the work — scatter, regroup and one
k_skm_cross launch per pass (a second one when slots overflowed their region), no set operation, no union, no bitmap.

The inputs are those of tests/test_gpu_exp3.py where it has them; the planted case is rebuilt here from a seeded pool of
codes (the bitmap tests' edge codes enumerate the code space, which ends at k = 12).  The unmarked tests prove on the
CPU what the cases claim to hold."""
import functools
import math
import random
import re

import numpy as np
import pytest

from oracle import kmer_oracle as O
from tests import test_gpu_exp2_bmp as X2     # kmer_text, revcomp_code, is_canonical
from tests import test_gpu_exp3 as X3          # oracle, species, read_shaped_case, walk_case, the planted kinds
from tests.util import ARENA_ALIGNED, ARENA_UNALIGNED, Arena

SWITCH = "KHOICE_EXP3_SKM"
FIELDS = X3.FIELDS
COUNTERS = ("retries", "builds", "bases", "kmers", "distinct", "setops", "setop_in", "setop_out", "text_packed",
            "skm_records", "big_slots", "cross_multi_slots")
EVERY_K = tuple(range(17, 33)) + (33, 41, 63)
ROUND = {1: 4096 - 4096 // 4, 2: 2048 - 2048 // 4}     # instances k_skm_cross takes in one round: one-word, two-word keys
MAX_OPS = 64


@pytest.fixture(scope="module")
def eng():
    from khoice_amd import build as kbuild
    from khoice_amd import engine as E
    kbuild.build_library()
    e = E.Engine(0)
    yield e
    e.close()


@pytest.fixture
def cross_on(monkeypatch):
    monkeypatch.setenv(SWITCH, "1")
    return monkeypatch


def deltas(st0, st1):
    """Launches of every kernel class and the growth of the counters; `skm_cross` is a class of this form only."""
    d = {n: st1["kernels"][n]["launches"] - st0["kernels"][n]["launches"] for n in st1["kernels"]}
    assert "skm_cross" in d, sorted(d)
    for n in COUNTERS + ("poisoned_bytes",):
        d[n] = st1[n] - st0[n]
    return d


def run(eng, seqs, group_of, pivots, k, cs=5000, hist_len=5001, want=None, texts=None):
    eng.profile(True)
    st0 = eng.stats()
    a, b = texts if texts else (seqs, pivots)
    got = eng.exp3_run(a, group_of, b, k, cs=cs, hist_len=hist_len)
    st1 = eng.stats()
    eng.profile(False)
    if want is None:
        want = X3.oracle(seqs, group_of, pivots, k, cs, hist_len)
    for f in FIELDS:
        assert got[f].shape == want[f].shape, (f, k, cs, hist_len)
        assert (got[f] == want[f]).all(), (f, k, cs, hist_len, np.argwhere(got[f] != want[f])[:8].tolist())
    return got, deltas(st0, st1)


def check(eng, seqs, group_of, pivots, k, launches=1, **kw):
    """The oracle's answers, and the super-k-mer form alone did the work, in `launches` launches of k_skm_cross."""
    got, d = run(eng, seqs, group_of, pivots, k, **kw)
    assert d["skm_cross"] == launches >= 1, d
    assert d["skm_scatter"] >= 1 and d["skm_regroup"] >= 1, d
    assert d["skm_union"] == 0 and d["skm_big"] == 0 and d["setop"] == 0 and d["union_tagged"] == 0 and d["retries"] == 0, d
    assert all(v == 0 for n, v in d.items() if n.startswith("bmp_")), d
    assert d["builds"] == len(seqs) + len(pivots), d
    return got, d


def by_sets(eng, seqs, group_of, pivots, k, retries=0, **kw):
    got, d = run(eng, seqs, group_of, pivots, k, **kw)
    assert d["setop"] > 0 and d["retries"] == retries, d
    assert all(v == 0 for n, v in d.items() if n.startswith("bmp_")), d
    return got, d


def same(a, b):
    return all(a[f].shape == b[f].shape and (a[f] == b[f]).all() for f in FIELDS)


def small_species():
    return X3.species(8_000)                  # 9 genomes in 3 groups, 6 read sets


@functools.lru_cache(maxsize=None)
def species_answer(k, cs=5000, hist_len=5001):
    """Computed once per (k, cs, hist_len) and shared by the tests; nobody writes to it."""
    return X3.oracle(*small_species(), k, cs, hist_len)


# ---------------------------------------------------------------- 1. every k
def every_k(eng, k):
    seqs, group_of, pivots = small_species()
    want = species_answer(k)
    got1, d1 = check(eng, seqs, group_of, pivots, k, want=want)
    got2, d2 = check(eng, seqs, group_of, pivots, k, want=want)
    unpoisoned = lambda d: {n: v for n, v in d.items() if n != "poisoned_bytes"}   # (a recycled block may be larger than asked for)
    assert same(got1, got2) and unpoisoned(d1) == unpoisoned(d2), (d1, d2)
    assert d1["bases"] == sum(len(s) for s in seqs + pivots)
    assert d1["distinct"] == int(want["distinct_per_seq"].sum() + want["distinct_per_pivot"].sum())
    return d1


@pytest.mark.gpu
@pytest.mark.parametrize("k", EVERY_K)
def test_exp3_skm_every_k(eng, cross_on, k):
    every_k(eng, k)


@pytest.mark.gpu
@pytest.mark.parametrize("k", (21, 41))
def test_exp3_skm_several_slots_per_workgroup(eng, cross_on, k):
    """Slots of 64 positions: some three thousand of them, several to every persistent workgroup."""
    seqs, group_of, pivots = small_species()
    cross_on.setenv("KHOICE_SKM_MEAN", "64")
    assert sum(len(s) for s in seqs + pivots) // 64 > 4 * 512
    check(eng, seqs, group_of, pivots, k, want=species_answer(k))


MAX_SLOTS = {1: 512 * 512, 2: 512 * 1024}      # coarse buckets x slots per bucket the records number


@functools.lru_cache(maxsize=None)
def many_slots_case():
    """2 groups x 2 genomes x 4.3 Mbp and two read sets: at 64 positions per slot more slots than one-word records
    number, so the plan keeps the 512 x 512 and fills them fuller.  Too large for the Python oracle: the set form is
    the reference."""
    rng = np.random.default_rng(77)
    fam = [X2.related(rng, 3, 4_300_000) for _ in range(2)]
    pivots = []
    for f in fam:
        codes = np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), np.frombuffer(f[2][:50_000], dtype=np.uint8)).astype(np.uint8)
        pivots.append(X3.read_text(codes, 200, 150, 0.01, 5))
    return [t for f in fam for t in f[:2]], [0, 0, 1, 1], pivots


@pytest.mark.gpu
def test_exp3_skm_more_slots_than_numbered(eng, monkeypatch):
    seqs, group_of, pivots = many_slots_case()
    assert sum(len(t) - 20 for t in seqs + pivots) // 64 > MAX_SLOTS[1]
    monkeypatch.delenv(SWITCH, raising=False)
    want = eng.exp3_run(seqs, group_of, pivots, 21)
    assert want["distinct_per_pivot"].min() > 0 and want["inter_hist"].sum() > 0
    monkeypatch.setenv(SWITCH, "1")
    monkeypatch.setenv("KHOICE_SKM_MEAN", "64")
    check(eng, seqs, group_of, pivots, 21, want=want)


# ---------------------------------------------------------------- 2. read-shaped pivots
@pytest.mark.gpu
@pytest.mark.parametrize("k", (17, 21, 32, 33))
def test_exp3_skm_read_shaped_pivots(eng, cross_on, k):
    seqs, group_of, pivots, names = X3.read_shaped_case(k)
    got, _ = check(eng, seqs, group_of, pivots, k)
    assert got["distinct_per_pivot"][names.index("empty")] == 0 and got["distinct_per_pivot"][names.index("shorter_than_k")] == 0
    assert (got["inter_hist"][names.index("empty")] == 0).all()
    p = names.index("a_genome")                                           # identical to a genome of group 1: every k-mer of it is met there
    assert got["inter_hist"][p, 1].sum() == got["distinct_per_pivot"][p] == got["distinct_per_seq"][2] > 0


# ---------------------------------------------------------------- 3. planted k-mers
PLANT_K = (21, 32)
PLANT_SIZES, PLANT_PIVOT_SETS, PLANT_VECTORS = X3.PLANT_SIZES, X3.PLANT_PIVOT_SETS, X3.PLANT_VECTORS
PLANT_ROUNDS = 4                 # plants per kind: both spellings of the genomes' copies, twice


def plant_kinds():
    return [(ps, vec) for ps in PLANT_PIVOT_SETS for vec in PLANT_VECTORS if ps or any(vec)]


@functools.lru_cache(maxsize=None)
def planted_case(k):
    """X3.planted_case with codes from a seeded pool: every code a record of its own; a plant is (code, pivots, vector,
    genomes, rc, what): held by the pivots of the set and by vector[g] genomes of group g, which spell its reverse
    complement when rc.  Every kind gets PLANT_ROUNDS plants, rc alternating.  k = 32 (even): every kind gets one more
    plant whose code is its own reverse complement.  Returns seqs, group_of, pivots, plants."""
    ng = len(PLANT_SIZES)
    group_of = [g for g, n in enumerate(PLANT_SIZES) for _ in range(n)]
    first = [group_of.index(g) for g in range(ng)]
    rng = random.Random(2300 + k)
    used = set()

    def fresh():
        while True:
            c = rng.randrange(4 ** k)
            if X2.is_canonical(c, k) and c != X2.revcomp_code(c, k) and c not in used:
                used.add(c)
                return c

    def palindrome():
        while True:
            h = rng.randrange(4 ** (k // 2))
            c = (h << k) | X2.revcomp_code(h, k // 2)
            if c not in used:
                assert c == X2.revcomp_code(c, k)
                used.add(c)
                return c

    plants = []
    i = 0
    for r in range(PLANT_ROUNDS + (1 if k % 2 == 0 else 0)):
        for ps, vec in plant_kinds():
            i += 1
            own = r == PLANT_ROUNDS
            code = palindrome() if own else fresh()
            genomes = tuple(first[g] + (i + j) % PLANT_SIZES[g] for g in range(ng) for j in range(vec[g]))
            plants.append((code, ps, vec, genomes, (not own) and r % 2 == 1, "own_revcomp" if own else "fill"))
    rng.shuffle(plants)
    texts = [[] for _ in group_of]
    ptexts = [[] for _ in range(4)]
    for code, ps, vec, genomes, rc, _ in plants:
        for p in ps:
            ptexts[p].append(X2.kmer_text(code, k))
        for gi in genomes:
            texts[gi].append(X2.kmer_text(X2.revcomp_code(code, k) if rc else code, k))
    return ["N".join(t).encode() for t in texts], group_of, ["\n".join(t).encode() for t in ptexts], plants


def planted_answer(k, cs=5000, hist_len=5001):
    """The expected outputs worked out from the plants alone; occ[p][g][v], v = 0 .. size."""
    seqs, group_of, pivots, plants = planted_case(k)
    ng = len(PLANT_SIZES)
    occ = [[[0] * (n + 1) for n in PLANT_SIZES] for _ in pivots]
    dseq, dpiv = [0] * len(seqs), [0] * len(pivots)
    for code, ps, vec, genomes, rc, _ in plants:
        for gi in genomes:
            dseq[gi] += 1
        for p in ps:
            dpiv[p] += 1
            for g in range(ng):
                occ[p][g][vec[g]] += 1
    want = {"inter_hist": np.zeros((len(pivots), ng, hist_len), dtype=np.uint64),
            "distinct_per_seq": np.array(dseq, dtype=np.uint64), "distinct_per_pivot": np.array(dpiv, dtype=np.uint64)}
    for p in range(len(pivots)):
        for g in range(ng):
            for v in range(1, PLANT_SIZES[g] + 1):
                want["inter_hist"][p, g, min(1 + min(v, cs), cs, hist_len - 1)] += occ[p][g][v]
    return want, occ


@pytest.mark.parametrize("k", PLANT_K)
def test_planted_case_holds_every_count(k):
    seqs, group_of, pivots, plants = planted_case(k)
    want, occ = planted_answer(k)
    assert all(occ[p][g][v] > 0 for p in range(len(pivots)) for g, n in enumerate(PLANT_SIZES) for v in range(n + 1))
    for kind in plant_kinds():                                            # every kind in both spellings
        assert {rc for _, ps, vec, _, rc, what in plants if (ps, vec) == kind and what == "fill"} == {False, True}, kind
        if k % 2 == 0:
            assert any((ps, vec) == kind and what == "own_revcomp" for _, ps, vec, _, _, what in plants), kind
    assert len({code for code, *_ in plants}) == len(plants)
    have = X3.oracle(seqs, group_of, pivots, k)                           # and the oracle's sets say the same
    assert all((have[f] == want[f]).all() for f in FIELDS)


@pytest.mark.gpu
@pytest.mark.parametrize("k", PLANT_K)
def test_exp3_skm_planted(eng, cross_on, k):
    seqs, group_of, pivots, _ = planted_case(k)
    want, _ = planted_answer(k)
    cross_on.setenv("KHOICE_SKM_MEAN", "64")                              # many small slots, some of them empty
    check(eng, seqs, group_of, pivots, k, want=want)


# ---------------------------------------------------------------- 4. the 64-operand edge, both mask halves
WALK = [(6, 21, 1), (7, 21, 2), (15, 21, 3), (6, 33, 1), (7, 41, 2)]      # pivots, k, passes


def passes(nseq, npiv):
    batch = min(npiv, MAX_OPS - nseq)
    return [min(batch, npiv - p0) for p0 in range(0, npiv, batch)]


def large_group_counts(hist):
    """Counts that only the groups of 17 and 33 can give (test_exp3_walk_edges): v >= 1 of group 3, v >= 17 of group 4."""
    return hist[:, 3, 2:19].sum() > 0 and hist[:, 4, 18:35].sum() > 0


@functools.lru_cache(maxsize=None)
def walk_answer(npiv, k):
    return X3.oracle(*X3.walk_case(npiv), k)


@functools.lru_cache(maxsize=None)
def declined_case():
    """64 genomes (the 58 of the walk case and a sixth group of six) and one pivot: no room for a pivot's bit."""
    seqs, group_of, pivots = X3.walk_case(6)
    return seqs + [bytes(p.replace(b"\n", b"N")) for p in pivots], group_of + [5] * 6, pivots[:1]


@pytest.mark.parametrize("npiv,k,n", WALK)
def test_walk_cases_have_the_operands_claimed(npiv, k, n):
    seqs, group_of, pivots = X3.walk_case(npiv)
    assert len(seqs) == 58 and len(pivots) == npiv
    assert passes(58, npiv) == {6: [6], 7: [6, 1], 15: [6, 6, 3]}[npiv] and len(passes(58, npiv)) == n
    assert 58 + passes(58, npiv)[0] == MAX_OPS
    first = group_of.index(4)
    assert group_of.count(4) == 33 and first < 32 < first + 33           # the group of 33 spans operand 32: both mask halves
    assert large_group_counts(walk_answer(npiv, k)["inter_hist"])
    seqs, group_of, pivots = declined_case()
    assert len(seqs) == MAX_OPS and len(pivots) == 1 and max(group_of) == 5


@pytest.mark.gpu
@pytest.mark.parametrize("npiv,k,n", WALK)
def test_exp3_skm_operand_edge(eng, cross_on, npiv, k, n):
    seqs, group_of, pivots = X3.walk_case(npiv)
    got, _ = check(eng, seqs, group_of, pivots, k, launches=n, want=walk_answer(npiv, k))
    assert large_group_counts(got["inter_hist"])


@pytest.mark.gpu
def test_exp3_skm_declines_64_genomes(eng, cross_on):
    seqs, group_of, pivots = declined_case()
    _, d = by_sets(eng, seqs, group_of, pivots, 21)
    assert d["skm_cross"] == 0 and d["skm_scatter"] == 0, d


# ---------------------------------------------------------------- 5. rounds
# (k, KHOICE_SKM_MEAN, KHOICE_SKM_M).  The plan lowers a mean whose records would not fit a slot's region: at k = 21
# with its minimizer of 12 bases 4000 becomes 2648, below a round — with a minimizer of 8 (records of up to 14 windows)
# 3460 stay; at k = 31 3808.
ROUNDS = [(31, 4000, None), (21, 4000, 8)]


def minimizer_len(k):
    """skm_minimizer_len of kh_engine.cpp, one-word keys."""
    if k <= 24:
        return 12 if k >= 17 else 11
    if k <= 27:
        return 13
    w15 = k - 15 + 1
    return 16 if w15 > 1 and (w15 - 1) & (w15 - 2) == 0 else 15


def planned_mean(k, mean, m, fan, max_cap2=1024):
    """skm_plan's rule restated: the mean is lowered until mean x records per k-mer x slack + 112 fits a region."""
    w = k - (m or minimizer_len(k)) + 1
    per_kmer = 2.0 / (w + 1) + 1.0 / 48.0
    clump = 0.5 * (w + 1) * fan
    mean = max(64, mean)
    for _ in range(8):
        slack = max(1.7, 1.0 + 5.0 * math.sqrt(clump / mean))
        c2 = mean * per_kmer * slack + 96 + 16
        if c2 <= max_cap2 or mean <= 256:
            break
        mean = max(256, int(mean * max_cap2 / c2 * 0.98))
    return mean


def instances_per_slot(k, mean, m):
    seqs, group_of, pivots = small_species()
    fan = max(group_of.count(g) for g in set(group_of)) + 1               # the hint of exp3_skm: the largest group + 1
    positions = sum(max(0, len(t) - k + 1) for t in seqs + pivots)
    nslots = -(-positions // planned_mean(k, mean, m, fan))
    # instances: the oracle's counters of every text added up (saturation far above any count here)
    inst = sum(sum(O.build(b"".join(b">r\n" + r + b"\n" for r in t.split(b"\n")), k, cs=1 << 30).values()) for t in seqs + pivots)
    assert inst == sum(max(0, len(r) - k + 1) for t in seqs + pivots for r in re.split(b"[^ACGTacgt]+", t))   # = positions inside runs of bases
    print(k, mean, m, "positions", positions, "nslots", nslots, "instances", inst)
    return inst / nslots


@pytest.mark.parametrize("k,mean,m", ROUNDS)
def test_rounds_case_fills_more_than_a_round(k, mean, m):
    assert instances_per_slot(k, mean, m) > ROUND[1], instances_per_slot(k, mean, m)
    assert planned_mean(21, 4000, None, 4) < ROUND[1]                     # why k = 21 needs the shorter minimizer


@pytest.mark.gpu
@pytest.mark.parametrize("k,mean,m", ROUNDS)
def test_exp3_skm_rounds(eng, cross_on, k, mean, m):
    seqs, group_of, pivots = small_species()
    cross_on.setenv("KHOICE_SKM_MEAN", str(mean))
    if m:
        cross_on.setenv("KHOICE_SKM_M", str(m))
    got, d = run(eng, seqs, group_of, pivots, k, want=species_answer(k))
    assert d["cross_multi_slots"] > 0 and d["skm_cross"] >= 1 and d["retries"] == 0 and d["setop"] == 0, d


# ---------------------------------------------------------------- 6. side list
# Regions of `slack` x the mean record count + 96: at k = 21 a slot has some 500 records and 0.3 cuts its region below
# them; at k = 41 the plan's slots have some 100 records, fewer than the constant alone holds: larger slots (the plan
# lowers 2400 to about 1900 instances, 175 records) and a tenth.
SIDE_LIST = {21: {"KHOICE_SKM_SLACK": "0.3"}, 41: {"KHOICE_SKM_SLACK": "0.1", "KHOICE_SKM_MEAN": "2400"}}


def side_list(eng, monkeypatch, k):
    for name, value in SIDE_LIST[k].items():
        monkeypatch.setenv(name, value)
    seqs, group_of, pivots = small_species()
    got, d = check(eng, seqs, group_of, pivots, k, launches=2, want=species_answer(k))
    assert d["big_slots"] > 0, d
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("k", (21, 41))
def test_exp3_skm_side_list(eng, cross_on, k):
    side_list(eng, cross_on, k)


@functools.lru_cache(maxsize=None)
def coarse_overflow_case():
    """A seventh pivot of one tandem repeat: 120 000 positions with one minimizer, some 3 900 records for one coarse
    bucket, whose region holds 2 048 and a hundredth of the mean."""
    seqs, group_of, pivots = small_species()
    return seqs, group_of, pivots + [b"AC" * 60_000]


@pytest.mark.gpu
def test_exp3_skm_coarse_overflow_falls_back(eng, cross_on):
    seqs, group_of, pivots = coarse_overflow_case()
    want = X3.oracle(seqs, group_of, pivots, 21)
    cross_on.setenv("KHOICE_SKM_SLACK", "0.01")
    got, d = by_sets(eng, seqs, group_of, pivots, 21, retries=1, want=want)
    assert d["skm_scatter"] == 1 and d["builds"] == len(seqs) + len(pivots), d
    cross_on.delenv(SWITCH)
    sets, d = by_sets(eng, seqs, group_of, pivots, 21, want=want)
    assert same(got, sets) and d["skm_scatter"] == 0, d


@functools.lru_cache(maxsize=None)
def coarse_overflow_case_two_words():
    """The same with two-word keys (k = 41): a record holds at most 63 k-mers, so a tandem repeat of 200 000 positions
    makes at least 3 174 records for one coarse bucket, whose region holds 2 048 and a hundredth of the mean."""
    seqs, group_of, pivots = small_species()
    return seqs, group_of, pivots + [b"AC" * 100_000]


@pytest.mark.gpu
def test_exp3_skm_coarse_overflow_falls_back_two_word_keys(eng, cross_on):
    seqs, group_of, pivots = coarse_overflow_case_two_words()
    want = X3.oracle(seqs, group_of, pivots, 41)
    cross_on.setenv("KHOICE_SKM_SLACK", "0.01")
    got, d = by_sets(eng, seqs, group_of, pivots, 41, retries=1, want=want)
    assert d["skm_scatter"] == 1 and d["builds"] == len(seqs) + len(pivots), d


# ---------------------------------------------------------------- 7. clamps
@pytest.mark.gpu
@pytest.mark.parametrize("cs", (1, 2, 5000))
@pytest.mark.parametrize("hist_len", (2, 3, 5001))
def test_exp3_skm_clamps(eng, cross_on, cs, hist_len):
    seqs, group_of, pivots = small_species()
    check(eng, seqs, group_of, pivots, 21, cs=cs, hist_len=hist_len, want=species_answer(21, cs, hist_len))


# ---------------------------------------------------------------- 8. the switch
@pytest.mark.gpu
def test_exp3_skm_switch(eng, monkeypatch):
    seqs, group_of, pivots = small_species()
    monkeypatch.delenv(SWITCH, raising=False)
    sets, d = by_sets(eng, seqs, group_of, pivots, 21, want=species_answer(21))
    assert d["skm_cross"] == 0 and d["skm_scatter"] == 0, d
    for value in ("0", "", "2"):                                          # only "1" takes the form
        monkeypatch.setenv(SWITCH, value)
        _, d = by_sets(eng, seqs, group_of, pivots, 21, want=species_answer(21))
        assert d["skm_cross"] == 0, (value, d)
    monkeypatch.setenv(SWITCH, "1")
    got, _ = check(eng, seqs, group_of, pivots, 21, want=species_answer(21))
    assert same(got, sets)
    monkeypatch.setenv("KHOICE_NO_SKM", "1")
    _, d = by_sets(eng, seqs, group_of, pivots, 21, want=species_answer(21))
    assert d["skm_cross"] == 0 and d["skm_scatter"] == 0, d
    monkeypatch.delenv("KHOICE_NO_SKM")
    monkeypatch.setenv("KHOICE_NO_SKM2", "1")                             # two-word keys only
    _, d = by_sets(eng, seqs, group_of, pivots, 41, want=species_answer(41))
    assert d["skm_cross"] == 0, d
    check(eng, seqs, group_of, pivots, 21, want=species_answer(21))
    none, d = run(eng, seqs, group_of, [], 21)                            # no pivot: the set form builds the genomes only
    assert d["skm_cross"] == 0 and d["retries"] == 0 and d["builds"] == len(seqs) and none["inter_hist"].shape == (0, 3, 5001), d


# ---------------------------------------------------------------- 9. device-resident texts
@pytest.mark.gpu
@pytest.mark.parametrize("k", (21, 41))
def test_exp3_skm_device_texts(eng, cross_on, k):
    seqs, group_of, pivots = small_species()
    texts = seqs + pivots
    total = sum(len(t) for t in texts)
    host, hd = check(eng, seqs, group_of, pivots, k, want=species_answer(k))
    assert hd["text_packed"] == total, hd
    mixes = {"aligned": [ARENA_ALIGNED[i % 2] for i in range(len(texts))],
             "unaligned": [ARENA_UNALIGNED[i % 3] for i in range(len(texts))],
             "mixed": [(ARENA_ALIGNED + ARENA_UNALIGNED)[i % 5] for i in range(len(texts))]}
    for name, classes in mixes.items():
        arena = Arena(texts, classes, [None] * len(texts), 900 + k)
        dev = arena.upload()
        got, d = check(eng, seqs, group_of, pivots, k, want=species_answer(k), texts=(dev[:len(seqs)], dev[len(seqs):]))
        assert same(got, host), name
        assert d["text_packed"] == sum(len(t) for t, c in zip(texts, classes) if c % 16), (name, d)   # read in place or packed
        assert {n: v for n, v in d.items() if n != "text_packed"} == {n: v for n, v in hd.items() if n != "text_packed"}, (name, d, hd)
        assert (arena.download() == arena.host).all(), name               # and the texts are as they were


# ---------------------------------------------------------------- 10. poisoned pool
PATTERNS = (0, 65, 99, 255)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", PATTERNS, ids=lambda p: f"p{p:02X}")
@pytest.mark.parametrize("k", (21, 41))
def test_exp3_skm_every_k_poisoned(eng, cross_on, k, pattern):
    cross_on.setenv("KHOICE_DEBUG_POISON", str(pattern))
    assert every_k(eng, k)["poisoned_bytes"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", PATTERNS, ids=lambda p: f"p{p:02X}")
@pytest.mark.parametrize("k", (21, 41))
def test_exp3_skm_side_list_poisoned(eng, cross_on, k, pattern):
    cross_on.setenv("KHOICE_DEBUG_POISON", str(pattern))
    assert side_list(eng, cross_on, k)["poisoned_bytes"] > 0
