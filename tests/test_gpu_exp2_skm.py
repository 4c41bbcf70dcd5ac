"""kh_exp2_run above the bitmaps through k_skm_cross with the own-group read-out (kh_skm_device.h; KHOICE_EXP2_SKM=1, k = 17 .. 63) against the
oracle of tests/test_gpu_exp2_bmp.py: for every pivot the `intersect -ocsum` histograms and `kmers_subtract` counts
against its own group and against the other groups, and the distinct counts, bit-exact; and from the statistics that the
super-k-mer form alone did the work — scatter, regroup and one launch of the slot walk per pass (a second one when
slots overflowed their region), no set operation, no union, no bitmap.

With the switch set on a library without the form the set form answers, so every `check` fails there.  The unmarked
tests prove on the CPU what the cases claim to hold."""
import functools
import re

import numpy as np
import pytest

from oracle import kmer_oracle as O
from tests import test_gpu_exp2_bmp as X2     # oracle, species, shape_case, related
from tests import test_gpu_exp3_skm as S3      # planted_case, deltas, the environment settings of rounds and side list
from tests.util import ARENA_ALIGNED, ARENA_UNALIGNED, Arena

SWITCH = "KHOICE_EXP2_SKM"
FIELDS = X2.FIELDS
EVERY_K = tuple(range(17, 33)) + (33, 41, 63)
MAX_OPS, MAX_BINS = 64, 1024                   # operands and bins of one pass


@pytest.fixture(scope="module")
def eng():
    from khoice_amd import build as kbuild
    from khoice_amd import engine as E
    kbuild.build_library()
    e = E.Engine(0)
    yield e
    e.close()


@pytest.fixture
def pivot_on(monkeypatch):
    monkeypatch.setenv(SWITCH, "1")
    return monkeypatch


def run(eng, seqs, group_of, pivots, pivot_group, k, cs=5000, hist_len=5001, want=None, texts=None):
    eng.profile(True)
    st0 = eng.stats()
    a, b = texts if texts else (seqs, pivots)
    got = eng.exp2_run(a, group_of, b, pivot_group, k, cs=cs, hist_len=hist_len)
    st1 = eng.stats()
    eng.profile(False)
    if want is None:
        want = X2.oracle(seqs, group_of, pivots, pivot_group, k, cs, hist_len)
    for f in FIELDS:
        assert got[f].shape == want[f].shape, (f, k, cs, hist_len)
        assert (got[f] == want[f]).all(), (f, k, cs, hist_len, np.argwhere(got[f] != want[f])[:8].tolist())
    return got, S3.deltas(st0, st1)


def check(eng, seqs, group_of, pivots, pivot_group, k, launches=1, **kw):
    """The oracle's answers; the super-k-mer form alone did the work, in `launches` launches of the slot walk; and every
    distinct k-mer of a pivot was counted once within and once across."""
    got, d = run(eng, seqs, group_of, pivots, pivot_group, k, **kw)
    assert d["skm_cross"] == launches >= 1, d
    assert d["skm_scatter"] >= 1 and d["skm_regroup"] >= 1, d
    assert d["skm_union"] == 0 and d["skm_big"] == 0 and d["setop"] == 0 and d["union_tagged"] == 0 and d["retries"] == 0, d
    assert all(v == 0 for n, v in d.items() if n.startswith("bmp_")), d
    assert d["builds"] == len(seqs) + len(pivots), d
    for p in range(len(pivots)):
        for scope in ("within", "across"):
            assert int(got[scope + "_hist"][p].sum() + got[scope + "_only"][p]) == int(got["distinct_per_pivot"][p]), (scope, p)
    return got, d


def by_sets(eng, seqs, group_of, pivots, pivot_group, k, retries=0, **kw):
    got, d = run(eng, seqs, group_of, pivots, pivot_group, k, **kw)
    assert d["setop"] > 0 and d["retries"] == retries, d
    assert all(v == 0 for n, v in d.items() if n.startswith("bmp_")), d
    return got, d


def same(a, b):
    return all(a[f].shape == b[f].shape and (a[f] == b[f]).all() for f in FIELDS)


def passes(group_of, pivot_group):
    """The pass rule: pivots in the caller's order while genomes + pivots <= 64 and the bins (per pivot the size of its
    group + 1 within, one per group across) <= 1024."""
    ng = max(group_of) + 1
    out, np_, bins = [], 0, 0
    for g in pivot_group:
        need = group_of.count(g) + 1 + ng
        if np_ and (len(group_of) + np_ + 1 > MAX_OPS or bins + need > MAX_BINS):
            out.append(np_)
            np_, bins = 0, 0
        np_ += 1
        bins += need
    return out + [np_] if np_ else out


def counts_seen(hist, only):
    """The counts v with a non-zero bin: 0 from the subtract count, v >= 1 from bin v + 1 of the -ocsum histogram."""
    return ({0} if only else set()) | {int(b) - 1 for b in np.flatnonzero(hist)}


def small_species():
    return X2.species(8_000)                   # 9 genomes in 3 groups, one pivot per group


@functools.lru_cache(maxsize=None)
def species_answer(k, cs=5000, hist_len=5001):
    """Computed once per (k, cs, hist_len) and shared by the tests; nobody writes to it."""
    return X2.oracle(*small_species(), k, cs, hist_len)


# ---------------------------------------------------------------- 1. every k
def every_k(eng, k):
    seqs, group_of, pivots, pivot_group = small_species()
    want = species_answer(k)
    got1, d1 = check(eng, seqs, group_of, pivots, pivot_group, k, want=want)
    got2, d2 = check(eng, seqs, group_of, pivots, pivot_group, k, want=want)
    unpoisoned = lambda d: {n: v for n, v in d.items() if n != "poisoned_bytes"}   # (a recycled block may be larger than asked for)
    assert same(got1, got2) and unpoisoned(d1) == unpoisoned(d2), (d1, d2)
    assert d1["bases"] == sum(len(s) for s in seqs + pivots)
    assert d1["distinct"] == int(want["distinct_per_seq"].sum() + want["distinct_per_pivot"].sum())
    assert d1["setop_out"] == int((want["distinct_per_pivot"] - want["within_only"]).sum())   # pivot k-mers their own group holds
    return d1


@pytest.mark.gpu
@pytest.mark.parametrize("k", EVERY_K)
def test_exp2_skm_every_k(eng, pivot_on, k):
    every_k(eng, k)


# ---------------------------------------------------------------- 2. planted k-mers
PLANT_K = S3.PLANT_K
PLANT_SIZES = S3.PLANT_SIZES
PLANT_PIVOT_GROUP = [0, 1, 2, 0]               # two pivots share group 0


def planted_answer(k, cs=5000, hist_len=5001):
    """The expected outputs worked out from the plants alone: a plant held by pivot p of group g and by vec[h] genomes of
    group h counts vec[g] within and the groups h != g with vec[h] > 0 across.  -> want, occ_w[p][v], occ_a[p][v]"""
    seqs, group_of, pivots, plants = S3.planted_case(k)
    ng = len(PLANT_SIZES)
    occ_w = [[0] * (PLANT_SIZES[g] + 1) for g in PLANT_PIVOT_GROUP]
    occ_a = [[0] * ng for _ in PLANT_PIVOT_GROUP]
    dseq, dpiv = [0] * len(seqs), [0] * len(pivots)
    for code, ps, vec, genomes, rc, _ in plants:
        for gi in genomes:
            dseq[gi] += 1
        for p in ps:
            g = PLANT_PIVOT_GROUP[p]
            dpiv[p] += 1
            occ_w[p][vec[g]] += 1
            occ_a[p][sum(1 for h in range(ng) if h != g and vec[h] > 0)] += 1
    npv = len(pivots)
    want = {"within_hist": np.zeros((npv, hist_len), dtype=np.uint64), "across_hist": np.zeros((npv, hist_len), dtype=np.uint64),
            "within_only": np.array([o[0] for o in occ_w], dtype=np.uint64),
            "across_only": np.array([o[0] for o in occ_a], dtype=np.uint64),
            "distinct_per_seq": np.array(dseq, dtype=np.uint64), "distinct_per_pivot": np.array(dpiv, dtype=np.uint64)}
    for p in range(npv):
        for occ, f in ((occ_w[p], "within_hist"), (occ_a[p], "across_hist")):
            for v in range(1, len(occ)):
                want[f][p, min(1 + min(v, cs), cs, hist_len - 1)] += occ[v]
    return want, occ_w, occ_a


@pytest.mark.parametrize("k", PLANT_K)
def test_planted_case_holds_every_count(k):
    seqs, group_of, pivots, plants = S3.planted_case(k)
    assert len(pivots) == len(PLANT_PIVOT_GROUP) and PLANT_PIVOT_GROUP.count(0) == 2
    want, occ_w, occ_a = planted_answer(k)
    assert all(v > 0 for occ in occ_w + occ_a for v in occ)               # every within bin 0 .. size, every across bin 0 .. 2
    if k == 21:
        assert occ_w == [[24, 24, 12, 12], [36, 36], [24, 24, 24], [24, 24, 12, 12]], occ_w
        assert occ_a == [[12, 36, 24], [12, 24, 36], [12, 36, 24], [12, 36, 24]], occ_a
    if k % 2 == 0:                                                        # the plants that are their own reverse complement
        assert any(what == "own_revcomp" and ps for _, ps, _, _, _, what in plants)
    have = X2.oracle(seqs, group_of, pivots, PLANT_PIVOT_GROUP, k)        # and the oracle's sets say the same
    assert all((have[f] == want[f]).all() for f in FIELDS)


@pytest.mark.gpu
@pytest.mark.parametrize("k", PLANT_K)
def test_exp2_skm_planted(eng, pivot_on, k):
    seqs, group_of, pivots, _ = S3.planted_case(k)
    want, _, _ = planted_answer(k)
    pivot_on.setenv("KHOICE_SKM_MEAN", "64")                              # many small slots, some of them empty
    got, _ = check(eng, seqs, group_of, pivots, PLANT_PIVOT_GROUP, k, want=want)
    for p, g in enumerate(PLANT_PIVOT_GROUP):
        assert counts_seen(got["within_hist"][p], got["within_only"][p]) == set(range(PLANT_SIZES[g] + 1))
        assert counts_seen(got["across_hist"][p], got["across_only"][p]) == set(range(len(PLANT_SIZES)))


# ---------------------------------------------------------------- 3. the 64-operand edge, both mask halves
EDGE_SIZES = (1, 3, 4, 17, 33)
EDGE = [(6, 21, 1), (7, 21, 2), (6, 41, 1), (7, 41, 2)]                   # pivots, k, passes


@functools.lru_cache(maxsize=None)
def edge_case(npiv):
    """58 genomes of ONE ancestor in groups of 1, 3, 4, 17 and 33, and the next npiv texts as pivots of groups 4, 3, 2,
    1, 0, 4, 3: every k-mer of a pivot is met in its own and in other groups."""
    fam = X2.related(np.random.default_rng(4242), 65, 1500)
    group_of = [g for g, n in enumerate(EDGE_SIZES) for _ in range(n)]
    return fam[:58], group_of, fam[58:58 + npiv], [(4 - p) % 5 for p in range(npiv)]


@functools.lru_cache(maxsize=None)
def edge_answer(npiv, k):
    return X2.oracle(*edge_case(npiv), k)


@pytest.mark.parametrize("npiv,k,n", EDGE)
def test_edge_cases_have_the_operands_claimed(npiv, k, n):
    seqs, group_of, pivots, pivot_group = edge_case(npiv)
    assert len(seqs) == 58 and len(pivots) == npiv
    assert passes(group_of, pivot_group) == {6: [6], 7: [6, 1]}[npiv] and len(passes(group_of, pivot_group)) == n
    assert 58 + passes(group_of, pivot_group)[0] == MAX_OPS               # the first pass fills the mask
    first = group_of.index(4)
    assert first == 25 and group_of.count(4) == 33 and first < 32 < first + 33   # the group of 33 spans operand 32: both mask halves
    want = edge_answer(npiv, k)
    assert (want["within_hist"].sum(axis=1) + want["within_only"] == want["distinct_per_pivot"]).all()
    if k == 21:
        own = [counts_seen(want["within_hist"][p], want["within_only"][p]) for p in (0, 5)]   # the pivots of the group of 33
        assert all(set(range(14, 27)) <= seen for seen in own) and set(range(13, 27)) <= own[0] | own[1], own   # counts that need both halves
        for p in range(6):
            seen = counts_seen(want["across_hist"][p], want["across_only"][p])
            assert seen >= ({1, 3, 4} if p == 3 else {1, 2, 3, 4}) and (2 in seen) == (p != 3), (p, sorted(seen))


@pytest.mark.gpu
@pytest.mark.parametrize("npiv,k,n", EDGE)
def test_exp2_skm_operand_edge(eng, pivot_on, npiv, k, n):
    check(eng, *edge_case(npiv), k, launches=n, want=edge_answer(npiv, k))


# ---------------------------------------------------------------- 4. the bins edge
@functools.lru_cache(maxsize=None)
def bins_case():
    """32 groups of one genome and a pivot of every group, all of one ancestor: 64 operands would fit one pass, the
    34 bins of a pivot (2 within, 32 across) let 30 of them in."""
    fam = X2.related(np.random.default_rng(4243), 64, 1500)
    return fam[:32], list(range(32)), fam[32:], list(range(32))


@functools.lru_cache(maxsize=None)
def bins_answer():
    return X2.oracle(*bins_case(), 21)


def test_bins_case_is_cut_by_the_bins():
    seqs, group_of, pivots, pivot_group = bins_case()
    assert len(seqs) + len(pivots) == MAX_OPS and 30 * 34 <= MAX_BINS < 31 * 34
    assert passes(group_of, pivot_group) == [30, 2]
    want = bins_answer()
    seen = set().union(*(counts_seen(want["across_hist"][p], want["across_only"][p]) for p in range(32)))
    assert set(range(10, 27)) <= seen and max(seen) < 32, sorted(seen)       # across counts far above a handful of groups


@pytest.mark.gpu
def test_exp2_skm_bins_edge(eng, pivot_on):
    check(eng, *bins_case(), 21, launches=2, want=bins_answer())


# ---------------------------------------------------------------- 5. shapes of the type-2 contract
@functools.lru_cache(maxsize=None)
def widths_case():
    """X2.shape_case("counter_widths") without its group of 70 (at most 63 genomes): groups of 1, 2 and 17; pivots: a
    further genome of group 0, a genome OF group 1, a further genome of group 2, one with a run of N, one shorter than k."""
    seqs, group_of, pivots, pivot_group = X2.shape_case("counter_widths")
    keep = [i for i, g in enumerate(group_of) if g < 3]
    return [seqs[i] for i in keep], [group_of[i] for i in keep], pivots[:4] + [pivots[5]], [0, 1, 2, 2, 0]


def shape(name):
    return widths_case() if name == "widths" else X2.shape_case(name)


def test_skm_shape_cases_are_what_they_claim():
    seqs, group_of, pivots, pivot_group = widths_case()
    assert [group_of.count(g) for g in range(3)] == [1, 2, 17] and len(seqs) < MAX_OPS
    assert pivots[1] in [s for s, g in zip(seqs, group_of) if g == 1] and len(pivots[4]) < 17 and b"N" * 40 in pivots[3]
    seqs, group_of, pivots, pivot_group = X2.shape_case("two_and_none")
    assert pivot_group.count(2) == 2 and pivot_group.count(1) == 0
    seqs, group_of, pivots, pivot_group = X2.shape_case("one_group")
    assert set(group_of) == {0}
    seqs, group_of, pivots, pivot_group = X2.shape_case("many_pivots")
    assert passes(group_of, pivot_group) == [18]


@pytest.mark.gpu
@pytest.mark.parametrize("k", (21, 33))
@pytest.mark.parametrize("name", ("two_and_none", "one_group", "many_pivots", "widths"))
def test_exp2_skm_shapes(eng, pivot_on, name, k):
    seqs, group_of, pivots, pivot_group = shape(name)
    got, _ = check(eng, seqs, group_of, pivots, pivot_group, k)
    if name == "widths":
        assert got["within_only"][1] == 0 and got["distinct_per_pivot"][1] > 0    # the pivot that is a genome of its group
        assert (got["within_hist"][4] == 0).all() and (got["across_hist"][4] == 0).all()
        assert got["within_only"][4] == 0 and got["across_only"][4] == 0 and got["distinct_per_pivot"][4] == 0
        assert 0 < got["distinct_per_pivot"][3] < got["distinct_per_pivot"][2] + 40   # the run of N starts no k-mer
    if name == "one_group":
        assert (got["across_hist"] == 0).all() and (got["across_only"] == got["distinct_per_pivot"]).all()


# ---------------------------------------------------------------- 6. declines
@functools.lru_cache(maxsize=None)
def declined_case():
    """64 genomes (the 58 of the edge case and a sixth group of six) and one pivot: no room for a pivot's bit."""
    fam = X2.related(np.random.default_rng(4242), 65, 1500)
    group_of = [g for g, n in enumerate(EDGE_SIZES + (6,)) for _ in range(n)]
    return fam[:64], group_of, fam[64:], [4]


def test_declined_case_has_64_genomes():
    seqs, group_of, pivots, pivot_group = declined_case()
    assert len(seqs) == len(group_of) == MAX_OPS and len(pivots) == 1


@pytest.mark.gpu
def test_exp2_skm_declines_64_genomes(eng, pivot_on):
    _, d = by_sets(eng, *declined_case(), 21)
    assert d["skm_cross"] == 0 and d["skm_scatter"] == 0, d


# ---------------------------------------------------------------- 7. rounds, side list, coarse overflow
ROUND, ROUNDS, SIDE_LIST = S3.ROUND, S3.ROUNDS, S3.SIDE_LIST


def instances_per_slot(k, mean, m):
    seqs, group_of, pivots, _ = small_species()
    fan = max(group_of.count(g) for g in set(group_of)) + 1               # the hint of exp2_skm: the largest group + 1
    positions = sum(max(0, len(t) - k + 1) for t in seqs + pivots)
    nslots = -(-positions // S3.planned_mean(k, mean, m, fan))
    inst = sum(max(0, len(r) - k + 1) for t in seqs + pivots for r in re.split(b"[^ACGTacgt]+", t))   # positions inside runs of bases
    assert inst == sum(sum(O.build(b"".join(b">r\n" + r + b"\n" for r in t.split(b"\n")), k, cs=1 << 30).values()) for t in seqs + pivots)
    return inst / nslots


@pytest.mark.parametrize("k,mean,m", ROUNDS)
def test_rounds_case_fills_more_than_a_round(k, mean, m):
    assert instances_per_slot(k, mean, m) > ROUND[1], instances_per_slot(k, mean, m)


@pytest.mark.gpu
@pytest.mark.parametrize("k,mean,m", ROUNDS)
def test_exp2_skm_rounds(eng, pivot_on, k, mean, m):
    pivot_on.setenv("KHOICE_SKM_MEAN", str(mean))
    if m:
        pivot_on.setenv("KHOICE_SKM_M", str(m))
    got, d = run(eng, *small_species(), k, want=species_answer(k))
    assert d["cross_multi_slots"] > 0 and d["skm_cross"] >= 1 and d["retries"] == 0 and d["setop"] == 0, d


def side_list(eng, monkeypatch, k):
    for name, value in SIDE_LIST[k].items():
        monkeypatch.setenv(name, value)
    got, d = check(eng, *small_species(), k, launches=2, want=species_answer(k))
    assert d["big_slots"] > 0, d
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("k", (21, 41))
def test_exp2_skm_side_list(eng, pivot_on, k):
    side_list(eng, pivot_on, k)


@functools.lru_cache(maxsize=None)
def coarse_overflow_case(k):
    """A fourth pivot of one tandem repeat: 120 000 positions with one minimizer (k = 41, records of at most 63 k-mers:
    200 000), thousands of records for one coarse bucket, whose region holds 2 048 and a hundredth of the mean."""
    seqs, group_of, pivots, pivot_group = small_species()
    return seqs, group_of, pivots + [b"AC" * (60_000 if k <= 32 else 100_000)], pivot_group + [0]


@pytest.mark.gpu
@pytest.mark.parametrize("k", (21, 41))
def test_exp2_skm_coarse_overflow_falls_back(eng, pivot_on, k):
    case = coarse_overflow_case(k)
    want = X2.oracle(*case, k)
    pivot_on.setenv("KHOICE_SKM_SLACK", "0.01")
    got, d = by_sets(eng, *case, k, retries=1, want=want)
    assert d["skm_scatter"] == 1 and d["builds"] == len(case[0]) + len(case[2]), d
    pivot_on.delenv(SWITCH)
    sets, d = by_sets(eng, *case, k, want=want)
    assert same(got, sets) and d["skm_scatter"] == 0, d


# ---------------------------------------------------------------- 8. clamps
@pytest.mark.gpu
@pytest.mark.parametrize("cs", (1, 2, 5000))
@pytest.mark.parametrize("hist_len", (2, 3, 5001))
def test_exp2_skm_clamps(eng, pivot_on, cs, hist_len):
    check(eng, *small_species(), 21, cs=cs, hist_len=hist_len, want=species_answer(21, cs, hist_len))


# ---------------------------------------------------------------- 9. the switch
@pytest.mark.gpu
def test_exp2_skm_switch(eng, monkeypatch):
    case = small_species()
    seqs, group_of, pivots, pivot_group = case
    monkeypatch.delenv(SWITCH, raising=False)
    monkeypatch.delenv(S3.SWITCH, raising=False)
    sets, d = by_sets(eng, *case, 21, want=species_answer(21))
    assert d["skm_cross"] == 0 and d["skm_scatter"] == 0, d
    for value in ("0", "", "2"):                                          # only "1" takes the form
        monkeypatch.setenv(SWITCH, value)
        _, d = by_sets(eng, *case, 21, want=species_answer(21))
        assert d["skm_cross"] == 0 and d["skm_scatter"] == 0, (value, d)
    monkeypatch.setenv(SWITCH, "1")
    got, _ = check(eng, *case, 21, want=species_answer(21))
    assert same(got, sets)
    monkeypatch.setenv("KHOICE_NO_SKM", "1")
    _, d = by_sets(eng, *case, 21, want=species_answer(21))
    assert d["skm_cross"] == 0 and d["skm_scatter"] == 0, d
    monkeypatch.delenv("KHOICE_NO_SKM")
    monkeypatch.setenv("KHOICE_NO_SKM2", "1")                             # two-word keys only
    _, d = by_sets(eng, *case, 41, want=species_answer(41))
    assert d["skm_cross"] == 0 and d["skm_scatter"] == 0, d
    check(eng, *case, 21, want=species_answer(21))
    monkeypatch.delenv("KHOICE_NO_SKM2")
    none, d = run(eng, seqs, group_of, [], [], 21)                        # no pivot: the set form builds the genomes only
    assert d["skm_cross"] == 0 and d["skm_scatter"] == 0 and d["retries"] == 0 and d["builds"] == len(seqs), d
    assert none["within_hist"].shape == (0, 5001)
    # the switches of types 2 and 3 are each their own
    monkeypatch.delenv(SWITCH)
    monkeypatch.setenv(S3.SWITCH, "1")
    _, d = by_sets(eng, *case, 21, want=species_answer(21))
    assert d["skm_cross"] == 0 and d["skm_scatter"] == 0, d
    monkeypatch.delenv(S3.SWITCH)
    monkeypatch.setenv(SWITCH, "1")
    eng.profile(True)
    st0 = eng.stats()
    eng.exp3_run(seqs, group_of, pivots, 21)
    d = S3.deltas(st0, eng.stats())
    eng.profile(False)
    assert d["skm_cross"] == 0 and d["skm_scatter"] == 0 and d["setop"] > 0, d


# ---------------------------------------------------------------- 10. device-resident texts
@pytest.mark.gpu
@pytest.mark.parametrize("k", (21, 41))
def test_exp2_skm_device_texts(eng, pivot_on, k):
    seqs, group_of, pivots, pivot_group = small_species()
    texts = seqs + pivots
    total = sum(len(t) for t in texts)
    host, hd = check(eng, seqs, group_of, pivots, pivot_group, k, want=species_answer(k))
    assert hd["text_packed"] == total, hd
    mixes = {"aligned": [ARENA_ALIGNED[i % 2] for i in range(len(texts))],
             "unaligned": [ARENA_UNALIGNED[i % 3] for i in range(len(texts))],
             "mixed": [(ARENA_ALIGNED + ARENA_UNALIGNED)[i % 5] for i in range(len(texts))]}
    for name, classes in mixes.items():
        arena = Arena(texts, classes, [None] * len(texts), 700 + k)
        dev = arena.upload()
        got, d = check(eng, seqs, group_of, pivots, pivot_group, k, want=species_answer(k), texts=(dev[:len(seqs)], dev[len(seqs):]))
        assert same(got, host), name
        assert d["text_packed"] == sum(len(t) for t, c in zip(texts, classes) if c % 16), (name, d)   # read in place or packed
        assert {n: v for n, v in d.items() if n != "text_packed"} == {n: v for n, v in hd.items() if n != "text_packed"}, (name, d, hd)
        assert (arena.download() == arena.host).all(), name               # and the texts are as they were


# ---------------------------------------------------------------- 11. poisoned pool
PATTERNS = S3.PATTERNS


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", PATTERNS, ids=lambda p: f"p{p:02X}")
@pytest.mark.parametrize("k", (21, 41))
def test_exp2_skm_every_k_poisoned(eng, pivot_on, k, pattern):
    pivot_on.setenv("KHOICE_DEBUG_POISON", str(pattern))
    assert every_k(eng, k)["poisoned_bytes"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", PATTERNS, ids=lambda p: f"p{p:02X}")
@pytest.mark.parametrize("k", (21, 41))
def test_exp2_skm_side_list_poisoned(eng, pivot_on, k, pattern):
    pivot_on.setenv("KHOICE_DEBUG_POISON", str(pattern))
    assert side_list(eng, pivot_on, k)["poisoned_bytes"] > 0
