"""The presence-bitmap form of kh_exp6_run (k <= 12: k_bmp_build, k_bmp_present, k_bmp_group_masks, k_read_lookup,
k_read_fold) against the plain-Python restatement of src/merge_lists.py:160-179 (tests/read_level_oracle.py) over
Python sets of the canonical k-mers of every group's genomes, and against the set form of the same call
(KHOICE_NO_BMP=1): the tie masks and the unmatched counts of every read, the within-group histograms and the distinct
counts, and which kernels ran.  The unmarked test proves on the oracle alone that the inputs hold what the GPU tests
rely on."""
import functools
import itertools
import random

import numpy as np
import pytest

from oracle import kmer_oracle as O
from tests import read_level_oracle as RL

TILE = 256                      # positions per workgroup of k_read_lookup
KS = (3, 4, 5, 8, 11, 12)
EDGE_GROUPS = ((7, 1), (7, 2), (7, 63), (7, 64), (7, 65), (7, 66), (5, 1024))      # (k, ngroups)
MAX_GROUPS = 1024
PATTERNS = (0x00, 0x41, 0x63, 0xFF)                     # of tests/test_gpu_pool_poison.py
PALINDROME_12, POLY_A_12 = "TTTTTTAAAAAA", "A" * 12     # codes 0xFFF000 (the last of sixteen ranges) and 0
KH_E_ARG = -1
CS, HIST_LEN = 5000, 64


@pytest.fixture(scope="module")
def eng():
    import torch
    from khoice_amd import build as kbuild
    from khoice_amd import engine as E
    kbuild.build_library()
    torch.cuda.init()
    e = E.Engine(0)
    yield e
    e.close()


# ---------------------------------------------------------------- helpers (restated, not imported)
def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def layout(reads):
    text = "".join(r + "\n" for r in reads).encode()
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    if reads:
        off[1:] = np.cumsum([len(r) + 1 for r in reads])
    return text, off


def genome_kmers(text, k):
    """The canonical k-mers of a genome as the build sees it: case folded, a window with any other byte left out."""
    return {RL.canonical(w) for w in O.windows(text.upper(), k) if set(w) <= set("ACGT")}


def group_sets(genomes, group_of, k):
    sets = [set() for _ in range(max(group_of) + 1)]
    for text, g in zip(genomes, group_of):
        sets[g] |= genome_kmers(text, k)
    return sets


def depth(kmer, sets):
    return sum(RL.canonical(kmer) in s for s in sets)


def find_kmer(k, sets, want, rng):
    """A k-mer that exactly `want` of the sets hold, or None: the sets' own k-mers first, then every k-mer (k <= 5) or
    2000 random ones."""
    own = sorted(set().union(*sets))
    other = ("".join(t) for t in itertools.product("ACGT", repeat=k)) if k <= 5 else (rand_seq(rng, k) for _ in range(2000))
    for kmer in itertools.chain(own, other):
        if depth(kmer, sets) == want:
            return kmer
    return None


def batches_of(off, max_pos):
    """The batches of whole reads that read_votes_batches cuts (kh_engine.cpp): their number."""
    n, b0, count = len(off) - 1, 0, 0
    while b0 < n:
        b1 = b0 + 1
        while b1 < n and int(off[b1 + 1]) - int(off[b0]) <= max_pos:
            b1 += 1
        count, b0 = count + 1, b1
    return count


def measured(eng, call):
    """(outputs, {kernel class: launches, poisoned_bytes: growth}) of one call."""
    eng.profile(True)
    st0 = eng.stats()
    out = call()
    st1 = eng.stats()
    eng.profile(False)
    d = {n: st1["kernels"].get(n, {"launches": 0})["launches"] - st0["kernels"].get(n, {"launches": 0})["launches"]
         for n in set(st1["kernels"]) | {"bmp_group_masks", "read_lookup"}}
    d["poisoned_bytes"] = st1["poisoned_bytes"] - st0["poisoned_bytes"]
    return out, d


def run6(eng, case, k):
    genomes, group_of, pivots = case
    return eng.exp6_run([g.encode() for g in genomes], group_of, [layout(p) for p in pivots], k, cs=CS, hist_len=HIST_LEN)


def same_outputs(a, b):
    assert (a["within_hist"] == b["within_hist"]).all() and (a["distinct_per_seq"] == b["distinct_per_seq"]).all()
    assert len(a["tie_masks"]) == len(b["tie_masks"])
    for p in range(len(a["tie_masks"])):
        assert a["tie_masks"][p].shape == b["tie_masks"][p].shape and (a["tie_masks"][p] == b["tie_masks"][p]).all(), p
        assert (a["unmatched"][p] == b["unmatched"][p]).all(), p


@functools.lru_cache(maxsize=None)
def wanted(name, k):
    """The oracle's (tie masks, unmatched) per pivot of a named case: computed once, shared, left unchanged."""
    genomes, group_of, pivots = CASES[name](k)
    sets = group_sets(genomes, group_of, k)
    out = []
    for reads in pivots:
        want = RL.reads_votes(reads, k, sets)
        out.append((RL.tie_masks(want, len(sets)), np.array([w[2] for w in want], dtype=np.uint32)))
    return out


def check_against_oracle(res, name, k):
    for p, (ties, unm) in enumerate(wanted(name, k)):
        assert res["tie_masks"][p].shape == ties.shape and (res["tie_masks"][p] == ties).all(), (name, k, p)
        assert (res["unmatched"][p] == unm).all(), (name, k, p)


def bitmap_form(d, pairs):
    assert d["bmp_build"] >= 1 and d["bmp_present"] == 1 and d["bmp_group_masks"] == 1, d
    assert d["read_lookup"] == pairs and d["read_masks"] == 0 and d["read_fold"] == pairs, d


def set_form(d, pairs):
    assert d["bmp_build"] == 0 and d["bmp_present"] == 0 and d["bmp_group_masks"] == 0 and d["read_lookup"] == 0, d
    assert d["read_masks"] == pairs and d["read_fold"] == pairs, d


# ---------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def base_text(k):
    """3000 random bases; an even k gets reverse-complement palindromes planted every 400 bases; k = 12 gets
    TTTTTTAAAAAA and poly-A as well."""
    rng = random.Random(600 + k)
    t = list(rand_seq(rng, 3000))
    if k % 2 == 0:
        for at in range(100, 2900, 400):
            half = rand_seq(rng, k // 2)
            t[at:at + k] = half + O.reverse_complement(half)
    if k == 12:
        t[1300:1312] = PALINDROME_12
        t[1500:1514] = "A" * 14
    return "".join(t)


@functools.lru_cache(maxsize=None)
def form_case(k):
    """Test 1: 5 groups of 1 - 3 genomes of 2 - 3 kb.  Group 1's genomes are shorter than k (an empty dataset), group 4
    is group 0 again (ties of two).  k <= 5: every group has an alphabet of its own (AC, AG, CG), or all groups would
    hold all k-mers; else the genomes are overlapping slices of one text, and one text of its own."""
    rng = random.Random(700 + k)
    if k <= 5:
        g0 = [rand_seq(rng, 2400, "AC"), rand_seq(rng, 2000, "AC")]
        g2 = [rand_seq(rng, 2200, "AG"), rand_seq(rng, 2600, "AG"), rand_seq(rng, 2000, "AG")]
        g3 = [rand_seq(rng, 3000, "CG")]
    else:
        base = base_text(k)
        g0 = [base[0:2200], base[200:2400]]
        g2 = [base[800:3000], base[1000:3000], base[600:2700]]
        g3 = [rand_seq(rng, 2000) + base[1250:1550]]
    g1 = [rand_seq(rng, k - 1), rand_seq(rng, k - 1)]
    genomes = g0 + g1 + g2 + g3 + g0
    group_of = [0] * 2 + [1] * 2 + [2] * 3 + [3] + [4] * 2
    sets = group_sets(genomes, group_of, k)
    sources = g0 + g2 + g3

    def cut(n):
        src = sources[rng.randrange(len(sources))]
        at = rng.randrange(0, len(src) - n)
        return src[at:at + n]

    reads = [cut(n) for n in (0, k - 1, k, k + 1)]
    reads += [cut(w + k - 1) for w in (63, 64, 65)]
    reads += [find_kmer(k, sets, want, rng) or "" for want in (0, 1)]             # single-window reads: L = 0, L = 1
    if k % 2 == 0:
        pal = [w for s in sources for w in O.windows(s, k) if w == O.reverse_complement(w)]
        reads.append(pal[0] if pal else "")
    if k == 12:
        reads += [PALINDROME_12, POLY_A_12, base_text(k)[1290:1320], base_text(k)[1490:1520]]
    total = sum(len(r) + 1 for r in reads)
    n = (-total - 1) % TILE + 1                    # its newline is the first byte of a tile
    while n < k + 5:
        n += TILE
    ends = len(reads)
    reads.append(cut(n))
    total = sum(len(r) + 1 for r in reads)
    n = (-total - 1) % TILE                        # the next read starts a tile
    while n < k + 5:
        n += TILE
    reads.append(cut(n))
    starts = len(reads)
    reads.append(cut(2 * k + 70))
    reads += [rand_seq(rng, n) for n in (k + 90, k, 3 * k)]
    while len(reads) < 60:
        reads.append(cut(rng.randrange(0, 2 * k + 40)))
    second = [cut(rng.randrange(0, 150)) if i % 5 else rand_seq(rng, k + i) for i in range(40)]
    special = {"ends_at_tile": ends, "starts_at_tile": starts}
    return (tuple(genomes), tuple(group_of), (tuple(reads), tuple(second))), special


@functools.lru_cache(maxsize=None)
def cells_case(k, ngroups):
    """Test 2: tiny genomes of 40 - 80 bases, one per group, none with a T in it (a k-mer with A and T in it is in no
    group: cells of zero); the reads are all 4^k k-mers, one read each, then the
    reverse complement of each, in two pivots."""
    rng = random.Random(800 + 10 * k + ngroups)
    genomes = [rand_seq(rng, rng.randrange(40, 81), ("ACG", "AC", "CG", "AG", "ACG")[g % 5]) for g in range(ngroups)]
    kmers = ["".join(t) for t in itertools.product("ACGT", repeat=k)]
    return tuple(genomes), tuple(range(ngroups)), (tuple(kmers), tuple(O.reverse_complement(m) for m in kmers))


@functools.lru_cache(maxsize=None)
def edge_case(k, ngroups):
    """Test 3: one genome of 60 - 200 bases per group, every one with the same 16 bases in it (a k-mer of all groups);
    single-window reads and reads of 63 .. 129 windows pieced together from the genomes."""
    rng = random.Random(900 + ngroups)
    shared = rand_seq(rng, 16)
    genomes = []
    for _ in range(ngroups):
        g = rand_seq(rng, rng.randrange(60, 185))
        at = rng.randrange(0, len(g))
        genomes.append(g[:at] + shared + g[at:])

    def pieced(n):
        out = ""
        while len(out) < n:
            g = genomes[rng.randrange(ngroups)]
            at = rng.randrange(0, len(g) - 30)
            out += g[at:at + 30]
        return out[:n]

    reads = [shared[:k], shared[3:3 + k], rand_seq(rng, k), genomes[0][:k], genomes[-1][-k:], ""]
    reads += [pieced(w + k - 1) for w in (63, 64, 65, 100, 127, 128, 129)]
    reads += [rand_seq(rng, k + 70), shared + pieced(40)]
    return tuple(genomes), tuple(range(ngroups)), (tuple(reads[:8]), tuple(reads[8:]))


@functools.lru_cache(maxsize=None)
def symbols_case(k):
    """Test 5: the genomes of test 1 with stretches in lower case and N in them (the reads stay clean)."""
    (genomes, group_of, pivots), _ = form_case(k)
    rng = random.Random(1000 + k)
    out = []
    for g in genomes:
        t = list(g)
        for _ in range(6 if len(t) > 100 else 0):
            at = rng.randrange(0, len(t) - 40)
            t[at:at + 30] = "".join(t[at:at + 30]).lower()
            t[rng.randrange(0, len(t))] = "N"
        out.append("".join(t))
    return tuple(out), group_of, pivots


CASES = {"form": lambda k: form_case(k)[0], "cells5": lambda k: cells_case(k, 5), "cells66": lambda k: cells_case(k, 66),
         "symbols": symbols_case}
for _k, _n in EDGE_GROUPS:
    CASES[f"edge{_n}"] = functools.partial(lambda k, n: edge_case(k, n), n=_n)


# ---------------------------------------------------------------- the inputs hold what they claim (no GPU)
def test_the_inputs_hold_what_the_gpu_tests_rely_on():
    for k in KS:
        (genomes, group_of, pivots), special = form_case(k)
        sets = group_sets(genomes, group_of, k)
        reads = pivots[0]
        _, off = layout(reads)
        assert [len(s) > 0 for s in sets] == [True, False, True, True, True] and sets[0] == sets[4]
        assert all(2000 <= len(g) <= 3300 or len(g) == k - 1 for g in genomes)
        assert [len(r) for r in reads[:4]] == [0, k - 1, k, k + 1]
        assert [len(r) - k + 1 for r in reads[4:7]] == [63, 64, 65]
        assert len(reads[7]) == k and depth(reads[7], sets) == 0                    # a single window, L = 0
        assert len(reads[8]) == k and depth(reads[8], sets) == 1                    # a single window, L = 1
        e, s = special["ends_at_tile"], special["starts_at_tile"]
        assert (int(off[e + 1]) - 1) % TILE == 0 and len(reads[e]) >= k             # the last base closes a tile
        assert int(off[s]) % TILE == 0 and len(reads[s]) >= k                       # the first base opens one
        seen = {depth(w, sets) for r in reads + pivots[1] for w in O.windows(r, k)}
        assert {0, 2} <= seen and len(seen) >= 3                                    # no set, the identical pair, more
        if k % 2 == 0:
            assert reads[9] == O.reverse_complement(reads[9]) and len(reads[9]) == k and depth(reads[9], sets) >= 1
        if k == 12:
            assert O.encode(PALINDROME_12) == 0xFFF000 and PALINDROME_12 == O.reverse_complement(PALINDROME_12)
            assert O.encode(POLY_A_12) == 0 and RL.canonical("T" * 12) == POLY_A_12
            assert depth(PALINDROME_12, sets) >= 1 and depth(POLY_A_12, sets) >= 1
            assert PALINDROME_12 in reads and POLY_A_12 in reads
            assert any(PALINDROME_12 in r and len(r) > 12 for r in reads) and any(POLY_A_12 in r and len(r) > 12 for r in reads)
        assert all(len(p) <= 300 for p in pivots)
    for k in (3, 4):
        for ngroups in (5, 66):
            genomes, group_of, pivots = cells_case(k, ngroups)
            assert len(pivots[0]) == 4 ** k == len(set(pivots[0])) and all(40 <= len(g) <= 80 for g in genomes)
            assert [O.reverse_complement(m) for m in pivots[0]] == list(pivots[1])
            sets = group_sets(genomes, group_of, k)
            depths = {depth(m, sets) for m in pivots[0]}
            assert 0 in depths and max(depths) >= 2                                 # cells of zero and of several bits
            assert any(m == O.reverse_complement(m) for m in pivots[0]) == (k % 2 == 0)
            if ngroups == 66:
                assert any(RL.canonical(m) in sets[64] or RL.canonical(m) in sets[65] for m in pivots[0])   # the second mask word
    for k, ngroups in EDGE_GROUPS:
        genomes, group_of, pivots = edge_case(k, ngroups)
        sets = group_sets(genomes, group_of, k)
        reads = pivots[0] + pivots[1]
        assert len(genomes) == ngroups and all(60 <= len(g) <= 200 for g in genomes)
        assert len(reads[0]) == k and depth(reads[0], sets) == ngroups              # a single window, L = ngroups
        assert len(reads[3]) == k and 1 <= depth(reads[3], sets)
        assert [len(r) - k + 1 for r in reads[6:13]] == [63, 64, 65, 100, 127, 128, 129]
        assert len({depth(w, sets) for r in reads for w in O.windows(r, k)}) >= min(3, ngroups + 1)
    for k in KS:
        genomes, group_of, _ = symbols_case(k)
        long = [g for g in genomes if len(g) > 100]
        assert all("N" in g and any(c in g for c in "acgt") for g in long)
        if k >= 8:                                                                  # the N's cost k-mers
            assert all(genome_kmers(a, k) != genome_kmers(b, k) for a, b in zip(genomes, form_case(k)[0][0]) if len(a) > 100)


# ---------------------------------------------------------------- 1. the form is taken, and the set form agrees
@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_the_form_is_taken_and_the_set_form_agrees(eng, k, monkeypatch):
    monkeypatch.delenv("KHOICE_NO_BMP", raising=False)
    case, _ = form_case(k)
    genomes, group_of, pivots = case
    res, d = measured(eng, lambda: run6(eng, case, k))
    bitmap_form(d, len(pivots))
    check_against_oracle(res, "form", k)
    ref4 = eng.exp4_run([g.encode() for g in genomes], group_of, [], k, cs=CS, hist_len=HIST_LEN)
    assert (res["within_hist"] == ref4["within_hist"]).all() and res["within_hist"].sum() > 0
    assert (res["distinct_per_seq"] == ref4["distinct_per_seq"]).all()
    monkeypatch.setenv("KHOICE_NO_BMP", "1")
    ref, d = measured(eng, lambda: run6(eng, case, k))
    set_form(d, len(pivots))
    same_outputs(res, ref)


# ---------------------------------------------------------------- 2. every cell of the table
@pytest.mark.gpu
@pytest.mark.parametrize("ngroups", (5, 66))
@pytest.mark.parametrize("k", (3, 4))
def test_every_cell_of_the_table(eng, k, ngroups):
    case = cells_case(k, ngroups)
    genomes, group_of, pivots = case
    res, d = measured(eng, lambda: run6(eng, case, k))
    bitmap_form(d, 2)
    check_against_oracle(res, f"cells{ngroups}", k)
    sets = group_sets(genomes, group_of, k)
    everyone = RL.tie_masks([([], list(range(ngroups)), 0)], ngroups)[0]
    for p, reads in enumerate(pivots):
        for i, kmer in enumerate(reads):                    # a one-window read: its tie mask is its membership mask
            held = [g for g in range(ngroups) if RL.canonical(kmer) in sets[g]]
            cell = RL.tie_masks([([], held, 0)], ngroups)[0]
            assert (res["tie_masks"][p][i] == (cell if held else everyone)).all(), (kmer, held)
            assert res["unmatched"][p][i] == (0 if held else 1), kmer


# ---------------------------------------------------------------- 3. group-count edges
@pytest.mark.gpu
@pytest.mark.parametrize("k,ngroups", EDGE_GROUPS)
def test_numbers_of_groups(eng, k, ngroups):
    case = edge_case(k, ngroups)
    res, d = measured(eng, lambda: run6(eng, case, k))
    bitmap_form(d, 2)
    check_against_oracle(res, f"edge{ngroups}", k)
    assert res["tie_masks"][0].shape[1] == max(1, (ngroups + 63) // 64)


@pytest.mark.gpu
def test_one_group_too_many(eng, monkeypatch):
    from khoice_amd import engine as E
    k = 5
    genomes, group_of, pivots = edge_case(k, MAX_GROUPS)
    genomes, group_of = genomes + (genomes[0],), group_of + (MAX_GROUPS,)
    texts = []
    for no_bmp in (False, True):
        monkeypatch.setenv("KHOICE_NO_BMP", "1") if no_bmp else monkeypatch.delenv("KHOICE_NO_BMP", raising=False)
        with pytest.raises(E.KhoiceError) as ei:
            run6(eng, (genomes, group_of, (pivots[0][:2],)), k)
        assert ei.value.code == KH_E_ARG, str(ei.value)
        texts.append(str(ei.value))
    assert texts[0] == texts[1] and str(MAX_GROUPS) in texts[0], texts


# ---------------------------------------------------------------- 4. batches
@pytest.mark.gpu
def test_several_batches_give_the_single_batch_outputs(eng, monkeypatch):
    k = 8
    case, _ = form_case(k)
    pivots = case[2]
    one = run6(eng, case, k)
    offs = [layout(p)[1] for p in pivots]
    max_pos = int(offs[0][-1]) // 4
    want = [batches_of(off, max_pos) for off in offs]
    assert min(want) >= 3, want
    monkeypatch.setenv("KHOICE_READS_MAX_POS", str(max_pos))
    many, d = measured(eng, lambda: run6(eng, case, k))
    bitmap_form(d, sum(want))
    same_outputs(one, many)
    check_against_oracle(many, "form", k)


# ---------------------------------------------------------------- 5. symbols
@pytest.mark.gpu
@pytest.mark.parametrize("k", (5, 12))
def test_lower_case_and_n_in_the_genomes(eng, k, monkeypatch):
    case = symbols_case(k)
    res, d = measured(eng, lambda: run6(eng, case, k))
    bitmap_form(d, 2)
    check_against_oracle(res, "symbols", k)
    monkeypatch.setenv("KHOICE_NO_BMP", "1")
    same_outputs(res, run6(eng, case, k))


@pytest.mark.gpu
@pytest.mark.parametrize("what", ("lower", "N", "CR"))
def test_bad_symbols_in_the_reads(eng, what, monkeypatch):
    from khoice_amd import engine as E
    k = 8
    (genomes, group_of, pivots), _ = form_case(k)
    second = list(pivots[1])
    long = [i for i, r in enumerate(second) if len(r) >= k + 2 and i > 3]
    lo, hi = long[2], long[-1]                             # two bad reads of the second pivot, in different batches
    spoil = {"lower": lambda r: r[:2] + r[2].lower() + r[3:], "N": lambda r: r[:-1] + "N", "CR": lambda r: r[:1] + "\r" + r[2:]}[what]
    second[lo], second[hi] = spoil(second[lo]), spoil(second[hi])
    second[3] = {"lower": "acg", "N": "NNN", "CR": "A\rC"}[what]   # shorter than k: no k-mer, no error
    case = (genomes, group_of, (pivots[0], tuple(second)))
    off = layout(second)[1]
    max_pos = int(off[-1]) // 4
    assert batches_of(off, max_pos) >= 3 and batches_of(off[:lo + 2], max_pos) < batches_of(off[:hi + 2], max_pos)
    monkeypatch.setenv("KHOICE_READS_MAX_POS", str(max_pos))
    texts = []
    for no_bmp in (False, True):
        monkeypatch.setenv("KHOICE_NO_BMP", "1") if no_bmp else monkeypatch.delenv("KHOICE_NO_BMP", raising=False)
        with pytest.raises(E.KhoiceError) as ei:
            run6(eng, case, k)
        assert ei.value.code == KH_E_ARG and f"read {lo} " in str(ei.value), str(ei.value)
        texts.append(str(ei.value))
    assert texts[0] == texts[1], texts
    monkeypatch.delenv("KHOICE_NO_BMP")
    second[lo], second[hi] = pivots[1][lo], pivots[1][hi]  # only the short read left: an answer, the oracle's
    clean = (genomes, group_of, (pivots[0], tuple(second)))
    res, d = measured(eng, lambda: run6(eng, clean, k))
    assert d["read_lookup"] >= 4 and d["read_masks"] == 0, d
    whole = list(wanted("form", k)[1])
    assert (np.delete(res["tie_masks"][1], 3, axis=0) == np.delete(whole[0], 3, axis=0)).all()
    assert (np.delete(res["unmatched"][1], 3) == np.delete(whole[1], 3)).all() and res["unmatched"][1][3] == 0
    assert res["tie_masks"][1][3, 0] == (1 << 5) - 1       # no window: every group ties


# ---------------------------------------------------------------- 6. declines
@pytest.mark.gpu
def test_too_small_a_budget_for_the_table_declines(eng, monkeypatch):
    k = 8
    case, _ = form_case(k)
    res = run6(eng, case, k)
    monkeypatch.setenv("KHOICE_BMP_MAX_BYTES", str(64 * 4 ** k // 64 * 8))   # the table alone: 64 rows of 4^k / 64 words
    ref, d = measured(eng, lambda: run6(eng, case, k))
    set_form(d, 2)
    same_outputs(res, ref)
    check_against_oracle(ref, "form", k)


@pytest.mark.gpu
def test_k13_takes_the_form_when_asked(eng, monkeypatch):
    k = 13
    rng = random.Random(13)
    base = rand_seq(rng, 3000)
    genomes = (base[:2000], base[500:2500], base[1000:3000], rand_seq(rng, 2000))
    group_of = (0, 0, 1, 2)
    reads = tuple([base[at:at + n] for at, n in ((0, 12), (5, 13), (40, 14), (700, 150), (1800, 300), (2600, 75))] +
                  [rand_seq(rng, 60), ""])
    case = (genomes, group_of, (reads,))
    ref, d = measured(eng, lambda: run6(eng, case, k))
    set_form(d, 1)                                          # k = 13 is the set form's by default
    monkeypatch.setenv("KHOICE_BMP_MAX_K", "13")
    res, d = measured(eng, lambda: run6(eng, case, k))
    bitmap_form(d, 1)
    same_outputs(res, ref)
    want = RL.reads_votes(reads, k, group_sets(genomes, group_of, k))
    assert (res["tie_masks"][0] == RL.tie_masks(want, 3)).all()
    assert (res["unmatched"][0] == np.array([w[2] for w in want], dtype=np.uint32)).all()


# ---------------------------------------------------------------- 7. stale memory
@pytest.mark.gpu
@pytest.mark.parametrize("pattern", PATTERNS, ids=lambda p: f"p{p:02X}")
def test_poisoned_pool(eng, pattern, monkeypatch):
    for name, case, k in (("form", form_case(8)[0], 8), ("cells66", cells_case(4, 66), 4)):
        monkeypatch.delenv("KHOICE_DEBUG_POISON", raising=False)
        clean, d0 = measured(eng, lambda: run6(eng, case, k))
        assert d0["poisoned_bytes"] == 0, d0
        monkeypatch.setenv("KHOICE_DEBUG_POISON", str(pattern))
        got, d1 = measured(eng, lambda: run6(eng, case, k))
        monkeypatch.delenv("KHOICE_DEBUG_POISON")
        assert d1["poisoned_bytes"] > 0, d1
        bitmap_form(d1, 2)
        same_outputs(got, clean)
        check_against_oracle(got, name, k)


# ---------------------------------------------------------------- 8. device-resident inputs
@pytest.mark.gpu
def test_genomes_and_reads_in_device_buffers(eng):
    import torch
    k = 8
    case, _ = form_case(k)
    genomes, group_of, pivots = case
    host = run6(eng, case, k)
    keep = [torch.frombuffer(bytearray(g.encode()), dtype=torch.uint8).to("cuda:0") for g in genomes]
    texts = [layout(p) for p in pivots]
    dev = [torch.frombuffer(bytearray(t), dtype=torch.uint8).to("cuda:0") for t, _ in texts]
    torch.cuda.synchronize()
    res, d = measured(eng, lambda: eng.exp6_run([(t.data_ptr(), t.numel()) for t in keep], group_of,
                                                [((b.data_ptr(), len(t)), off) for b, (t, off) in zip(dev, texts)], k,
                                                cs=CS, hist_len=HIST_LEN))
    bitmap_form(d, 2)
    same_outputs(res, host)
    check_against_oracle(res, "form", k)
