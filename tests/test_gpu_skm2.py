"""The two-word super-k-mer kernels (khoice_amd/csrc/kh_skm2.hip: k_skm2_scatter, k_skm2_regroup, k_skm2_union,
k_skm2_big), which take 33 <= k <= 63, bit-exact against the C restatement (oracle.c_oracle.exp1).  Every case also
asserts that the super-k-mer form did the work: one skm_union launch, no retry, no union_tagged launch, and a record
count that is a function of the input alone.

  * every k = 33 .. 63, so every scatter instantiation the planner can pick (windows of 18 .. 48 m-mers);
  * edge inputs at one k per window width: runs far longer than nmax, tandem repeats shorter than a window, runs that
    cross a thread boundary with p_tr + lead around nmax, N every k + j bases, lower case, short and sub-tile-edge
    lengths, several tiles, ends in 32 T and starts in 32 A;
  * distinct keys that share the word the hash set claims with its compare-and-swap, and (k >= 49) pairs that also
    share the probe sequence: the second word must keep them apart;
  * the LDS histogram stripes (sshift 2 / 1 / 0) of both unions at their bin-count boundaries."""
import random
import re

import numpy as np
import pytest

from khoice_amd import synth
from oracle import c_oracle as CO
from tests.util import random_dna

M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
ALL_K = list(range(33, 64))
# one k per window width (w = 18, 21, ..., 48), and k = 55 .. 63 where nmax = 118 - k cuts records below 63 k-mers
EDGE_K = [33, 35, 38, 41, 44, 47, 50, 53, 55, 56, 59, 62, 63]


def geometry(k):
    """(m, w, nmax) as skm_plan picks them for two-word keys: m = 16, 15 or 14, whichever makes w = k - m + 1 a
    multiple of 3 (the scatter is instantiated for every third width)."""
    m = {0: 16, 1: 14, 2: 15}[k % 3]
    return m, k - m + 1, min(63, 118 - k)


# ---- restatements of kh_skm_device.h / kh_skm2.hip (what decides a k-mer's slot and its hash-set probes)
def mmer_hash(canon):
    h = (canon * 0x9E3779B1) & M32
    return h ^ (h >> 15)


def slot_of(minv, nslots):
    x = (minv * 0xC2B2AE35) & M32
    x ^= x >> 16
    x = (x * 0x27D4EB2F) & M32
    x ^= x >> 15
    return (x * nslots) >> 32


def key2_hash(lo, hi):
    return ((lo ^ (lo >> 32) ^ hi ^ (hi >> 32)) & M32) * 0x9E3779B1 & M32


def code_of(s):
    c = 0
    for ch in s:
        c = (c << 2) | CODE[ch]
    return c


def revcomp(s):
    return "".join(COMP[ch] for ch in reversed(s))


def minimizer(kmer, m):
    """min over the k-mer's m-mers of mmer_hash(canonical m-mer), as k_skm2_scatter computes it."""
    return min(mmer_hash(min(code_of(kmer[i:i + m]), code_of(revcomp(kmer[i:i + m])))) for i in range(len(kmer) - m + 1))


# ---- running one case
@pytest.fixture(scope="module")
def eng():
    from khoice_amd import build as kbuild
    from khoice_amd import engine as E
    kbuild.build_library()
    e = E.Engine(0)
    yield e
    e.close()


def run(eng, seqs, group_of, k, cs, hist_len, across=True):
    """(result, what the call did: launches per kernel class, retries, records, overfull slots)"""
    eng.profile(True)
    st0 = eng.stats()
    got = eng.exp1_run(seqs, group_of, k, cs=cs, hist_len=hist_len, across=across)
    st1 = eng.stats()
    eng.profile(False)
    did = {name: st1["kernels"][name]["launches"] - st0["kernels"][name]["launches"]
           for name in ("skm_union", "skm_big", "union_tagged")}
    for name in ("retries", "skm_records", "big_slots"):
        did[name] = st1[name] - st0[name]
    return got, did


def same(got, want):
    assert (got["distinct_per_seq"] == want["distinct_per_seq"]).all()
    assert (got["within_hist"] == want["within_hist"]).all()
    assert (got["across_hist"] == want["across_hist"]).all()


def check(eng, seqs, group_of, k, cs=5000, hist_len=5001, unions=1):
    """The oracle's answer, from the super-k-mer form (`unions` launches of the union, nothing declined)."""
    want = CO.exp1(seqs, group_of, k, cs=cs, hist_len=hist_len)
    got, did = run(eng, seqs, group_of, k, cs, hist_len)
    assert did["skm_union"] == unions and did["retries"] == 0 and did["union_tagged"] == 0, did
    assert did["skm_records"] > 0
    same(got, want)
    again, did2 = run(eng, seqs, group_of, k, cs, hist_len)     # same input, same records
    assert did2 == did
    same(again, want)
    return did


SKM_LINE = re.compile(r"\[skm\] k=(\d+) m=(\d+) w=(\d+) nmax=(\d+)")
WIDTHS_SEEN = {}   # k -> w, from the engine's own debug line


def small_set():
    items = synth.species_set(2, 2, 40_000)
    return [t for _, _, t in items], [s - 1 for s, _, _ in items]


def run_k_with_debug(eng, k, capfd, monkeypatch):
    seqs, group_of = small_set()
    monkeypatch.setenv("KHOICE_SKM_DEBUG", "1")
    capfd.readouterr()
    want = CO.exp1(seqs, group_of, k, cs=5000, hist_len=5001)
    got, did = run(eng, seqs, group_of, k, 5000, 5001)
    lines = SKM_LINE.findall(capfd.readouterr().err)
    monkeypatch.delenv("KHOICE_SKM_DEBUG")
    assert did["skm_union"] == 1 and did["retries"] == 0 and did["union_tagged"] == 0 and did["skm_records"] > 0, did
    same(got, want)
    assert len(lines) == 1, lines
    kk, m, w, nmax = (int(x) for x in lines[0])
    assert (kk, m, w, nmax) == (k,) + geometry(k)
    WIDTHS_SEEN[k] = w
    return seqs, group_of, did


@pytest.mark.gpu
@pytest.mark.parametrize("k", ALL_K)
def test_every_k(eng, k, capfd, monkeypatch):
    """k -> (m, w): 33 -> (16, 18); 34 .. 36 -> 21; 37 .. 39 -> 24; 40 .. 42 -> 27; 43 .. 45 -> 30; 46 .. 48 -> 33;
    49 .. 51 -> 36; 52 .. 54 -> 39; 55 .. 57 -> 42; 58 .. 60 -> 45; 61 .. 63 -> 48, m = 16 / 14 / 15 for k = 0 / 1 / 2
    mod 3; nmax = min(63, 118 - k)."""
    seqs, group_of, did = run_k_with_debug(eng, k, capfd, monkeypatch)
    again, did2 = run(eng, seqs, group_of, k, 5000, 5001)
    assert did2 == did
    same(again, CO.exp1(seqs, group_of, k, cs=5000, hist_len=5001))


@pytest.mark.gpu
def test_every_window_width_reached(eng, capfd, monkeypatch):
    """Across k = 33 .. 63 the engine ran every scatter width 18, 21, ..., 48 (the k of test_every_k that did not run
    in this session are run here).  w = 51 is compiled too, but k <= 63 never asks for it (it would need k >= 64 with
    m = 14 .. 16), so no test can reach it."""
    for k in ALL_K:
        if k not in WIDTHS_SEEN:
            run_k_with_debug(eng, k, capfd, monkeypatch)
    assert sorted(set(WIDTHS_SEEN[k] for k in ALL_K)) == list(range(18, 49, 3))


# ---- edge inputs
def boundary_runs(k, rng):
    """Runs of k-mers with one minimizer that start `p_tr` positions before a thread boundary (32 positions) and go
    `lead` positions past it, p_tr + lead just below, at and just above min(nmax, 62).  A run is made by an A run of
    X >= m bases flanked by other bases: every k-mer that holds all m-mer A^m (hash 0, the least) has it as its
    minimizer, which makes exactly X - m + w such k-mers."""
    m, w, nmax = geometry(k)
    top = min(nmax, 62)
    lengths = sorted({max(w, top - 1), max(w, top), top + 1, max(w, 40)})
    shapes = []
    for L in lengths:
        for p_tr in sorted({L - 31, L // 2, 31, 1}):
            if 1 <= p_tr <= 31 and L - p_tr >= 1:
                shapes.append((p_tr, L - p_tr))
    t = list(random_dna(rng, 96 + 192 * len(shapes) + 2 * k, "CGT"))
    for i, (p_tr, lead) in enumerate(shapes):
        thread = 4 + 6 * i                                 # (never the last lane of a wave: the merge is inside a wave)
        s = 32 * (thread + 1) - p_tr                       # first position of the run
        a, X = s + (k - m), p_tr + lead - w + m
        t[a - 1], t[a + X] = "C", "G"
        t[a:a + X] = "A" * X
    return "".join(t)


def edge_inputs(k, seed):
    rng = random.Random(seed * 1000 + k)
    body = random_dna(rng, 60_000)
    u5, u11, u17 = random_dna(rng, 5), random_dna(rng, 11), random_dna(rng, 17)
    every = [("".join(body[i:i + k + j - 1] + "N" for i in range(0, 6_000, k + j)))
             for j in (1, 2, 5, 17, 31)]                                           # an N every k + j bases
    seqs = [
        "A" * 6_000 + body[:2_000] + "C" * 3_000,                                  # homopolymers: runs far past nmax
        ("AC" * 3_000) + "\n" + ("AT" * 2_000) + "\n" + ("GGT" * 1_500),           # dinucleotide / trinucleotide runs
        u5 * 800 + body[2_000:4_000] + u11 * 400 + "N" + u17 * 300,                # tandem units shorter than any window
        boundary_runs(k, rng),
        *every,
        body[4_000:20_000].lower(),                                                # lower case
        body[20_000:20_000 + k - 1], body[20_100:20_100 + k], body[20_200:20_200 + k + 1],
        body[21_000:21_000 + 8_192 + k - 2], body[21_000:21_000 + 8_192 + k - 1], body[30_000:30_000 + 8_192 + k],
        body[20_000:60_000],                                                       # several tiles
        body[:5_000] + "T" * 32, "A" * 32 + body[5_000:10_000],                    # ends in 32 T, starts with 32 A
        "T" * 2_000 + "A" * 2_000,
    ]
    return [s.encode() for s in seqs], [i % 4 for i in range(len(seqs))]


@pytest.mark.gpu
@pytest.mark.parametrize("k", EDGE_K)
def test_edge_inputs(eng, k):
    seqs, group_of = edge_inputs(k, 1)
    check(eng, seqs, group_of, k, hist_len=64)
    check(eng, seqs, group_of, k, cs=2, hist_len=5)


def insertion_sequence_set(copies=120, genomes=4, seed=3):
    """Genomes of 20 kb that each carry `copies` copies of one 400-base insertion sequence: each of its minimizers
    puts copies x genomes records in one slot, more than the union holds (448), so those slots go to k_skm2_big."""
    rng = random.Random(seed)
    ins = random_dna(rng, 400)
    seqs = []
    for g in range(genomes):
        parts = []
        for c in range(copies):
            parts.append(random_dna(rng, 150))
            parts.append(ins)
        parts.append(random_dna(rng, 2_000))
        seqs.append("".join(parts).encode())
    return seqs, [g // 2 for g in range(genomes)]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [35, 47, 59])
def test_overfull_slots_go_to_big(eng, k):
    seqs, group_of = insertion_sequence_set()
    did = check(eng, seqs, group_of, k, hist_len=64)
    assert did["big_slots"] > 0 and did["skm_big"] == 1, did


# ---- keys that share the claimed word
def collision_family(k, n, shared, seed, pairs=0):
    """Up to n distinct canonical k-mers that share `shared` ("last": the last 32 bases, the word k_skm2_union claims
    with its compare-and-swap; "first": the first 32) and their minimizer (the all-A m-mer, hash 0, inside the shared
    part: one slot whatever nslots is).  `pairs` of them (k >= 49) are a member with the same 2-bit pattern XOR-ed into
    two bases 16 apart in the other word: key2_hash folds that word to 32 bits, so the pair has one probe sequence.
    At k = 33 one base is free: at most four keys, and key2_hash puts them about 1100 entries apart in k_skm2_union's
    table (the fold differs in two bits, times one odd constant), so there they meet only in a crowded table."""
    m, _, _ = geometry(k)
    rng = random.Random(seed)
    if shared == "last":
        fixed = "A" * m + random_dna(rng, 31 - m, "CGT") + "A"        # last base A: the reverse complement starts with T
        make = lambda: "A" + random_dna(rng, k - 33) + fixed if k > 33 else rng.choice("ACGT") + fixed
        other = range(0, k - 32 - 16)                                 # bases of the high word with a partner 16 on
    else:
        fixed = "A" * m + random_dna(rng, 32 - m, "CGT")
        make = lambda: fixed + random_dna(rng, k - 33) + "A" if k > 33 else fixed + rng.choice("ACGT")
        other = range(32, k - 16)                                     # bases of the low word past the shared 32
    out, seen = [], set()

    def add(s):
        if s not in seen and code_of(s) < code_of(revcomp(s)):
            seen.add(s)
            out.append(s)
            return True
        return False

    for _ in range(50 * n):
        if len(out) >= n - pairs:
            break
        add(make())
    base = list(out)
    made = 0
    for _ in range(50 * max(1, pairs)):
        if made >= pairs:
            break
        s = list(rng.choice(base))
        j = rng.choice(list(other))
        p = rng.choice((1, 2, 3))
        for q in (j, j + 16):
            s[q] = "ACGT"[CODE[s[q]] ^ p]
        made += add("".join(s))
    return out


FAMILY_K = [33, 41, 49, 55, 63]


def family_cases(k):
    pairs = 60 if k >= 49 else 0
    return [(shared, collision_family(k, 160, shared, 7 * k + (shared == "last"), pairs)) for shared in ("last", "first")]


def family_genomes(kmers, ngen=6):
    """Each k-mer a record of its own in genome i % ngen, every fifth also in another group's genome."""
    recs = [[] for _ in range(ngen)]
    for i, s in enumerate(kmers):
        recs[i % ngen].append(s)
        if i % 5 == 0:
            recs[(i + 3) % ngen].append(s)
    return ["\n".join(r).encode() for r in recs], [g // 2 for g in range(ngen)]


@pytest.mark.parametrize("k", FAMILY_K)
def test_collision_family_preconditions(k):
    """What the GPU collision test relies on, checked against the oracle's own keys (CO.count): every k-mer canonical
    as written, the shared word equal, the minimizer (so the slot) equal, and for k >= 49 the pairs' key2_hash equal."""
    m, _, _ = geometry(k)
    for shared, fam in family_cases(k):
        assert len(set(fam)) == len(fam) >= (3 if k == 33 else 160)
        lo, hi = [], []
        for s in fam:
            keys, counts = CO.count(s.encode(), k).arrays()
            assert keys.shape == (1, 2) and int(counts[0]) == 1
            c = code_of(s)
            assert int(keys[0, 0]) == c & M64 and int(keys[0, 1]) == c >> 64     # canonical as written
            lo.append(int(keys[0, 0]))
            hi.append(int(keys[0, 1]))
        word = lo if shared == "last" else hi
        assert len(set(word)) == 1
        assert len(set(zip(lo, hi))) == len(fam)
        mins = {minimizer(s, m) for s in fam}
        assert mins == {0}
        for ns in (1, 7, 1000, 500_000):                                   # one slot whatever nslots is
            assert len({slot_of(mn, ns) for mn in mins}) == 1
        if k >= 49:
            by_hash = {}
            for a, b in zip(lo, hi):
                by_hash.setdefault(key2_hash(a, b), []).append((a, b))
            assert sum(len(v) - 1 for v in by_hash.values()) >= 50          # pairs on one probe sequence
            if shared == "last":
                assert any(len({b for _, b in v}) > 1 for v in by_hash.values())


@pytest.mark.gpu
@pytest.mark.parametrize("k", FAMILY_K)
def test_same_claim_word_keys_stay_apart(eng, k):
    """One slot of 160 distinct keys (about 190 records: the union's table, not k_skm2_big) that share their claimed
    word: every probe that meets an occupied entry has to compare the other word."""
    for shared, fam in family_cases(k):
        seqs, group_of = family_genomes(fam)
        did = check(eng, seqs, group_of, k, hist_len=16)
        assert did["skm_big"] == 0, (shared, did)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [41, 55])
def test_same_claim_word_keys_in_big(eng, k):
    """1200 keys of one family in one slot: more records than the union takes, so k_skm2_big counts them."""
    fam = collision_family(k, 1200, "last", 11 * k, 200 if k >= 49 else 0)
    seqs, group_of = family_genomes(fam)
    did = check(eng, seqs, group_of, k, hist_len=16)
    assert did["big_slots"] >= 1 and did["skm_big"] == 1, did


# ---- histogram stripes
def layout_set(ngenomes, ngroups, seed=5, length=3_000):
    """ngenomes related genomes in ngroups groups (sizes as equal as they come), with a block shared by all."""
    rng = random.Random(seed)
    shared = random_dna(rng, 800)
    anc = [random_dna(rng, length) for _ in range(ngroups)]
    seqs, group_of = [], []
    for i in range(ngenomes):
        g = i % ngroups
        t = list(anc[g])
        for _ in range(len(t) // 100):
            t[rng.randrange(len(t))] = rng.choice("ACGT")
        seqs.append(("".join(t) + "\n" + shared).encode())
        group_of.append(g)
    return seqs, group_of


LAYOUTS = [(64, 1, 67, 2), (63, 4, 72, 2), (64, 4, 73, 1), (63, 40, 144, 1), (64, 40, 145, 0), (64, 64, 193, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 41])
@pytest.mark.parametrize("ngenomes,ngroups,nbins,sshift", LAYOUTS)
def test_bin_layouts(eng, k, ngenomes, ngroups, nbins, sshift):
    """nbins = genomes + 2 groups + 1 decides the union's LDS histogram stripes: 4 copies per bin up to 72 bins, 2 up
    to 144, 1 above.  k = 31: k_skm_union, k = 41: k_skm2_union.  cs below the largest group (counts clamp)."""
    assert ngenomes + 2 * ngroups + 1 == nbins
    assert sshift == (2 if nbins <= 72 else (1 if nbins <= 144 else 0))
    seqs, group_of = layout_set(ngenomes, ngroups)
    largest = max(np.bincount(group_of))
    check(eng, seqs, group_of, k, cs=5000, hist_len=80)
    check(eng, seqs, group_of, k, cs=max(1, min(3, largest - 1)), hist_len=80)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 41])
def test_bin_layout_two_pass(eng, k):
    """128 genomes in 64 groups of 2: two batches of 32 groups, then the pass by group (3 x 64 + 1 = 193 bins, one
    copy per bin).  cs = 1 below the groups' size; hist_len = 2 (its least) below the across-group counts."""
    seqs, group_of = layout_set(128, 64, seed=6, length=2_000)
    check(eng, seqs, group_of, k, cs=1, hist_len=2, unions=3)
    check(eng, seqs, group_of, k, cs=5000, hist_len=80, unions=3)
