"""The batched build kh_build_batch (pass A / B, the bucket plan, pass C) and its grid-mode twins at every tile,
bucket and sort-tier edge, bit-exact against the C restatement (oracle.c_oracle.count / exp1).

Random DNA puts Poisson-tight counts in every bucket and about 0.4 keys in a fine bin, so the bitonic fallback, the
repair work list at its limit, the oversize fold at its pair capacity, the re-plan and rle_emit's ranking of kept runs
are reached rarely or never.  Here the inputs are built for them:

  * planted keys (tests/util.py: planted_codes, planted_text): canonical k-mers chosen by the slot and the fine bin of
    their MIXED key, written one per N-separated word in shuffled order and followed by a run of N.  N adds k-mer
    start positions (so buckets: nbuckets = ceil(npos / mean)) but no keys: a bucket's key count, its distinct count,
    the fill of its fine bins and the number of buckets are all chosen independently;
  * extraction edges: an N (a run of 1, 2 or k) at every offset around the code-word, thread, sub-tile, staging-round
    and tile boundaries, and sequences that end at every such boundary -2 .. +2, through both scatter forms, both
    start orders, every tile size, device-resident inputs at unaligned addresses and forced chunking;
  * bucket-plan edges: batches of 4095 .. 8193 buckets (k_exscan's tiles), 63 .. 129 segments of mixed depth (the
    64-segment interleave), segments of 1 .. 300 tiles (k_col_*'s 8 tile groups) and of 1 .. 4096 buckets;
  * the same planted families through the key-array form of kh_exp1_run (KHOICE_NO_SKM).

The CPU tests read the constants out of the sources and prove every construction on the oracle's keys (per-bucket key
count, distinct count, fullest fine bin, keys in bins with more than one distinct key), so a retune fails there
instead of weakening a case."""
import functools
import hashlib
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import c_oracle as CO
from tests.util import (CAP, FINE_BITS, MEAN, Planted, codes_text, fine_bin_np, grid_sub_ranges, key_view, mix_np,
                        planted_text, random_dna_np, slot_np, words)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "khoice_amd", "csrc")

# ---- the plan and sort-tier constants (test_constants_match_sources reads them out of the sources)
# (MEAN, CAP and FINE_BITS live in tests/util.py beside Planted, which needs them)
FINE_LIMIT = 64                  # fullest fine bin the in-bin repair accepts
WORKLIST = 1024                  # keys of out-of-order bins the repair lists
SUBTILE, SUBTILES_PER_TILE, HALO = 8192, 8, 96
MAX_BUCKETS_PER_SEG = 16384
SCAN_TILE = 4096                 # k_exscan
ST_THREADS = 1024                # k_extract_staged
COL_TY = 8                       # tile groups of k_col_totals / k_col_offsets
SORT_THREADS = 512
MIN_TILE = 2 * SUBTILE           # smallest tile (KHOICE_TILE_POS is rounded to its multiples); the default of a small batch
BIG = 1 << 30                    # a counter ceiling nothing here reaches


def capp(w):
    """Pair capacity of the oversize fold: keys[capp] | counters[capp] inside the key region of `cap` keys."""
    return ((CAP[w] * 8 * w) // (8 * w + 4)) & ~63


def _src(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def test_constants_match_sources():
    com, ker, dev, eng = _src("kh_common.h"), _src("kh_kernels.hip"), _src("kh_device.h"), _src("kh_engine.cpp")

    def num(pattern, text):
        return int(re.search(pattern, text).group(1))
    assert num(r"#define KH_TUNE_MEAN_W1 (\d+)", com) == MEAN[1]
    assert "constexpr int KH_BUCKET_MEAN_W1 = KH_TUNE_MEAN_W1;" in com
    assert num(r"constexpr int KH_BUCKET_MEAN_W2 = (\d+);", com) == MEAN[2]
    assert num(r"constexpr int KH_SORT_CAP_W1 = (\d+);", com) == CAP[1]
    assert num(r"constexpr int KH_SORT_CAP_W2 = (\d+);", com) == CAP[2]
    assert num(r"#define KH_TUNE_FINE_BITS (\d+)", com) == FINE_BITS
    assert "constexpr int KH_FINE_BITS = KH_TUNE_FINE_BITS;" in com
    assert num(r"constexpr int KH_FINE_LIMIT = (\d+);", com) == FINE_LIMIT
    assert num(r"constexpr int KH_WORKLIST = (\d+);", com) == WORKLIST
    assert num(r"constexpr int KH_SUBTILE = (\d+);", com) == SUBTILE
    assert num(r"constexpr int KH_SUBTILES_PER_TILE = (\d+);", com) == SUBTILES_PER_TILE
    assert num(r"constexpr int KH_HALO = (\d+);", dev) == HALO
    assert num(r"constexpr int KH_MAX_BUCKETS_PER_SEG = (\d+);", com) == MAX_BUCKETS_PER_SEG
    assert num(r"constexpr u32 KH_SCAN_TILE = (\d+);", ker) == SCAN_TILE
    assert num(r"constexpr u32 KH_ST_THREADS = (\d+);", ker) == ST_THREADS
    assert num(r"constexpr u32 KH_COL_TY = (\d+);", ker) == COL_TY
    assert num(r"constexpr int KH_SORT_THREADS = (\d+);", com) == SORT_THREADS
    # what the cases lean on besides the numbers
    assert "const u32 capp = ((cap * 8u * W) / (8u * W + 4u)) & ~63u;" in ker
    assert (capp(1), capp(2)) == (2688, 1600)
    assert "constexpr int IT = KH_WORKLIST / NT;" in ker and WORKLIST // SORT_THREADS == 2
    assert "if (bmax > (u32)KH_FINE_LIMIT)" in ker and "if (wlc > (u32)KH_WORKLIST)" in ker
    assert "if (acc >= capp) { fail = true; break; }" in ker
    assert "return frac >> (32 - KH_FINE_BITS);" in ker
    assert "const u32 next = std::max<u32>(floor_mean, mean / 4);" in eng
    assert "std::max<u64>(1, (s.npos + mean - 1) / mean)" in eng
    assert "for (int s0 = 0; s0 < nseq; s0 += 64)" in eng                       # the start-order interleave
    assert "nb_alloc <= 4 * KH_ST_THREADS" in ker and "<= 160 * 1024" in ker     # when pass B stages
    assert "std::max<u32>(2 * KH_SUBTILE, (u32)strtoul(ev, nullptr, 10) / (2 * KH_SUBTILE) * (2 * KH_SUBTILE))" in eng


def staged(w, nb):
    """kh_launch_extract's choice (kh_extract_staged_lds_bytes): pass B stages through LDS up to this many buckets."""
    nb_alloc = (nb + 3) & ~3
    sub = 2 * SUBTILE if w == 1 else SUBTILE
    cw = (sub + HALO) // 16
    lds = sub * 8 * w + nb_alloc * 4 + (nb_alloc + 4) * 4 + cw * 4 + cw * 2 + 8 + 64
    return nb_alloc <= 4 * ST_THREADS and lds <= 160 * 1024


# =========================================================================== planted cases
def nbuckets(k, text):
    return max(1, -(-(len(text) - k + 1) // MEAN[words(k)])) if len(text) >= k else 1


def profile(k, text, nb=None):
    """{bucket: (keys, distinct keys, fullest fine bin, keys in fine bins with more than one distinct key)} of the
    text's non-empty buckets, from the ORACLE's keys and exact counters."""
    nb = nb or nbuckets(k, text)
    keys, counts = CO.count(text, k, cs=BIG).arrays()
    mixed = mix_np(k, keys)
    slot = slot_np(k, mixed, nb).astype(np.int64)
    fine = fine_bin_np(k, mixed, nb, FINE_BITS).astype(np.int64)
    bins, inv = np.unique((slot << FINE_BITS) | fine, return_inverse=True)      # the occupied (bucket, fine bin) pairs
    raw = np.bincount(inv, weights=counts).astype(np.int64)
    dist = np.bincount(inv)
    slots, of = np.unique(bins >> FINE_BITS, return_inverse=True)
    fullest = np.zeros(slots.shape[0], dtype=np.int64)
    np.maximum.at(fullest, of, raw)
    n = np.bincount(of, weights=raw).astype(np.int64)
    d = np.bincount(of, weights=dist).astype(np.int64)
    listed = np.bincount(of, weights=raw * (dist > 1), minlength=slots.shape[0]).astype(np.int64)
    return {int(b): (int(n[i]), int(d[i]), int(fullest[i]), int(listed[i])) for i, b in enumerate(slots)}


def min_nb(k, nwords, spare=2):
    """Buckets a text of `nwords` planted words needs so that the N tail is not negative."""
    return -(-(nwords * (k + 1) + k) // MEAN[words(k)]) + spare


@functools.lru_cache(maxsize=None)
def sizes_case(k):
    """Buckets of 0 (the first, a middle one, the last), 1, cap - 1 and cap keys."""
    cap = CAP[words(k)]
    p = Planted(k, max(8, min_nb(k, 2 * cap)), 100 + k)
    p.add(1, None, 1)
    p.add(2, None, cap - 1)
    p.add(4, None, cap)
    return p.text(), {1: (1, 1), 2: (cap - 1, cap - 1), 4: (cap, cap)}


@functools.lru_cache(maxsize=None)
def fold_case(k, distinct, raw, slot_of_nb=(3, None)):
    """One bucket of `raw` keys, `distinct` of them distinct: key 0 is written 300 times (above the default counter
    ceiling), the others once or twice (copies of a key are shuffled over the text, so over the fold's chunks)."""
    p = Planted(k, max(8, min_nb(k, raw)), 200 + k + distinct)
    mult = np.ones(distinct, dtype=np.int64)
    if raw > distinct:
        mult[0] = min(300, raw - distinct + 1)
        extra = raw - int(mult.sum())
        step = 0
        while extra > 0:                       # 2, then 3, ... copies of the keys after the first
            n = min(extra, distinct - 1)
            mult[1:1 + n] += 1
            extra -= n
            step += 1
    assert int(mult.sum()) == raw
    p.add(slot_of_nb[0], None, distinct, mult)
    return p.text(), {slot_of_nb[0]: (raw, distinct)}


def fold_cases(k):
    """name -> (distinct, raw, retries expected: a number, or None where the order of arrival decides)."""
    w = words(k)
    cap, cp = CAP[w], capp(w)
    return {
        "few_distinct": (100, cap + 1, 0),             # the fold, nothing near its limit
        "cap+1_distinct": (cap + 1, cap + 1, 1),       # more distinct keys than pairs fit: one re-plan
        "capp-1": (cp - 1, cap + 700, 0),              # acc never reaches capp
        "capp": (cp, cap + 700, None),                 # fails iff the last new key arrives before the last chunk
        "capp+1": (cp + 1, cap + 700, 1),
    }


TIER_P = 1024      # the power of two of the bitonic cases (n = P - 1, P, P + 1 fit both capacities)


@functools.lru_cache(maxsize=None)
def tiers_case(k):
    """One text, one bucket per sort tier.  Returns (text, {bucket: (what, keys, distinct, fullest bin)})."""
    nwords = 64 + 65 + 66 + 3 * 200 + 960 + 50 + 1120 + 3 * (TIER_P + 1)
    nb = max(40, min_nb(k, nwords))
    p = Planted(k, nb, 300 + k)
    want = {}
    # fullest bin exactly at and one above KH_FINE_LIMIT
    p.add(0, 100, 64)
    p.add(0, None, 200, avoid=(100,))
    want[0] = ("bin64", 264, 264, 64)
    p.add(5, 8191, 65)
    p.add(5, None, 200, avoid=(8191,))
    want[5] = ("bin65", 265, 265, 65)
    # 65 copies of one key and one other key in one bin
    p.add(9, 7, 2, np.array([65, 1]))
    p.add(9, None, 200, avoid=(7,))
    want[9] = ("copies65+1", 266, 202, 66)
    # bins of 16 distinct keys: 60 of them stay on the work list (both passes of IT = 2), 70 exceed it
    for j in range(60):
        p.add(17, 64 + 131 * j, 16)
    want[17] = ("repair960", 960, 960, 16)
    for j in range(70):
        p.add(nb - 1, 3 + 117 * j, 16)
    want[nb - 1] = ("worklist1120", 1120, 1120, 16)
    # the bitonic network at a power of two, one below and one above (a bin of 65 sends the bucket there)
    for b, n in ((21, TIER_P - 1), (22, TIER_P), (23, TIER_P + 1)):
        p.add(b, 4096, 65)
        p.add(b, None, n - 65, avoid=(4096,))
        want[b] = ("bitonic%d" % n, n, n, 65)
    return p.text(), want


FILTERS = ((2, 0xFFFFFFFF), (1, 1), (2, 2), (3, 5))
FILTER_NB = 640
FILTER_TYPES = ((1, 1, 1), (2, 2, 2), (1, 2, 3, 4, 5, 6), (3, 4, 5), ())     # multiplicities of bucket b's keys, b % 5


@functools.lru_cache(maxsize=None)
def filters_case(k):
    """640 buckets (more than one look-back window of 512) whose kept count differs from their run count: under each
    of FILTERS some buckets keep nothing, some everything, some a part, and every fifth bucket is empty."""
    p = Planted(k, FILTER_NB, 400 + k)
    for b in range(FILTER_NB):
        m = FILTER_TYPES[b % 5]
        if m:
            p.add(b, None, len(m), np.array(m))
    return p.text()


@functools.lru_cache(maxsize=None)
def replan_direct_case(k):
    """One sequence of real random DNA (every bucket full) with `extra` planted keys in one bucket: that bucket holds
    more distinct keys than pairs fit, the re-plan's mean / 4 gives more than 4096 buckets and so the direct scatter."""
    w = words(k)
    nb = 1217 if w == 1 else 1030
    extra = 1200 if w == 1 else 700
    p = Planted(k, nb, 500 + k)
    p.add(611, None, extra)
    body = nb * MEAN[w] - extra * (k + 1) - 1000
    return p.text(head=random_dna_np(p.rng, body) + b"N"), nb, 611, extra


# --------------------------------------------------------------------------- CPU proofs of the constructions
PLANT_K = (31, 41)            # one one-word and one two-word k
TIER_K = (31, 32, 41, 63)     # the sort-tier cases also at the widest key of each form


@pytest.mark.parametrize("k", (21, 31, 32, 41, 63))
def test_planted_keys_land_where_chosen(k):
    nb = 36 if k <= 32 else 80
    p = Planted(k, nb, k)
    p.add(17, 5, 65)
    p.add(17, 4000, 1200)
    text = p.text()
    assert nbuckets(k, text) == nb
    keys, counts = CO.count(text, k, cs=BIG).arrays()
    assert keys.shape[0] == 1265 and (counts == 1).all()
    assert (key_view(keys) == np.sort(key_view(p.keys))).all()         # canonical as written
    assert profile(k, text) == {17: (1265, 1265, 1200, 1265)}
    rows = codes_text(k, p.keys)
    assert [len(wd) for wd in text.rstrip(b"N").split(b"N")] == [k] * 1265 and rows.shape == (1265, k)


@pytest.mark.parametrize("k", PLANT_K)
def test_sizes_case_preconditions(k):
    text, want = sizes_case(k)
    prof = profile(k, text)
    assert {b: v[:2] for b, v in prof.items()} == want
    assert nbuckets(k, text) > 5 and 0 not in prof and 3 not in prof and nbuckets(k, text) - 1 not in prof
    assert max(v[2] for v in prof.values()) <= FINE_LIMIT


@pytest.mark.parametrize("k", PLANT_K)
def test_fold_case_preconditions(k):
    w = words(k)
    for name, (distinct, raw, _) in fold_cases(k).items():
        text, want = fold_case(k, distinct, raw)
        prof = profile(k, text)
        assert {b: v[:2] for b, v in prof.items()} == want, name
        assert raw > CAP[w]                                              # the oversize path
        _, counts = CO.count(text, k, cs=BIG).arrays()
        if distinct < raw:
            assert counts.max() > 255 and (counts > 1).sum() > 50 and counts.min() < 255   # the ceiling, and chunk sums
    assert fold_cases(k)["capp+1"][0] == capp(w) + 1 and fold_cases(k)["capp-1"][0] == capp(w) - 1


@pytest.mark.parametrize("k", TIER_K)
def test_tiers_case_preconditions(k):
    text, want = tiers_case(k)
    prof = profile(k, text)
    assert set(prof) == set(want)
    for b, (what, n, distinct, fullest) in want.items():
        assert prof[b][:3] == (n, distinct, fullest), (what, prof[b])
        assert n <= CAP[words(k)]
    assert want[0][3] == FINE_LIMIT and want[5][3] == FINE_LIMIT + 1
    # the repair tier: every listed key fits the work list and both of its passes run; one bin more would not fit
    b_rep, b_wl = 17, nbuckets(k, text) - 1
    assert SORT_THREADS < prof[b_rep][3] <= WORKLIST and prof[b_rep][3] == 960
    # 70 bins of 16 shuffled distinct keys: a bin arrives sorted with probability 1 / 16!, so 1120 keys are listed
    assert prof[b_wl][3] == 1120 > WORKLIST and prof[b_wl][2] <= FINE_LIMIT
    for b, n in ((21, TIER_P - 1), (22, TIER_P), (23, TIER_P + 1)):
        assert prof[b][0] == n and prof[b][2] > FINE_LIMIT
    assert TIER_P & (TIER_P - 1) == 0


@pytest.mark.parametrize("k", PLANT_K)
def test_filters_case_preconditions(k):
    text = filters_case(k)
    assert nbuckets(k, text) == FILTER_NB >= 600
    prof = profile(k, text)
    assert sorted(prof) == [b for b in range(FILTER_NB) if b % 5 != 4]
    keys, counts = CO.count(text, k, cs=BIG).arrays()
    slot = slot_np(k, mix_np(k, keys), FILTER_NB).astype(np.int64)
    for ci, cx in FILTERS:
        kept = (counts >= ci) & (counts <= cx)
        per = np.bincount(slot, weights=kept, minlength=FILTER_NB).astype(np.int64)
        runs = np.bincount(slot, minlength=FILTER_NB)
        nothing, everything = (per == 0) & (runs > 0), (per == runs) & (runs > 0)
        part = (per > 0) & (per < runs)
        assert nothing.sum() >= 100 and everything.sum() >= 100 and part.sum() >= 100, (ci, cx)


@pytest.mark.parametrize("k", PLANT_K)
def test_replan_direct_case_preconditions(k):
    w = words(k)
    text, nb, b, extra = replan_direct_case(k)
    npos = len(text) - k + 1
    assert nbuckets(k, text) == nb and staged(w, nb)
    prof = profile(k, text)
    n, distinct = prof[b][:2]
    assert n > CAP[w] and distinct > capp(w)                             # cannot be folded: KH_ERR_CAPACITY
    # every other bucket is within capacity, so the one re-plan is this bucket's
    assert sorted(v[0] for v in prof.values())[-2] <= CAP[w] and len(prof) == nb
    nb2 = -(-npos // (MEAN[w] // 4))
    assert 4 * ST_THREADS < nb2 <= MAX_BUCKETS_PER_SEG and not staged(w, nb2)   # the direct scatter, unforced
    assert max(v[0] for v in profile(k, text, nb2).values()) <= CAP[w]  # and the second plan holds


# =========================================================================== GPU
@pytest.fixture(scope="module")
def eng():
    from khoice_amd import build as kbuild
    from khoice_amd import engine as E
    if not os.environ.get("KHOICE_HIP_LIB"):
        kbuild.build_library()
    e = E.Engine(0)
    yield e
    e.close()


def oracle_all(seqs, k, **kw):
    with ThreadPoolExecutor(8) as ex:
        return list(ex.map(lambda s: CO.count(s, k, **kw), seqs))


def same_db(kset, want, what, plain=False):
    keys, counts = kset.download_sorted()
    okeys, ocounts = want.arrays()
    assert keys.shape == okeys.shape, (what, keys.shape, okeys.shape)
    assert (keys == okeys).all(), what
    assert (counts == (1 if plain else ocounts)).all(), what


def build_checked(eng, seqs, k, what, retries=0, ci=1, cx=0xFFFFFFFF):
    """The batch in the three forms (exact counters, the default ceiling of 255, no counters), each against the oracle;
    `retries`: re-plans each build must take (None: not pinned)."""
    for form in ("exact", "default", "plain"):
        cs = BIG if form == "exact" else 255
        want = oracle_all(seqs, k, ci=ci, cx=cx, cs=cs)
        r0 = eng.stats()["retries"]
        got = eng.build_batch(seqs, k, ci=ci, cx=cx, cs=cs, with_counts=form != "plain")
        r = eng.stats()["retries"] - r0
        assert retries is None or r == retries, (what, form, r)
        assert r <= 1
        for i, (g, w) in enumerate(zip(got, want)):
            same_db(g, w, (what, form, i), plain=form == "plain")


# --------------------------------------------------------------------------- 1. planted keys
@pytest.mark.gpu
@pytest.mark.parametrize("k", PLANT_K)
def test_bucket_sizes(eng, k):
    build_checked(eng, [sizes_case(k)[0]], k, "sizes")


@pytest.mark.gpu
@pytest.mark.parametrize("k", PLANT_K)
def test_oversize_fold_and_replan(eng, k):
    for name, (distinct, raw, retries) in fold_cases(k).items():
        build_checked(eng, [fold_case(k, distinct, raw)[0]], k, name, retries=retries)


@pytest.mark.gpu
@pytest.mark.parametrize("k", TIER_K)
def test_sort_tiers(eng, k):
    build_checked(eng, [tiers_case(k)[0]], k, "tiers")


@pytest.mark.gpu
@pytest.mark.parametrize("k", PLANT_K)
def test_filters_drop_runs(eng, k):
    for ci, cx in FILTERS:
        build_checked(eng, [filters_case(k)], k, ("filters", ci, cx), ci=ci, cx=cx)


@pytest.mark.gpu
@pytest.mark.parametrize("k", PLANT_K)
def test_replan_reaches_direct_scatter(eng, k, monkeypatch):
    monkeypatch.delenv("KHOICE_DIRECT_SCATTER", raising=False)
    monkeypatch.delenv("KHOICE_TILE_POS", raising=False)
    build_checked(eng, [replan_direct_case(k)[0]], k, "replan_direct", retries=1)


# --------------------------------------------------------------------------- 2. extraction edges
LEN_K = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)
NSWEEP_K = (21, 32, 33, 41, 64)
LEN_BOUNDS = (8, 16, 32, SUBTILE, 2 * SUBTILE, 4 * SUBTILE, 8 * SUBTILE)     # thread ranges of 8 / 16 / 32 positions, the
N_ANCHORS = (0, 256, SUBTILE, 2 * SUBTILE, 4 * SUBTILE, 8 * SUBTILE)         # sub-tile, the staging rounds, the tiles


def length_edge_seqs(k, seed=7):
    """ACGT sequences whose number of k-mer positions is each boundary -2 .. +2."""
    rng = np.random.default_rng(seed + k)
    return [random_dna_np(rng, b + d + k - 1) for b in LEN_BOUNDS for d in range(-2, 3)]


def n_sweep_seqs(k, seed=11):
    """Per offset d in [-k - 2, k + 2] and run length in (1, 2, k): one ACGT sequence with that run of N at B + d for
    every anchor B (the anchors are far more than k apart, so each run meets its boundary alone).  The offsets cover
    every residue of the 8-, 16- and 32-position thread ranges and of the 16-base code word."""
    rng = np.random.default_rng(seed + k)
    length = N_ANCHORS[-1] + 3 * k + 40
    out = []
    for d in range(-k - 2, k + 3):
        for run in (1, 2, k):
            a = np.frombuffer(random_dna_np(rng, length), dtype=np.uint8).copy()
            for anchor in N_ANCHORS:
                if anchor + d >= 0:
                    a[anchor + d:anchor + d + run] = ord("N")
            out.append(a.tobytes())
    return out


def test_extraction_inputs_preconditions():
    for k in NSWEEP_K:
        seqs = n_sweep_seqs(k)
        assert len(seqs) == 3 * (2 * k + 5) and 2 * k + 5 >= 32
        assert {s.count(b"N") for s in seqs[:3]} == {len(N_ANCHORS) - 1, 2 * (len(N_ANCHORS) - 1), k * (len(N_ANCHORS) - 1)}
        last = seqs[-1]                                                   # d = k + 2, run = k
        assert all(last[b + k + 2:b + 2 * k + 2] == b"N" * k for b in N_ANCHORS) and len(last) > N_ANCHORS[-1] + 2 * k + 2
    for k in LEN_K:
        npos = [len(s) - k + 1 for s in length_edge_seqs(k)]
        assert npos == [b + d for b in LEN_BOUNDS for d in range(-2, 3)] and min(npos) > 0


def digest(kset):
    keys, counts = kset.download()          # storage order (sorted by mixed key): the same for every form of the build
    return hashlib.blake2b(keys.tobytes() + counts.tobytes(), digest_size=16).digest(), keys.shape[0]


@pytest.mark.gpu
@pytest.mark.parametrize("k", sorted(set(LEN_K) | set(NSWEEP_K)))
def test_extraction_edges(eng, k, monkeypatch):
    """Every sequence against the oracle in the default form; then the same batch through the direct scatter, every
    tile size, and a second engine that takes its buckets by ticket: each set identical to the first form's."""
    from khoice_amd import engine as E
    seqs = (length_edge_seqs(k) if k in LEN_K else []) + (n_sweep_seqs(k) if k in NSWEEP_K else [])
    for name in ("KHOICE_DIRECT_SCATTER", "KHOICE_TILE_POS", "KHOICE_TICKETS", "KHOICE_MAX_SEG_POS"):
        monkeypatch.delenv(name, raising=False)
    want = oracle_all(seqs, k, cs=BIG)
    got = eng.build_batch(seqs, k, cs=BIG)
    base = []
    for i, (g, w) in enumerate(zip(got, want)):
        same_db(g, w, ("default", i, len(seqs[i])))
        base.append(digest(g))
    del got, want
    forms = [{"KHOICE_DIRECT_SCATTER": "1"}, {"KHOICE_TILE_POS": str(4 * SUBTILE)}, {"KHOICE_TILE_POS": str(8 * SUBTILE)},
             {"KHOICE_TILE_POS": str(8 * SUBTILE), "KHOICE_DIRECT_SCATTER": "1"}]
    for env in forms:
        for name, v in env.items():
            monkeypatch.setenv(name, v)
        got = eng.build_batch(seqs, k, cs=BIG)
        for name in env:
            monkeypatch.delenv(name)
        for i, g in enumerate(got):
            assert digest(g) == base[i], (env, i, len(seqs[i]))
        del got
    monkeypatch.setenv("KHOICE_TICKETS", "1")
    with E.Engine(0) as e2:
        monkeypatch.delenv("KHOICE_TICKETS")
        for env in ({}, {"KHOICE_DIRECT_SCATTER": "1"}):
            for name, v in env.items():
                monkeypatch.setenv(name, v)
            got = e2.build_batch(seqs, k, cs=BIG)
            for name in env:
                monkeypatch.delenv(name)
            for i, g in enumerate(got):
                assert digest(g) == base[i], ("tickets", env, i, len(seqs[i]))
            del got
        assert e2.stats()["order_fallbacks"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("k", (21, 31, 41, 64))
def test_device_inputs_at_every_alignment(eng, k, monkeypatch):
    """(ptr, len) inputs inside one device tensor at byte offsets 0, 1, 15 and 16 from an aligned base, each followed by
    valid ACGT bytes: reading past a sequence's end stays inside the allocation and shows as extra k-mers."""
    import torch
    seqs = length_edge_seqs(k, seed=23) + n_sweep_seqs(k if k in NSWEEP_K else 21, seed=29)[::17]
    if k not in NSWEEP_K:
        seqs = [s for s in seqs if len(s) >= k]
    rng = np.random.default_rng(31 + k)
    offs, at, cursor = (0, 1, 15, 16), [], 256
    for i, s in enumerate(seqs):
        base = (cursor + 255) & ~255
        at.append(base + offs[i % 4])
        cursor = at[-1] + len(s) + 3 * k
    host = np.frombuffer(random_dna_np(rng, cursor + 4096), dtype=np.uint8).copy()
    for s, a in zip(seqs, at):
        host[a:a + len(s)] = np.frombuffer(s, dtype=np.uint8)
    dev = torch.from_numpy(host).to("cuda:0")
    torch.cuda.synchronize()
    shift = (-dev.data_ptr()) & 255                       # offsets are counted from a 256-byte aligned address
    if shift:
        dev2 = torch.empty(host.shape[0] + 256, dtype=torch.uint8, device="cuda:0")
        shift = (-dev2.data_ptr()) & 255
        dev2[shift:shift + host.shape[0]] = dev
        dev = dev2
        torch.cuda.synchronize()
    ptrs = [(dev.data_ptr() + shift + a, len(s)) for s, a in zip(seqs, at)]
    assert {p & 15 for p, _ in ptrs} == {0, 1, 15}
    want = oracle_all(seqs, k, cs=BIG)
    for env in ({}, {"KHOICE_DIRECT_SCATTER": "1"}):
        for name, v in env.items():
            monkeypatch.setenv(name, v)
        got = eng.build_batch(ptrs, k, cs=BIG)
        for name in env:
            monkeypatch.delenv(name)
        for i, (g, w) in enumerate(zip(got, want)):
            same_db(g, w, ("device", env, i, len(seqs[i]), ptrs[i][0] & 15))
    eng.sync()
    del dev


@pytest.mark.gpu
@pytest.mark.parametrize("k", (21, 41))
def test_chunk_edges(eng, k, monkeypatch):
    """Forced chunking at and around a tile multiple, on sequences whose N sit at the chunk edges."""
    rng = np.random.default_rng(41 + k)
    for chunk in (MIN_TILE - 1, MIN_TILE, MIN_TILE + 1, 2 * MIN_TILE):
        seqs = []
        for d in (-k - 1, -k, -k + 1, -1, 0, 1, k - 2, k - 1, k):
            a = np.frombuffer(random_dna_np(rng, 3 * chunk + 1000 + 7 * (d + k)), dtype=np.uint8).copy()
            for c in (1, 2, 3):
                a[c * chunk + d] = ord("N")
            seqs.append(a.tobytes())
        seqs.append(random_dna_np(rng, 2 * chunk + k - 1))           # ends exactly with its second chunk
        seqs.append(random_dna_np(rng, 2 * chunk + k))               # a last chunk of one position
        seqs.append(random_dna_np(rng, 500))                         # not chunked
        for form in ("exact", "default", "plain"):
            cs = BIG if form == "exact" else 255
            want = oracle_all(seqs, k, cs=cs)
            monkeypatch.setenv("KHOICE_MAX_SEG_POS", str(chunk))
            got = eng.build_batch(seqs, k, cs=cs, with_counts=form != "plain")
            monkeypatch.delenv("KHOICE_MAX_SEG_POS")
            for i, (g, w) in enumerate(zip(got, want)):
                same_db(g, w, ("chunk", chunk, form, i), plain=form == "plain")


# --------------------------------------------------------------------------- 3. bucket-plan edges
def short_seqs(n, k, seed):
    """n sequences of 0 .. 200 bases (most 40 .. 200; empty ones, shorter-than-k ones and a few N among them): one
    bucket each."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(40, 201, size=n)
    lens[rng.integers(0, n, size=n // 50)] = 0
    lens[rng.integers(0, n, size=n // 50)] = rng.integers(1, k, size=n // 50) if k > 1 else 0
    buf = np.frombuffer(random_dna_np(rng, int(lens.sum()) + 1), dtype=np.uint8).copy()
    buf[rng.integers(0, buf.shape[0], size=n // 10)] = ord("N")
    ends = np.cumsum(lens)
    return [buf[e - ln:e].tobytes() for e, ln in zip(ends, lens)]


def test_short_seqs_preconditions():
    for n in (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE + 1):
        seqs = short_seqs(n, 31, n)
        assert len(seqs) == n and sum(nbuckets(31, s) for s in seqs) == n
        assert sum(1 for s in seqs if not s) > 10 and sum(1 for s in seqs if 0 < len(s) < 31) > 10
        assert max(len(s) for s in seqs) <= 200


@pytest.mark.gpu
@pytest.mark.parametrize("n,k", [(SCAN_TILE - 1, 31), (SCAN_TILE, 31), (SCAN_TILE + 1, 31), (2 * SCAN_TILE + 1, 31),
                                 (SCAN_TILE + 1, 41)])
def test_total_bucket_counts(eng, n, k):
    """The exclusive scan of the bucket totals at and across its 4096-entry tiles: n one-bucket sequences."""
    seqs = short_seqs(n, k, n + k)
    want = oracle_all(seqs, k)
    got = eng.build_batch(seqs, k)
    for i, (g, w) in enumerate(zip(got, want)):
        same_db(g, w, ("buckets", n, i))
    plain = eng.build_batch(seqs, k, with_counts=False)
    for i, (g, w) in enumerate(zip(plain, want)):
        assert len(g) == len(w), ("buckets plain", n, i)


def depth_seqs(nseq, k, seed):
    """nseq sequences of random DNA with 1, 2, 7 and 40 buckets in turn (the last position of a depth, or one past it)."""
    rng = np.random.default_rng(seed)
    mean = MEAN[words(k)]
    out = []
    for i in range(nseq):
        depth = (1, 2, 7, 40)[(i + i // 4) % 4]
        npos = depth * mean - int(rng.integers(0, 2)) * int(rng.integers(0, mean))
        out.append(random_dna_np(rng, npos + k - 1, b"ACGTN" if i % 9 == 0 else b"ACGT"))
    return out


def test_depth_seqs_preconditions():
    for nseq in (63, 64, 65, 129):
        depths = [nbuckets(31, s) for s in depth_seqs(nseq, 31, nseq)]
        assert set(depths) == {1, 2, 7, 40} and len(depths) == nseq
        for s0 in range(0, nseq, 64):                                   # every interleave group mixes the depths
            assert len(set(depths[s0:s0 + 64])) >= (1 if nseq - s0 < 4 else 4)


@pytest.mark.gpu
@pytest.mark.parametrize("nseq,k", [(63, 31), (64, 31), (65, 31), (129, 31), (65, 41)])
def test_segment_interleave(eng, nseq, k):
    """The 64-segment start-order interleave and the per-segment look-back chains, buckets of mixed depth."""
    seqs = depth_seqs(nseq, k, nseq)
    want = oracle_all(seqs, k)
    got = eng.build_batch(seqs, k)
    for i, (g, w) in enumerate(zip(got, want)):
        same_db(g, w, ("interleave", nseq, i))


@pytest.mark.gpu
@pytest.mark.parametrize("k", PLANT_K)
def test_tile_counts(eng, k, monkeypatch):
    """Segments of 1, 7, 8, 9 and 10 tiles (k_col_*'s 8 tile groups: fewer tiles than groups, as many, more), and a
    5 Mbp sequence cut into some 300 tiles."""
    rng = np.random.default_rng(53 + k)
    seqs = [random_dna_np(rng, t * MIN_TILE + d + k - 1) for t, d in ((1, 0), (7, 0), (8, 0), (9, 0), (9, 1), (1, -3), (8, -1))]
    seqs.append(random_dna_np(rng, 5_000_000))
    monkeypatch.setenv("KHOICE_TILE_POS", str(MIN_TILE))
    want = oracle_all(seqs, k)
    got = eng.build_batch(seqs, k)
    for i, (g, w) in enumerate(zip(got, want)):
        same_db(g, w, ("tiles", i))


@pytest.mark.gpu
@pytest.mark.parametrize("k", PLANT_K)
def test_segment_bucket_counts(eng, k):
    """Segments of 1, 63, 64 and 65 buckets, to the last position and one past it."""
    rng = np.random.default_rng(59 + k)
    mean = MEAN[words(k)]
    seqs = [random_dna_np(rng, nb * mean + d + k - 1) for nb in (1, 63, 64, 65) for d in (0, 1)]
    assert [nbuckets(k, s) for s in seqs] == [1, 2, 63, 64, 64, 65, 65, 66]
    want = oracle_all(seqs, k)
    got = eng.build_batch(seqs, k)
    for i, (g, w) in enumerate(zip(got, want)):
        same_db(g, w, ("segment buckets", i))


def test_staging_limits():
    """Where pass B changes form: up to 3072 buckets a thread of the staged form scans 3 entries, above 4 (per = 4),
    and the LDS bound ends the staged form before 4096 buckets."""
    for w in (1, 2):
        assert staged(w, 3073) and not staged(w, 4096)
    assert -(-3073 // ST_THREADS) == 4 and -(-3072 // ST_THREADS) == 3


@pytest.mark.gpu
def test_segments_at_the_staging_limit(eng, monkeypatch):
    """One segment of 3073 buckets (the staged form at four scan entries per thread) and one of 4096 (the most a
    sequence has before it is chunked; the direct form), two-word keys."""
    k = 41
    monkeypatch.delenv("KHOICE_DIRECT_SCATTER", raising=False)
    rng = np.random.default_rng(61)
    seqs = [random_dna_np(rng, nb * MEAN[2] + k - 1) for nb in (3073, MAX_BUCKETS_PER_SEG // 4)]
    assert [nbuckets(k, s) for s in seqs] == [3073, 4096]
    want = oracle_all(seqs, k)
    for s, w in zip(seqs, want):                    # one at a time: each segment alone decides the form of pass B
        same_db(eng.build(s, k), w, ("staging limit", len(s)))


# --------------------------------------------------------------------------- 4. grid mode (key-array form of exp1)
GRID_NB = 100
GRID_GENOMES, GRID_GROUP_OF = 6, [0, 0, 0, 1, 1, 1]


@functools.lru_cache(maxsize=None)
def grid_case(k, kind):
    """Six genomes in two groups, every genome GRID_NB buckets of planted keys.  The genomes draw from shared family
    pools, so keys repeat across genomes and groups.  Returns (seqs, planted fine bins {bucket: bins})."""
    w = words(k)
    cap = CAP[w]
    rng = np.random.default_rng(600 + k)
    pool = Planted(k, GRID_NB, 700 + k)
    fam, bins = {}, {}

    def family(name, b, f, n):
        fam[name] = pool.add(b, f, n)
        bins.setdefault(b, set()).add(f)
    # bucket 3: fine bins of 3, 16 and 64 distinct keys, in two sub-ranges of the middle: the sub-ranges before,
    # between and behind them stay empty (grid_bucket's off[])
    family("bin3", 3, 2500, 5)
    family("bin16", 3, 2501, 24)
    family("bin64", 3, 5500, 80)
    # bucket 0: keys in the first fine bin only; the last bucket: in the last only; bucket 20: spread
    family("first", 0, 0, 20)
    family("last", GRID_NB - 1, (1 << FINE_BITS) - 1, 20)
    spread = pool.add(20, None, 600)
    if kind == "oversize":
        family("dup_a", 11, 2000, 25)          # 50 distinct keys in two fine bins, more than cap copies in all:
        family("dup_b", 11, 7000, 25)          # k_grid_oversize folds them; empty sub-ranges before, between, behind
    if kind == "too_many":
        over = pool.add(11, None, cap + 1)     # more distinct keys than fit LDS: KH_ERR_CAPACITY, the general path
    seqs = []
    for g in range(GRID_GENOMES):
        keys, mult = [], []

        def take(a, n, m=1):
            sel = a[rng.permutation(a.shape[0])[:n]]
            keys.append(sel)
            mult.append(np.broadcast_to(np.asarray(m, dtype=np.int64), (sel.shape[0],)))
        take(fam["bin3"], 3, np.array([1, 2, 1]))
        take(fam["bin16"], 16, 1 + (np.arange(16) % 3 == 0))
        take(fam["bin64"], 64)
        take(fam["first"], 12)
        take(fam["last"], 12, 2)
        take(spread, 400)
        if kind == "oversize" and g in (1, 4):
            take(fam["dup_a"], 25, np.full(25, (cap + 1000) // 50))
            take(fam["dup_b"], 25, np.full(25, (cap + 1000) // 50))
        if kind == "oversize" and g in (0, 3):     # the same keys where the bucket fits: grid_bucket's sub-ranges
            take(fam["dup_a"], 10)
            take(fam["dup_b"], 10, 2)
        if kind == "too_many" and g == 2:
            take(over, cap + 1)
        keys, mult = np.concatenate(keys), np.concatenate(mult)
        seqs.append(planted_text(k, keys, mult, GRID_NB * MEAN[w], rng))
    return tuple(seqs), bins


GRID_KINDS = ("bins", "oversize", "too_many")


@pytest.mark.parametrize("k", PLANT_K)
def test_grid_case_preconditions(k):
    w = words(k)
    for kind in GRID_KINDS:
        seqs, bins = grid_case(k, kind)
        assert [nbuckets(k, s) for s in seqs] == [GRID_NB] * GRID_GENOMES
        profs = [profile(k, s) for s in seqs]
        for g, prof in enumerate(profs):
            assert set(prof) >= {0, 3, 20, GRID_NB - 1}
            assert prof[3][1] == 3 + 16 + 64 and prof[3][2] == 64 and prof[3][0] == 4 + 22 + 64
            over = [b for b, v in prof.items() if v[0] > CAP[w]]
            if kind == "oversize" and g in (1, 4):
                assert over == [11] and prof[11][1] == 50
            elif kind == "oversize" and g in (0, 3):
                assert not over and prof[11][:2] == (30, 20)
            elif kind == "too_many" and g == 2:
                assert over == [11] and prof[11][1] == CAP[w] + 1
            else:
                assert not over
        # keys repeat across genomes and groups
        sets = [set(key_view(CO.count(s, k).arrays()[0]).tolist()) for s in seqs]
        assert len(sets[0] & sets[1]) > 100 and len(sets[0] & sets[4]) > 100 and sets[0] != sets[1]
        # empty sub-ranges before, between and behind the keys of bucket 3, in both forms of the union
        for hash_form in (False, True):
            s_ranges = grid_sub_ranges(k, GRID_GENOMES, 3, hash_form)
            for b in (3, 11) if kind == "oversize" else (3,):
                subs = sorted({(f * s_ranges) >> FINE_BITS for f in bins[b]})
                assert len(subs) == 2 and subs[0] > 0 and subs[1] - subs[0] > 1 and subs[1] < s_ranges - 1, (s_ranges, subs)


@functools.lru_cache(maxsize=None)
def grid_unequal_case(k):
    rng = np.random.default_rng(800 + k)
    seqs = [random_dna_np(rng, 40), random_dna_np(rng, 3_000_000), random_dna_np(rng, 100_000), b"", random_dna_np(rng, k)]
    seqs.append(seqs[1][1_000_000:1_200_000])                          # shares 200 kbp with the long genome
    return tuple(seqs), [0, 0, 1, 1, 2, 2]


def exp1_checked(eng, seqs, group_of, k, what, retries):
    """The oracle's histograms and distinct counts at two (cs, hist_len); the union kernel must have launched, and the
    retry counter moved exactly when `retries` says so."""
    for cs, hl in ((5000, 80), (2, 5)):
        want = CO.exp1(list(seqs), group_of, k, cs=cs, hist_len=hl)
        eng.profile(True)
        st0 = eng.stats()
        print("exp1_checked:", what, cs, hl)
        got = eng.exp1_run(list(seqs), group_of, k, cs=cs, hist_len=hl)
        st1 = eng.stats()
        eng.profile(False)
        for f in ("within_hist", "across_hist", "distinct_per_seq"):
            assert got[f].shape == want[f].shape and (got[f] == want[f]).all(), (what, cs, f)
        moved = st1["retries"] - st0["retries"]
        assert (moved > 0) == retries, (what, moved)
        assert st1["kernels"]["union_tagged"]["launches"] > st0["kernels"]["union_tagged"]["launches"] or retries, what
        assert st1["kernels"]["skm_union"]["launches"] == st0["kernels"]["skm_union"]["launches"], what


@pytest.mark.gpu
@pytest.mark.parametrize("no_hash", (False, True))
@pytest.mark.parametrize("k", PLANT_K)
def test_grid_mode_planted(eng, k, no_hash, monkeypatch):
    monkeypatch.setenv("KHOICE_NO_SKM", "1")
    if no_hash:
        monkeypatch.setenv("KHOICE_NO_UNION_HASH", "1")
    else:
        monkeypatch.delenv("KHOICE_NO_UNION_HASH", raising=False)
    for kind in GRID_KINDS:
        seqs, _ = grid_case(k, kind)
        exp1_checked(eng, seqs, GRID_GROUP_OF, k, (kind, no_hash), retries=kind == "too_many")


@pytest.mark.gpu
@pytest.mark.parametrize("no_hash", (False, True))
@pytest.mark.parametrize("k", PLANT_K)
def test_grid_mode_tiny_beside_long(eng, k, no_hash, monkeypatch):
    """A 40-base genome, an empty one and one of k bases beside a 3 Mbp one: a grid of nearly empty buckets."""
    monkeypatch.setenv("KHOICE_NO_SKM", "1")
    if no_hash:
        monkeypatch.setenv("KHOICE_NO_UNION_HASH", "1")
    else:
        monkeypatch.delenv("KHOICE_NO_UNION_HASH", raising=False)
    seqs, group_of = grid_unequal_case(k)
    exp1_checked(eng, seqs, group_of, k, ("unequal", no_hash), retries=False)
