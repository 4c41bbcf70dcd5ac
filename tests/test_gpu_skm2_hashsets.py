"""The LDS hash sets of the two-word forms of the fused exp-1 path (k = 33 .. 63), at every probe tier and exit, bit-exact
against the C restatement (oracle.c_oracle.exp1).  The twin of tests/test_gpu_skm_hashsets.py, which pins the one-word
forms.

k_skm2_union (khoice_amd/csrc/kh_skm2.hip) and k_skm_big<SkmBig2> (kh_skm_device.h) hold the same tiers as the
one-word kernels: KH_TUNE_SKM_FULL_ROUNDS probes in the main table from the key's home, eight in a small second table
with an independent hash, then the main table again from home + 4 to its end, whose last exit raises
KH_ERR_CAPACITY; slots of more than T instances are taken in R rounds of key subsets.  What differs is what such a test
depends on: the union's main table has 1792 entries (home (H * 1792) >> 32, wrap by a compare at 1791) and its second
table 32; a slot holds at most 448 records and 2048 chunks, over four index passes of 512 threads; k_skm_big has
2048 + 64 entries and rounds of 1536 instances; an entry is claimed on the LOW word and the winner publishes the HIGH
word into a plane of its own, which every key that meets its own low word must compare - in the second table too.

Natural input fills a span of homes with a key or two, so the inputs are built from keys chosen by their hashes:

  * slot: a k-mer that holds A^m has minimizer hash 0, the least, and slot_of(0, n) = 0: slot 0 under any plan;
  * home, second-table chain and key subset derive from H = key2_hash(lo, hi), the fold of the code's four 32-bit
    parts times 0x9E3779B1;
  * a span family has more keys with homes in a span than the span, the three entries behind it and the whole second
    table hold: the rest must take the last tier;
  * the same-H family XORs one 2-bit pattern into bases 16 apart (the fold is unchanged): one home, one chain;
  * the claim-word family shares its last 32 bases (the word that is claimed) inside the span: deep-tier probes, those
    of the second table included, meet an equal low word and have only the high plane to tell the keys apart.

Every GPU case asserts from eng.stats() which kernels did the work and runs twice with identical results and
statistics.  The CPU tests prove the constructions on the oracle's own keys and read the tier constants out of the
sources, so that a retune fails here instead of weakening the cases."""
import os
import random
import re

import numpy as np
import pytest

from oracle import c_oracle as CO
from tests import util
from tests.test_gpu_skm2 import code_of, geometry, key2_hash, minimizer, slot_of
from tests.util import instances, random_dna, records_of, revcomp, skm_line

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "khoice_amd", "csrc")

# ---- the tier constants (test_constants_match_sources reads them out of the sources)
FULL_ROUNDS = 4                  # KH_TUNE_SKM_FULL_ROUNDS
CHAIN = 8                        # probes in the second table
UT, UT2 = 1792, 32               # k_skm2_union: main and second table
U_CAP = 448                      # records of a slot (UT * 8 / 32, one per thread at most)
U_PLAN = U_CAP - 112             # what skm_plan asks of a slot's records before it clamps the region to U_CAP
U_NT, U_PASSES = 512, 4
U_MAXCH = U_NT * U_PASSES        # chunks (of two k-mers) of a slot
BT, BT2 = 2048, 64               # k_skm_big<SkmBig2>
B_ROUND = BT - BT // 4           # instances of one of its rounds
ONE_MAXCH, ONE_T, ONE_CAP = 3072, 4096, 1024   # k_skm_union (one-word keys): chunks, table, records of a slot

M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
SPAN = 40
ZERO_HOMES = 24
MARGIN = 40


# ---- restatements (kh_skm2.hip, kh_skm_device.h)
def H_of(s):
    """key2_hash of a k-mer that is canonical as written."""
    c = code_of(s)
    return key2_hash(c & M64, c >> 64)


def home(h, kind):
    return (h * UT) >> 32 if kind == "union" else h >> 21


def chain(h, kind):
    return ((h ^ (h >> 15)) * 0x85EBCA77 & M32) >> (27 if kind == "union" else 26)


def subset(h, r):
    return (((h >> 4) & 0xFFFF) * r) >> 16


def tables(kind):
    return (UT, UT2) if kind == "union" else (BT, BT2)


# ---- vectorised candidates
def _codes(b):
    c = np.zeros(b.shape[0], dtype=np.uint64)
    for j in range(b.shape[1]):
        c = (c << np.uint64(2)) | b[:, j].astype(np.uint64)
    return c


def _words2(b):
    """bases[n, k] -> (low word: the last 32 bases, high word: the bases before them)."""
    k = b.shape[1]
    return _codes(b[:, k - 32:]), _codes(b[:, :k - 32])


def _canon2_np(b):
    """bases[n, k], 33 <= k <= 63 -> (canonical as written, key2_hash of the canonical code)."""
    flo, fhi = _words2(b)
    rlo, rhi = _words2(3 - b[:, ::-1])
    fwd = (fhi < rhi) | ((fhi == rhi) & (flo < rlo))
    lo, hi = np.where(fwd, flo, rlo), np.where(fwd, fhi, rhi)
    s32 = np.uint64(32)
    h = (((lo ^ (lo >> s32) ^ hi ^ (hi >> s32)) & np.uint64(M32)) * np.uint64(0x9E3779B1)) & np.uint64(M32)
    return fwd, h


def _home_np(h, kind):
    return (h * np.uint64(UT)) >> np.uint64(32) if kind == "union" else h >> np.uint64(21)


def _in_span(h, kind, lo, homes):
    t = tables(kind)[0]
    return (_home_np(h, kind) + np.uint64(t - lo)) % np.uint64(t) < np.uint64(homes)


def _text(b):
    return "".join("ACGT"[x] for x in b)


def span_family(k, kind, lo, homes, n, seed, q=None, extra=()):
    """n distinct k-mers, canonical as written, each holding A^m (slot 0), whose homes lie in lo .. lo + homes - 1
    (mod the table).  q: also H bit 19 == q (subset q of a slot taken in two rounds)."""
    m = geometry(k)[0]
    rng = np.random.default_rng(seed)
    out = list(extra)
    seen = set(out)
    while len(out) < n:
        b = rng.integers(0, 4, size=(200_000, k), dtype=np.uint8)
        pos = rng.integers(0, k - m + 1, size=b.shape[0])
        np.put_along_axis(b, pos[:, None] + np.arange(m)[None, :], 0, axis=1)
        fwd, h = _canon2_np(b)
        ok = fwd & _in_span(h, kind, lo, homes)
        if q is not None:
            ok &= ((h >> np.uint64(19)) & np.uint64(1)) == np.uint64(q)
        for i in np.flatnonzero(ok):
            s = _text(b[i])
            if s not in seen:
                seen.add(s)
                out.append(s)
                if len(out) >= n:
                    break
    return out


def claim_family(k, kind, lo, homes, n, seed, q=None):
    """n distinct k-mers (k >= 41), canonical as written, that share their last 32 bases - the low word, the one the
    hash sets claim, with A^m inside it - and whose homes lie in the span: they differ in the high word alone."""
    m = geometry(k)[0]
    rng = np.random.default_rng(seed)
    r = random.Random(seed)
    a = r.randrange(1, 32 - m - 1)
    fixed = random_dna(r, a, "CGT") + "A" * m + random_dna(r, 32 - m - a - 1, "CGT") + r.choice("ACG")
    b = rng.integers(0, 4, size=(200_000, k), dtype=np.uint8)
    b[:, k - 32:] = np.array(["ACGT".index(c) for c in fixed], dtype=np.uint8)[None, :]
    b[:, 0] = 0                                         # starts with A, does not end in T: canonical as written
    fwd, h = _canon2_np(b)
    ok = fwd & _in_span(h, kind, lo, homes)
    if q is not None:
        ok &= ((h >> np.uint64(19)) & np.uint64(1)) == np.uint64(q)
    out = sorted({_text(b[i]) for i in np.flatnonzero(ok)})
    r.shuffle(out)
    assert len(out) >= n, (k, kind, len(out))
    return out[:n]


def same_hash_family(k, kind, lo, homes, n, seed, q=None):
    """n distinct k-mers (k >= 37), canonical as written, with ONE H whose home lies in the span: A^m ends the k-mer; one
    2-bit pattern XOR-ed into the bases 16 .. 19 and 32 .. 35 from the end flips the same bits of two of the four 32-bit
    parts that key2_hash folds."""
    m = geometry(k)[0]
    assert k >= 37 and m <= 16
    rng = np.random.default_rng(seed)
    pats = np.array([[(p >> (2 * i)) & 3 for i in range(4)] for p in range(256)], dtype=np.uint8)
    while True:
        base = rng.integers(0, 4, size=(4096, k), dtype=np.uint8)
        base[:, k - m:] = 0
        base[:, 0] = 0
        _, h = _canon2_np(base)
        ok = _in_span(h, kind, lo, homes)
        if q is not None:
            ok &= ((h >> np.uint64(19)) & np.uint64(1)) == np.uint64(q)
        for i in np.flatnonzero(ok):
            v = np.repeat(base[i][None, :], 256, axis=0)
            for j in range(4):
                v[:, k - 1 - (16 + j)] ^= pats[:, j]
                v[:, k - 1 - (32 + j)] ^= pats[:, j]
            fwd, _ = _canon2_np(v)
            fam = [_text(v[t]) for t in np.flatnonzero(fwd)]
            if len(fam) >= n:
                return fam[:n]


def run_records(k, n, seed, q=0, nk=8):
    """n records of nk k-mers (k + nk - 1 bases, A^m at bases nk - 1 .. nk + m - 2, inside every window) whose keys are
    distinct over all records and (q is not None) all have H bit 19 == q: every key in subset q of two rounds."""
    m = geometry(k)[0]
    assert nk - 1 + m <= k
    rng = np.random.default_rng(seed)
    out, seen = [], set()
    while len(out) < n:
        b = rng.integers(0, 4, size=(100_000, k + nk - 1), dtype=np.uint8)
        b[:, nk - 1:nk - 1 + m] = 0
        ok = np.ones(b.shape[0], dtype=bool)
        if q is not None:
            for j in range(nk):
                _, h = _canon2_np(b[:, j:j + k])
                ok &= ((h >> np.uint64(19)) & np.uint64(1)) == np.uint64(q)
        for i in np.flatnonzero(ok):
            s = _text(b[i])
            ks = {min(code_of(s[j:j + k]), code_of(revcomp(s[j:j + k]))) for j in range(nk)}
            if len(ks) == nk and not ks & seen:
                seen |= ks
                out.append(s)
                if len(out) >= n:
                    break
    return out


def filler_records(k, m, n, seed):
    """n records flank + A^m + flank (flanks of k - m bases): w = k - m + 1 k-mers each, all in slot 0."""
    rng = random.Random(seed)
    out = [random_dna(rng, k - m, "CGT") + "A" * m + random_dna(rng, k - m, "CGT") for _ in range(n)]
    assert len(set(out)) == n
    return out


# ---- what a slot's union will see of a text
def all_records(seqs):
    return [(g, r) for g in range(len(seqs)) for r in records_of(seqs, g) if r]


def merged(seqs, k):
    """The records the union keeps after it has merged identical ones: {(bases, half of the genome mask)}.  (A reverse
    complement is another record.)"""
    return {(r, g // 32) for g, r in all_records(seqs) if len(r) >= k}


def chunks_of(recs, k):
    return sum((len(r) - k + 2) // 2 for r, _ in recs)


def insts_of(recs, k):
    return sum(len(r) - k + 1 for r, _ in recs)


# ---- the inputs of each case (memoised: the CPU and the GPU tests use the same ones)
_CACHE = {}
memo = util.memo_in(_CACHE)

UNION_CASES = [(33, "wrap"), (41, "wrap"), (49, "wrap"), (63, "wrap"), (49, "zero")]
BIG_K = [41, 63]


@memo
def deep_family(k, kind, which, q=None):
    """{name: keys} whose union is one span family: `last` (at the table's last home), `claim` and `same_hash`
    (k >= 41) and `span`, all with homes in one span of the table of `kind`."""
    t, t2 = tables(kind)
    lo, homes = (t - SPAN, SPAN) if which == "wrap" else (0, ZERO_HOMES)
    parts = {}
    seed = 1000 * k + (7 if kind == "big" else 0) + (3 if which == "zero" else 0)
    if which == "wrap":
        parts["last"] = span_family(k, kind, t - 1, 1, 6, seed + 1, q)
    if k >= 41:
        parts["claim"] = claim_family(k, kind, lo, homes, 40, seed + 2, q)
        if which == "wrap":
            parts["same_hash"] = same_hash_family(k, kind, lo, homes, FULL_ROUNDS + CHAIN + MARGIN + 4, seed + 3, q)
    have = [s for p in parts.values() for s in p]
    n = homes + FULL_ROUNDS - 1 + t2 + MARGIN + 5
    parts["span"] = span_family(k, kind, lo, homes, max(n, len(have) + 12), seed + 4, q, tuple(have))[len(have):]
    return parts, lo, homes


def family_keys(k, kind, which, q=None):
    return [s for p in deep_family(k, kind, which, q)[0].values() for s in p]


@memo
def deep_case(k, kind, which):
    return util.skm_layout(family_keys(k, kind, which), 40, 10, geometry(k)[0])


@memo
def two_round_case():
    """k = 41: the wrap family in subset 1 plus 64 filler records of 27 k-mers: more than 1792 instances (R = 2) within
    the union's records and chunks."""
    fam = family_keys(41, "union", "wrap", 1)
    fill = filler_records(41, geometry(41)[0], 64, 4102)
    return fam, fill, util.skm_layout(fam, 40, 10, geometry(41)[0], fill)


def spread(recs, ngen, group_size):
    out = [[] for _ in range(ngen)]
    for j, r in enumerate(recs):
        out[j % ngen].append(r)
    return ["N".join(r).encode() for r in out], [g // group_size for g in range(ngen)]


UNION_SUBSET_RECORDS = 248     # x 8 keys = 1984 > UT + UT2 + 100
BIG_SUBSET_RECORDS = 560       # x 4 keys = 2240 > BT + BT2 + 100


@memo
def union_overflow_case():
    recs = run_records(41, UNION_SUBSET_RECORDS, 4103, 0, 8)
    return recs, spread(recs, 40, 10)


@memo
def big_overflow_case():
    recs = run_records(41, BIG_SUBSET_RECORDS, 4104, 0, 4)
    return recs, spread(recs, 40, 10)


BIG_TWO_ROUND_RECORDS = 560    # x 4 keys = 2240 instances: two of k_skm_big's rounds of 1536


@memo
def big_two_round_case():
    """k = 41: 560 records of 4 k-mers, all keys distinct and in whichever subset their hash says."""
    recs = run_records(41, BIG_TWO_ROUND_RECORDS, 4105, None, 4)
    return recs, spread(recs, 40, 10)


@memo
def handover_case(k, over):
    """Filler records whose chunks fill the union's chunk table exactly, and one short record of 8 k-mers (4 chunks) -
    or, `over`, of 9 (5 chunks: one chunk too many).  32 genomes (the low half of the mask) in groups of 8; the first ten
    filler records stand twice in their genome."""
    m = skm_m(k)
    if k > 32:    # 146 x 14 chunks + 4 (or 5)
        fill = filler_records(k, m, (U_MAXCH - 4) // ((k - m + 2) // 2), 100 * k + 5)
        short = run_records(k, 1, 100 * k + 8 + over, None, 8 + over)
    else:         # one-word keys: 384 (or 385) x 8 chunks
        fill = filler_records(k, m, ONE_MAXCH // ((k - m + 2) // 2) + over, 100 * k + 5)
        short = []
    recs = [[] for _ in range(32)]
    for j, r in enumerate(fill + short):
        recs[j % 32].append(r)
    for j in range(10):
        recs[j % 32].append(fill[j])
    return fill, short, (["N".join(r).encode() for r in recs], [g // 8 for g in range(32)])


def skm_m(k):
    """The minimizer length: two-word keys by geometry(); k = 31 (one-word keys): 16."""
    return geometry(k)[0] if k > 32 else {31: 16}[k]


# =========================================================================== CPU: the constructions
def _src(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def test_constants_match_sources():
    skm2, dev, skm1 = _src("kh_skm2.hip"), _src("kh_skm_device.h"), _src("kh_skm.hip")
    assert int(re.search(r"#define KH_TUNE_SKM_FULL_ROUNDS (\d+)", dev).group(1)) == FULL_ROUNDS
    assert int(re.search(r"#define KH_TUNE_SKM2_UT (\d+)", skm2).group(1)) == UT
    assert int(re.search(r"#define KH_TUNE_SKM2_UNT (\d+)", skm2).group(1)) == U_NT
    assert int(re.search(r"SKM2_UT2 = (\d+);", skm2).group(1)) == UT2
    assert int(re.search(r"constexpr u32 SKM2_PASSES = (\d+);", skm2).group(1)) == U_PASSES
    assert "SKM2_MAXCH = SKM2_PASSES * SKM2_UNT;" in skm2 and "SKM2_UE = 2;" in skm2
    assert "SKM2_STAGE = SKM2_UT * 8 / 32;" in skm2 and "SKM2_MAXREC = SKM2_STAGE < SKM2_UNT ? SKM2_STAGE : SKM2_UNT;" in skm2
    assert UT * 8 // 32 == U_CAP <= U_NT
    big = re.search(r"struct SkmBig2 \{.*?static constexpr u32 T = (\d+), T2 = (\d+),", skm2, re.S)
    assert (int(big.group(1)), int(big.group(2))) == (BT, BT2)
    assert "constexpr u32 skm_walk_round() { return Tr::T - Tr::T / 4; }" in dev
    assert "R = (N + skm_walk_round<Tr>() - 1u) / skm_walk_round<Tr>();" in dev
    assert "const u32 R = (N + T - 1) / T;" in skm2
    assert skm2.count("round < 8u") == 1 and "probes >= 8u" in dev                # the second-table chain
    assert ">> 27; }   // T2 = 32" in skm2
    assert "slot_[e] = (u32)(((u64)h * T) >> 32);" in skm2
    assert "u32 S = H >> (32 - HBITS)" in dev and "S = ((H ^ (H >> 15)) * 0x85EBCA77u) >> (32 - H2BITS);" in dev
    assert "(u32)(((u64)key2_hash(klo[e], khi[e]) * T) >> 32) + (u32)KH_TUNE_SKM_FULL_ROUNDS; slot_[e] = x >= T ? x - T : x;" in skm2
    assert "S = ((H >> (32 - HBITS)) + (u32)KH_TUNE_SKM_FULL_ROUNDS) & (T - 1u);" in dev
    assert ("key2_hash(u64 lo, u64 hi) { return ((u32)lo ^ (u32)(lo >> 32) ^ (u32)hi ^ (u32)(hi >> 32)) * 0x9E3779B1u; }"
            in skm2)
    assert "(((h >> 4) & 0xffffu) * R) >> 16 == q" in skm2
    assert "skm_round_of(const u32 H, const u32 R) { return (((H >> 4) & 0xffffu) * R) >> 16; }" in dev
    assert "if (R != 1 && skm_round_of(H, R) != q) return;" in dev
    assert "if ((sc0 & 0xffffu) > SKM2_MAXCH)" in skm2 and "if (C > SKM2_MAXCH)" in skm2
    # the planner's clamp (kh_engine.cpp) and the one-word union of the hand-over's twin
    eng = _src("kh_engine.cpp")
    assert "(double)fan + recs / (double)g.nslots <= (double)max_cap2 - 112.0" in eng
    assert "SKM_PASSES = SKM_UE == 2 ? 3 : 2;" in skm1 and "#define KH_TUNE_SKM_UE 2" in skm1
    assert "using SkmUnion = SkmUnionGeo<1024, 4096>;" in skm1 and "MAXCH = SKM_PASSES * NT;" in skm1
    assert "if ((sc0 & 0xffffu) > G::MAXCH)" in skm1 and 3 * ONE_CAP == ONE_MAXCH


def check_keys(fam, k):
    """Distinct, canonical as written on the oracle's own keys, A^m inside (minimizer 0: slot 0)."""
    m = geometry(k)[0]
    assert len(set(fam)) == len(fam)
    keys, counts = CO.count("N".join(fam).encode(), k).arrays()
    got = sorted(int(a) | (int(b) << 64) for a, b in zip(keys[:, 0], keys[:, 1]))
    assert got == sorted(code_of(s) for s in fam) and (counts == 1).all()
    assert {minimizer(s, m) for s in fam} == {0}


def check_family(k, kind, which, q=None):
    t, t2 = tables(kind)
    parts, lo, homes = deep_family(k, kind, which, q)
    fam = family_keys(k, kind, which, q)
    check_keys(fam, k)
    hs = [H_of(s) for s in fam]
    assert all((home(h, kind) - lo) % t < homes for h in hs)
    assert len(fam) >= homes + (FULL_ROUNDS - 1) + t2 + MARGIN          # the last tier must run
    if q is not None:
        assert {subset(h, 2) for h in hs} == {q}
    if which == "wrap":
        assert sum(home(h, kind) == t - 1 for h in hs) >= 3 and min(home(h, kind) for h in hs) >= t - SPAN
        assert len(parts["last"]) >= 3 and all(home(H_of(s), kind) == t - 1 for s in parts["last"])
    if k >= 41:
        cl = parts["claim"]
        assert len(cl) >= 40 and len({s[-32:] for s in cl}) == 1 and "A" * geometry(k)[0] in cl[0][-32:]
        assert len({code_of(s) & M64 for s in cl}) == 1 and len({code_of(s) >> 64 for s in cl}) == len(cl)
    if "same_hash" in parts:
        sh = [H_of(s) for s in parts["same_hash"]]
        assert len(set(sh)) == 1 and len(sh) > FULL_ROUNDS + CHAIN + MARGIN
        assert len({chain(h, kind) for h in sh}) == 1
    return fam


def test_slot_zero():
    """Minimizer hash 0 (check_keys proves it for every key) is slot 0 whatever number of slots the planner picks."""
    for ns in (1, 7, 12, 17, 1000, 500_000):
        assert slot_of(0, ns) == 0


@pytest.mark.parametrize("k,which", UNION_CASES)
def test_union_family_preconditions(k, which):
    fam = set(check_family(k, "union", which))
    seqs, _ = deep_case(k, "union", which)
    check_layout(seqs, fam, k)
    recs = all_records(seqs)
    assert len(recs) <= U_PLAN and chunks_of(merged(seqs, k), k) <= U_MAXCH
    assert instances(seqs, k) <= UT                                   # one round
    assert all(len(s) < 2048 for s in seqs)                           # no record is cut at a wave's edge


def check_layout(seqs, fam, k):
    m = geometry(k)[0]
    lo_half = {s for g in range(32) for s in records_of(seqs, g)}
    hi_half = {s for g in range(32, 40) for s in records_of(seqs, g)}
    assert len(fam & lo_half & hi_half) > 5 and len(fam & hi_half) > 20       # identical records in both halves
    rep_rc = rep_two = 0
    for g in range(len(seqs)):
        recs = set(records_of(seqs, g))
        rep_rc += sum(1 for s in fam if s in recs and revcomp(s) in recs)
        rep_two += sum(1 for s in fam if s in recs and util.two_kmer(s, m) in recs)
    assert rep_rc > len(fam) // 3 and rep_two > len(fam) // 5


def test_two_round_preconditions():
    k, m = 41, geometry(41)[0]
    fam, fill, (seqs, _) = two_round_case()
    assert fam == check_family(k, "union", "wrap", 1)                  # every family key in subset 1 of two rounds
    for r in fill:
        assert len(r) - k + 1 == k - m + 1 == 27
        assert {minimizer(r[j:j + k], m) for j in range(27)} == {0}
    kept = merged(seqs, k)
    assert UT < insts_of(kept, k) <= instances(seqs, k) <= 2 * UT       # R = 2, before and after the merge
    assert chunks_of(kept, k) <= U_MAXCH and len(all_records(seqs)) <= U_PLAN
    assert all(len(s) < 2048 for s in seqs)


def check_run_records(recs, k, nk, q):
    m = geometry(k)[0]
    keys = set()
    for r in recs:
        assert len(r) == k + nk - 1
        for j in range(nk):
            s = r[j:j + k]
            assert minimizer(s, m) == 0
            c = min(code_of(s), code_of(revcomp(s)))
            if q is not None:
                assert subset(key2_hash(c & M64, c >> 64), 2) == q
            keys.add(c)
    assert len(keys) == nk * len(recs)
    keys_o, _ = CO.count("N".join(recs).encode(), k).arrays()
    assert sorted(int(a) | (int(b) << 64) for a, b in zip(keys_o[:, 0], keys_o[:, 1])) == sorted(keys)
    return keys


def test_union_overflow_preconditions():
    recs, (seqs, _) = union_overflow_case()
    keys = check_run_records(recs, 41, 8, 0)
    assert UT + UT2 + 100 < len(keys) < 2 * UT and len(keys) == instances(seqs, 41)     # R = 2, subset 0 overflows
    assert len(recs) <= U_PLAN and chunks_of(merged(seqs, 41), 41) <= U_MAXCH              # the union's own slot
    assert all(len(s) < 2048 for s in seqs)


def test_big_overflow_preconditions():
    recs, (seqs, _) = big_overflow_case()
    keys = check_run_records(recs, 41, 4, 0)
    assert BT + BT2 + 100 < len(keys) <= 2 * B_ROUND and len(keys) == instances(seqs, 41)   # R = 2 in k_skm_big
    assert len(recs) > U_CAP                                                              # k_skm_big's under any slack
    assert all(len(s) < 2048 for s in seqs)


def test_big_two_round_preconditions():
    recs, (seqs, _) = big_two_round_case()
    keys = check_run_records(recs, 41, 4, None)
    assert B_ROUND < len(keys) <= 2 * B_ROUND and len(keys) == instances(seqs, 41)          # R = 2 in k_skm_big
    per_subset = [sum(subset(key2_hash(c & M64, c >> 64), 2) == q for c in keys) for q in (0, 1)]
    assert 0 < min(per_subset) and max(per_subset) <= BT + BT2                              # both rounds work, both fit
    assert len(recs) > U_CAP                                                              # k_skm_big's under any slack
    assert all(len(s) < 2048 for s in seqs)


@pytest.mark.parametrize("k", [41, 31])
def test_handover_preconditions(k):
    m = skm_m(k)
    maxch, cap, t = (U_MAXCH, U_CAP, UT) if k > 32 else (ONE_MAXCH, ONE_CAP, ONE_T)
    for over in (0, 1):
        fill, short, (seqs, group_of) = handover_case(k, over)
        recs = all_records(seqs)
        assert len(recs) == len(fill) + len(short) + 10 <= cap - 112
        assert max(len(records_of(seqs, g)) for g in range(32)) >= 2 and len(seqs) == 32   # the low half of the mask
        for r in fill:
            assert len(r) - k + 1 == k - m + 1 and "A" * m in r[k - m:k]                  # A^m inside every window
        kept = merged(seqs, k)
        assert len(kept) == len(fill) + len(short)
        assert chunks_of(kept, k) == maxch + over * (1 if k > 32 else 8)          # exactly full / one record over
        reps = [(g, r) for g in range(32) for r in set(records_of(seqs, g)) if records_of(seqs, g).count(r) == 2]
        assert len(reps) == 10                                                           # merged repeats inside genomes
        assert all(len(s) < 2048 for s in seqs)
        if k > 32:
            assert (len(fill), len(short[0]) - k + 1) == (146, 9 if over else 8)
            assert -(-insts_of(kept, k) // t) == 3 and maxch == U_PASSES * U_NT            # R = 3, all four index passes
            check_run_records(short, k, 9 if over else 8, None)
        else:
            assert len(fill) == (385 if over else 384) and (k - m + 2) // 2 == 8
            assert -(-insts_of(kept, k) // t) == 2


@pytest.mark.parametrize("k", BIG_K)
def test_big_family_preconditions(k):
    fam = set(check_family(k, "big", "wrap"))
    assert len(fam) >= SPAN + 3 + BT2 + MARGIN
    seqs, _ = deep_case(k, "big", "wrap")
    check_layout(seqs, fam, k)
    assert instances(seqs, k) <= B_ROUND                               # one round
    assert all(len(s) < 2048 for s in seqs)


# =========================================================================== GPU
KERNELS = ("skm_union", "skm_big", "union_tagged")
COUNTERS = ("retries", "big_slots", "skm_records")


@pytest.fixture(scope="module")
def eng():
    from khoice_amd import build as kbuild
    from khoice_amd import engine as E
    if not os.environ.get("KHOICE_HIP_LIB"):
        kbuild.build_library()
    e = E.Engine(0)
    yield e
    e.close()


def check(eng, capfd, seqs, group_of, k, expect):
    return util.exp1_check(eng, capfd, seqs, group_of, k, expect, KERNELS, COUNTERS)


UNION_ONLY = dict(skm_union=1, skm_big=0, union_tagged=0, retries=0, big_slots=0)
BIG = dict(skm_union=1, skm_big=1, union_tagged=0, retries=0, big_slots=(1, None))
FALLBACK = dict(skm_union=1, union_tagged=(1, None), retries=1)


@pytest.fixture
def skm_env(monkeypatch):
    monkeypatch.setenv("KHOICE_SKM_DEBUG", "1")
    return monkeypatch


# ---- A. k_skm2_union: slot 0 within its region (a slack the planner clamps to the union's 448 records)
@pytest.mark.gpu
@pytest.mark.parametrize("k,which", UNION_CASES)
def test_union_deep_tiers(eng, capfd, skm_env, k, which):
    """More keys in homes 1752 .. 1791 (several at 1791; `zero`: homes 0 .. 23) than the span, the three entries behind
    it and the second table hold: the last tier runs from home + 4 and wraps at 1791.  From k = 41 on, 40 of the keys share
    the claimed word and differ in the high plane only, and 56 share one H.  The layout puts the keys in both mask
    halves, repeats them in other records of one genome and keeps identical records of the two halves apart."""
    skm_env.setenv("KHOICE_SKM_SLACK", "50")
    seqs, group_of = deep_case(k, "union", which)
    nrec = len(all_records(seqs))
    for err in check(eng, capfd, seqs, group_of, k, dict(UNION_ONLY, skm_records=nrec)):
        d = skm_line(err)
        assert (d["k"], d["m"]) == (k, geometry(k)[0])
        assert d["cap"] == U_CAP and d["slot_max"] == nrec and d["overfull"] == 0 and d["errors"] == 0, d
        assert d["expanded"] == insts_of(merged(seqs, k), k) <= UT               # one round


# ---- B. two rounds
@pytest.mark.gpu
def test_union_two_rounds(eng, capfd, skm_env):
    """R = 2 with the whole wrap family in subset 1: its last-tier walk runs in a table that was cleared for round 2."""
    skm_env.setenv("KHOICE_SKM_SLACK", "50")
    _, _, (seqs, group_of) = two_round_case()
    for err in check(eng, capfd, seqs, group_of, 41, UNION_ONLY):
        d = skm_line(err)
        assert d["cap"] == U_CAP and d["slot_max"] <= d["cap"] and d["overfull"] == 0 and d["errors"] == 0, d
        assert UT < d["expanded"] == insts_of(merged(seqs, 41), 41) <= 2 * UT, d


# ---- C. a subset with more keys than both tables hold
@pytest.mark.gpu
def test_union_subset_overflow(eng, capfd, skm_env):
    """More than 1792 + 32 distinct keys in subset 0 of an R = 2 slot: the last tier's exit raises KH_ERR_CAPACITY, the
    call is retried once in the key-array form, and the answer is exact."""
    skm_env.setenv("KHOICE_SKM_SLACK", "50")
    _, (seqs, group_of) = union_overflow_case()
    for err in check(eng, capfd, seqs, group_of, 41, dict(FALLBACK, skm_big=0, big_slots=0)):
        d = skm_line(err)
        assert d["cap"] == U_CAP and d["slot_max"] <= d["cap"] and d["overfull"] == 0 and d["errors"] != 0, d


# ---- D. the chunk-count hand-over
@pytest.mark.gpu
@pytest.mark.parametrize("k", [41, 31])
def test_chunk_count_handover(eng, capfd, skm_env, k):
    """A slot whose merged records make exactly as many chunks as the union numbers (k = 41: 2048, R = 3, all four index
    passes; k = 31: 3072) stays the union's; one chunk more and k_skm_big takes it although its records fit the region.
    Ten records stand twice in their genome: the merge has counted those repeats before the hand-over is decided and
    must take them back, or distinct_per_seq comes out too small."""
    skm_env.setenv("KHOICE_SKM_SLACK", "50")
    cap = U_CAP if k > 32 else ONE_CAP
    for over, expect in ((0, UNION_ONLY), (1, dict(UNION_ONLY, skm_big=1, big_slots=1))):
        _, _, (seqs, group_of) = handover_case(k, over)
        nrec = len(all_records(seqs))
        for err in check(eng, capfd, seqs, group_of, k, dict(expect, skm_records=nrec)):    # the scatter cut no record
            d = skm_line(err)
            assert d["cap"] == cap and d["slot_max"] == nrec <= cap and d["errors"] == 0, d
            assert d["overfull"] == over and d["spilled"] == 0, d
            assert d["expanded"] == insts_of(merged(seqs, k), k), d


# ---- E. k_skm_big<SkmBig2>: slot 0 above its region
@pytest.mark.gpu
@pytest.mark.parametrize("k", BIG_K)
def test_big_deep_tiers(eng, capfd, skm_env, k):
    """Homes 2008 .. 2047 of k_skm_big's table of 2048, more keys than the span, the three entries behind it and its
    second table of 64 hold, the claim-word and the same-H family among them; part of the slot comes from the side list."""
    skm_env.setenv("KHOICE_SKM_SLACK", "0.3")
    seqs, group_of = deep_case(k, "big", "wrap")
    for err in check(eng, capfd, seqs, group_of, k, BIG):
        d = skm_line(err)
        assert d["overfull"] >= 1 and d["slot_max"] > d["cap"] and d["spilled"] > 0 and d["errors"] == 0, d


@pytest.mark.gpu
@pytest.mark.parametrize("big_y", [1, 2, 16])
def test_big_two_rounds(eng, capfd, skm_env, big_y):
    """k_skm_big completes a slot in R = ceil(2240 / 1536) = 2 rounds, neither subset above its tables; more records than
    the union's region holds, so part of them comes from the side list.  The rounds are shared out over KHOICE_SKM_BIG_Y
    workgroups: with 1 one workgroup clears the table between its two rounds, with 2 each runs one, with 16 fourteen
    have no round and only flush."""
    skm_env.setenv("KHOICE_SKM_SLACK", "50")
    skm_env.setenv("KHOICE_SKM_BIG_Y", str(big_y))
    recs, (seqs, group_of) = big_two_round_case()
    for err in check(eng, capfd, seqs, group_of, 41, BIG):
        d = skm_line(err)
        assert d["cap"] == U_CAP and d["overfull"] >= 1 and d["slot_max"] > d["cap"] and d["errors"] == 0, d
        assert d["spilled"] == len(recs) - U_CAP, d


# ---- F. k_skm_big: a subset with more keys than both tables hold
@pytest.mark.gpu
def test_big_subset_overflow(eng, capfd, skm_env):
    """k_skm_big takes R = ceil(N / 1536) = 2 rounds: every key in subset 0, more than 2048 + 64; more records than the
    union's region holds under any slack, so the surplus goes through the side list."""
    skm_env.setenv("KHOICE_SKM_SLACK", "50")
    recs, (seqs, group_of) = big_overflow_case()
    for err in check(eng, capfd, seqs, group_of, 41, dict(FALLBACK, skm_big=1)):
        d = skm_line(err)
        assert d["cap"] == U_CAP and d["overfull"] >= 1 and d["spilled"] == len(recs) - U_CAP, d
