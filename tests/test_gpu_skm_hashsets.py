"""The LDS hash sets of the one-word forms of the fused exp-1 path, at every probe tier and overflow exit, bit-exact
against the C restatement (oracle.c_oracle.exp1).

k_skm_union, k_skm_big and k_skm_phased (khoice_amd/csrc/kh_skm.hip) and k_union_hash (kh_kernels.hip) share one
design: a few probes in the main table from the key's home entry, then a small second table with an independent
hash, then unbounded probing of the main table, whose last exit raises KH_ERR_CAPACITY.  Natural input reaches the
deep tiers only by chance, so the inputs here are built from keys chosen by their hashes:

  * slot: a k-mer that holds the all-A m-mer (or the all-T one) has minimizer hash 0, the least (the m-mer hash is a
    bijection), and slot_of(0, n) = 0 for any n: every such k-mer lands in slot 0 whatever the plan;
  * home, second-table chain and key subset of the super-k-mer forms all derive from H = key_hash2(lo, hi);
  * the key-array form homes a key by the fine bin of its mixed key: keys that share their top 32 mixed bits share it.

A family of n keys whose homes lie in a span of `homes` entries cannot all be placed by the first tiers when
n > homes + (main-table probes - 1) + (second-table entries): the rest must take the last tier.  Every GPU case
asserts from eng.stats() which kernels did the work, and runs twice with identical results and statistics.  The
CPU tests prove the constructions (canonical keys, slot 0, shared homes / chains / subsets, the bounds) without a
kernel, and read the tier constants out of the sources, so that a retune fails here instead of weakening the cases."""
import os
import random
import re

import numpy as np
import pytest

from oracle import c_oracle as CO
from tests import util
from tests.util import (PAIRS, instances, mix_np, mixed_from_top32, random_dna, records_of, revcomp, skm_line, top32_np,
                        unmix_np)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "khoice_amd", "csrc")

# ---- the tier constants (test_constants_match_sources reads them out of the sources)
SKM_FULL_ROUNDS = 4        # KH_TUNE_SKM_FULL_ROUNDS: main-table probes of k_skm_union / k_skm_big / k_skm_phased
SKM_T, SKM_T2 = 4096, 128  # their main and second tables (T, T2)
SKM_CHAIN = 8              # probes in the second table before the main one again
PH_ROUND = 3072            # SKM_PH_ROUND: instances a round of k_skm_phased takes
PH_FULL = SKM_T - SKM_T // 16   # k_skm_phased's near-full check at the fold
HASH_ROUNDS = 3            # KH_TUNE_HASH_ROUNDS: main-table probes of k_union_hash
UH_T2 = 512                # k_union_hash<512, 4096>: second table (T / 8)

M32 = 0xFFFFFFFF


def minimizer_len(k):
    """skm_minimizer_len (kh_engine.cpp): 12 for k <= 24, 13 up to 27, then 16 where that makes the window a power of
    two, else 15.  (test_union_deep_tiers checks it against the engine's [skm] line.)"""
    if k <= 24:
        return 12
    if k <= 27:
        return 13
    w15 = k - 14
    return 16 if (w15 - 1) & (w15 - 2) == 0 else 15


# ---- restatements (kh_skm_device.h, kh_skm.hip)
def mmer_hash(canon):
    h = (canon * 0x9E3779B1) & M32
    return h ^ (h >> 15)


def slot_of(minv, nslots):
    x = (minv * 0xC2B2AE35) & M32
    x ^= x >> 16
    x = (x * 0x27D4EB2F) & M32
    x ^= x >> 15
    return (x * nslots) >> 32


def code_of(s):
    c = 0
    for ch in s:
        c = (c << 2) | "ACGT".index(ch)
    return c


def canon_of(s):
    return min(code_of(s), code_of(revcomp(s)))


def minimizer(kmer, m):
    return min(mmer_hash(canon_of(kmer[i:i + m])) for i in range(len(kmer) - m + 1))


def key_hash(code):
    """key_hash2 of a canonical code: its 32-bit halves XOR-ed, times 0x9E3779B1."""
    return ((code & M32) ^ (code >> 32)) * 0x9E3779B1 & M32


def home(h):
    return h >> 20                                            # (H * T) >> 32 with T = 4096


def chain(h):
    return ((h ^ (h >> 15)) * 0x85EBCA77 & M32) >> 25       # second-table start (T2 = 128)


def subset(h, r):
    return (((h >> 4) & 0xFFFF) * r) >> 16


# ---- vectorised candidates
def _codes(b):
    c = np.zeros(b.shape[0], dtype=np.uint64)
    for j in range(b.shape[1]):
        c = (c << np.uint64(2)) | b[:, j].astype(np.uint64)
    return c


def _canon_np(b):
    """bases[n, k] -> (code as written, canonical code, key_hash2 of the canonical code)."""
    f, r = _codes(b), _codes(3 - b[:, ::-1])
    c = np.minimum(f, r)
    h = (((c & np.uint64(M32)) ^ (c >> np.uint64(32))) * np.uint64(0x9E3779B1)) & np.uint64(M32)
    return f, c, h


def _text(b):
    return "".join("ACGT"[x] for x in b)


def span_family(k, lo, homes, n, seed, q=None, extra=()):
    """n distinct k-mers, canonical as written, each holding A^m (slot 0), whose homes lie in lo .. lo + homes - 1
    (mod 4096).  q: also H bit 19 == q (subset q of a slot taken in two rounds)."""
    m = minimizer_len(k)
    rng = np.random.default_rng(seed)
    out = list(extra)
    seen = {code_of(s) for s in out}
    while len(out) < n:
        b = rng.integers(0, 4, size=(200_000, k), dtype=np.uint8)
        pos = rng.integers(0, k - m + 1, size=b.shape[0])
        np.put_along_axis(b, pos[:, None] + np.arange(m)[None, :], 0, axis=1)
        f, c, h = _canon_np(b)
        ok = (f == c) & (((h >> np.uint64(20)) - np.uint64(lo)) % np.uint64(4096) < np.uint64(homes))
        if q is not None:
            ok &= ((h >> np.uint64(19)) & np.uint64(1)) == np.uint64(q)
        for i in np.flatnonzero(ok):
            if int(f[i]) not in seen:
                seen.add(int(f[i]))
                out.append(_text(b[i]))
                if len(out) >= n:
                    break
    return out


def same_hash_family(seed):
    """k = 24 (m = 12): A^12 at bases 4 .. 15; one 2-bit pattern XOR-ed into bases i and i + 16 (i < 4) flips the same
    bits of both 32-bit halves, so key_hash2 is unchanged: up to 256 keys with ONE H (one home, one chain)."""
    rng = np.random.default_rng(seed)
    pats = np.array([[(p >> (2 * i)) & 3 for i in range(4)] for p in range(256)], dtype=np.uint8)
    while True:
        base = rng.integers(0, 4, size=24, dtype=np.uint8)
        base[4:16] = 0
        v = np.repeat(base[None, :], 256, axis=0)
        v[:, 0:4] ^= pats
        v[:, 16:20] ^= pats
        f, c, _ = _canon_np(v)
        fam = [_text(v[i]) for i in np.flatnonzero(f == c)]
        if len(fam) >= 96:
            return fam


def run_records(k, n, seed, q=0, nk=8):
    """n records of nk k-mers (k + nk - 1 bases, A^m at bases nk - 1 .. nk + m - 2, inside every window) whose keys all
    have H bit 19 == q: in a slot taken in R = 2 rounds every key is in subset q."""
    m = minimizer_len(k)
    assert nk - 1 + m <= k
    rng = np.random.default_rng(seed)
    out, seen = [], set()
    while len(out) < n:
        b = rng.integers(0, 4, size=(100_000, k + nk - 1), dtype=np.uint8)
        b[:, nk - 1:nk - 1 + m] = 0
        ok = np.ones(b.shape[0], dtype=bool)
        keys = []
        for j in range(nk):
            _, c, h = _canon_np(b[:, j:j + k])
            ok &= ((h >> np.uint64(19)) & np.uint64(1)) == np.uint64(q)
            keys.append(c)
        for i in np.flatnonzero(ok):
            ks = {int(kc[i]) for kc in keys}
            if len(ks) == nk and not ks & seen:
                seen |= ks
                out.append(_text(b[i]))
                if len(out) >= n:
                    break
    return out


def filler_records(k, n, seed):
    """n records flank + A^m + flank (flanks of k - m bases): w = k - m + 1 k-mers each, all in slot 0."""
    m = minimizer_len(k)
    rng = random.Random(seed)
    return [random_dna(rng, k - m, "CGT") + "A" * m + random_dna(rng, k - m, "CGT") for _ in range(n)]


# ---- genomes: halves, repeats, identical records (tests/util.py: shared with the two-word module)
def two_kmer(s):
    return util.two_kmer(s, minimizer_len(len(s)))


def layout(keys, ngen, group_size, extra_records=()):
    return util.skm_layout(keys, ngen, group_size, minimizer_len(len(keys[0])), extra_records)


# ---- the inputs of each case (memoised: the CPU and the GPU tests use the same ones)
_CACHE = {}
memo = util.memo_in(_CACHE)


UNION_K = [20, 24, 27, 31, 32]
WRAP_HOMES = 40                 # homes 4056 .. 4095: the main-table walk wraps
ZERO_HOMES = 24                 # k = 32: homes 0 .. 23, with poly-A (key 0, home 0)
MARGIN = 40


@memo
def deep_families(k):
    """{name: (keys, first home, homes)}: families that the first two tiers cannot place."""
    fams = {}
    if k == 32:
        n = ZERO_HOMES + SKM_FULL_ROUNDS - 1 + SKM_T2 + MARGIN
        fams["zero"] = (span_family(k, 0, ZERO_HOMES, n, 3200, None, ("A" * 32,)), 0, ZERO_HOMES)
    else:
        n = WRAP_HOMES + SKM_FULL_ROUNDS - 1 + SKM_T2 + MARGIN
        last = span_family(k, SKM_T - 1, 1, 8, 100 * k)                       # (eight of them at home 4095)
        fams["wrap"] = (span_family(k, SKM_T - WRAP_HOMES, WRAP_HOMES, n, 100 * k + 1, None, last), SKM_T - WRAP_HOMES, WRAP_HOMES)
    if k == 24:
        fam = same_hash_family(24)
        fams["same_hash"] = (fam, home(key_hash(code_of(fam[0]))), 1)
    return fams


def family_keys(k):
    return [s for fam, _, _ in deep_families(k).values() for s in fam]


@memo
def deep_case(k, ngen=40, group_size=10):
    return layout(family_keys(k), ngen, group_size)


@memo
def two_round_case():
    """k = 31: a wrap family in subset 0 plus 240 filler records of 16 k-mers: more than 4096 instances (R = 2)
    within the union's records and chunks."""
    n = WRAP_HOMES + SKM_FULL_ROUNDS - 1 + SKM_T2 + MARGIN
    fam = span_family(31, SKM_T - WRAP_HOMES, WRAP_HOMES, n, 3101, 0)
    fill = filler_records(31, 240, 3102)
    return fam, fill, layout(fam, 40, 10, fill)


SUBSET_KEYS = SKM_T + SKM_T2 + 176     # more distinct keys in one subset than both tables hold


@memo
def overflow_records():
    return run_records(31, SUBSET_KEYS // 8, 3103)


def overflow_case(ngen, group_size):
    recs = [[] for _ in range(ngen)]
    for j, r in enumerate(overflow_records()):
        recs[j % ngen].append(r)
    return ["N".join(r).encode() for r in recs], [g // group_size for g in range(ngen)]


UH_K = [24, 31, 32]
UH_FAMILY = HASH_ROUNDS + UH_T2 + 105


def special_code(k=32):
    """The code whose mixed key is all ones (k_union_hash's empty marker: that key is carried beside the tables)."""
    return int(unmix_np(k, np.array([[(1 << 64) - 1]], dtype=np.uint64))[0, 0])


def rc_code(c, k):
    r = 0
    for _ in range(k):
        r = (r << 2) | (3 - (c & 3))
        c >>= 2
    return r


def decode(c, k):
    return "".join("ACGT"[(c >> (2 * (k - 1 - j))) & 3] for j in range(k))


@memo
def top32_family(k):
    """Canonical codes whose mixed keys share their top 32 bits (k = 32: all ones, the top of the key space): one slot
    and one fine bin, hence one home, in any geometry of the key arrays.  (The code whose mixed key is all ones is not
    canonical, so no canonical k-mer reaches k_union_hash's `special` path: test_top32_family_preconditions pins that.)"""
    top = 0xFFFFFFFF if k == 32 else (0x5A5A5A5A ^ (k * 0x01010101)) & M32
    rng = np.random.default_rng(k)
    out, seen = [], set()
    if k == 32 and special_code() < rc_code(special_code(), k):
        out.append(special_code())
        seen.add(out[0])
    while len(out) < UH_FAMILY:
        codes = unmix_np(k, mixed_from_top32(k, np.full(20_000, top, dtype=np.uint64), rng))[:, 0]
        for c in (int(x) for x in codes):
            if c not in seen and c < rc_code(c, k):
                seen.add(c)
                out.append(c)
                if len(out) >= UH_FAMILY:
                    break
    return top, out


@memo
def top32_case(k):
    """64 genomes in 4 groups: key i in genome i % 64, every even one also in another, every fifth once more as its
    reverse complement (a repeat when it lands in a genome that holds the key)."""
    _, codes = top32_family(k)
    recs = [[] for _ in range(64)]
    for i, c in enumerate(codes):
        s = decode(c, k)
        recs[i % 64].append(s)
        if i % 2 == 0:
            recs[(i * 7 + 5) % 64].append(s)
        if i % 5 == 0:
            recs[(i * 13 + 1) % 64].append(revcomp(s))
    return ["N".join(r).encode() for r in recs], [g // 16 for g in range(64)]


# =========================================================================== CPU: the constructions
def _src(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def test_constants_match_sources():
    # (kh_skm_device.h holds what the kernels of kh_skm.hip share with the two-word ones: the tuning macro, the probe
    # walk of k_skm_big / k_skm_phased; k_skm_union's serial tier is a loop of its own in kh_skm.hip)
    skm, ker, com = _src("kh_skm.hip") + _src("kh_skm_device.h"), _src("kh_kernels.hip"), _src("kh_common.h")
    assert int(re.search(r"#define KH_TUNE_SKM_FULL_ROUNDS (\d+)", skm).group(1)) == SKM_FULL_ROUNDS
    assert int(re.search(r"#define KH_TUNE_HASH_ROUNDS (\d+)", com).group(1)) == HASH_ROUNDS
    assert int(re.search(r"static constexpr u32 T2 = (\d+);", skm).group(1)) == SKM_T2
    assert int(re.search(r"using SkmUnion = SkmUnionGeo<1024, (\d+)>;", skm).group(1)) == SKM_T
    big = re.search(r"SKM_BIG_T = (\d+), SKM_BIG_T2 = (\d+)", skm)
    ph = re.search(r"SKM_PH_T = (\d+), SKM_PH_T2 = (\d+)", skm)
    assert (int(big.group(1)), int(big.group(2))) == (int(ph.group(1)), int(ph.group(2))) == (SKM_T, SKM_T2)
    assert int(re.search(r"SKM_PH_ROUND = (\d+);", skm).group(1)) == PH_ROUND
    assert "scratch[1] > T - T / 16" in skm
    assert skm.count("probes >= 8u") == 2                          # the second-table chain: the union's, the shared walk's
    assert "key_hash2(u32 lo, u32 hi) { return (lo ^ hi) * 0x9E3779B1u; }" in skm
    assert skm.count("(H ^ (H >> 15)) * 0x85EBCA77u") == 2
    # the subset rule: skm_round_of once, called by the slot walk and by k_skm_phased; the union's own line
    assert skm.count("skm_round_of(const u32 H, const u32 R) { return (((H >> 4) & 0xffffu) * R) >> 16; }") == 1
    assert skm.count("skm_round_of(H, R) != q") == 2 and skm.count("((H >> 4) & 0xffffu) * R) >> 16") == 1
    assert "((h >> 4) & 0xffffu) * R) >> 16 == q" in skm
    assert "k_union_hash<512, 4096>" in ker and "constexpr u32 T2 = T / 8;" in ker
    assert "KH_PROBE_ROUNDS(ovf, T2 - 1u, T2)" in ker and "KH_PROBE_ROUNDS(tbl, T - 1u, T)" in ker


@pytest.mark.parametrize("k", UNION_K)
def test_deep_family_preconditions(k):
    m = minimizer_len(k)
    for ns in (1, 7, 1000, 500_000):
        assert slot_of(0, ns) == 0
    for name, (fam, lo, homes) in deep_families(k).items():
        assert len(set(fam)) == len(fam)
        keys, counts = CO.count("N".join(fam).encode(), k).arrays()
        assert sorted(int(x) for x in keys[:, 0]) == sorted(code_of(s) for s in fam)   # canonical as written
        assert (counts == 1).all()
        assert {minimizer(s, m) for s in fam} == {0}                                    # slot 0
        hs = [key_hash(code_of(s)) for s in fam]
        assert all((home(h) - lo) % SKM_T < homes for h in hs)
        if name == "same_hash":     # one home and one chain: the chain fills while the second table does not
            assert len(set(hs)) == 1 and len({chain(h) for h in hs}) == 1
            assert len(fam) > SKM_FULL_ROUNDS + SKM_CHAIN + 40
        else:                       # more than the span, the main rounds and the whole second table hold
            assert len(fam) >= homes + (SKM_FULL_ROUNDS - 1) + SKM_T2 + MARGIN
        if name == "wrap":
            assert any(home(h) == SKM_T - 1 for h in hs)
        if name == "zero":
            assert code_of(fam[0]) == 0 and home(key_hash(0)) == 0
    seqs, _ = deep_case(k)
    fam = set(family_keys(k))
    lo_half = {s for g in range(32) for s in records_of(seqs, g)}
    hi_half = {s for g in range(32, 40) for s in records_of(seqs, g)}
    assert len(fam & lo_half & hi_half) > 10 and len(fam & hi_half) > 40      # identical records in both halves
    rep_rc = rep_two = 0
    for g in range(len(seqs)):
        recs = set(records_of(seqs, g))
        rep_rc += sum(1 for s in fam if s in recs and revcomp(s) in recs)
        rep_two += sum(1 for s in fam if s in recs and two_kmer(s) in recs)
    assert rep_rc > len(fam) // 3 and rep_two > len(fam) // 5
    assert instances(seqs, k) <= 3072 and sum(len(records_of(seqs, g)) for g in range(40)) <= 1024 - 112


def test_two_round_preconditions():
    k, m = 31, minimizer_len(31)
    fam, fill, (seqs, _) = two_round_case()
    assert all(subset(key_hash(code_of(s)), 2) == 0 for s in fam)
    assert all((home(key_hash(code_of(s))) - (SKM_T - WRAP_HOMES)) % SKM_T < WRAP_HOMES for s in fam)
    assert len(fam) >= WRAP_HOMES + SKM_FULL_ROUNDS - 1 + SKM_T2 + MARGIN
    assert {minimizer(s, m) for s in fam} == {0}
    for r in fill:
        assert len(r) - k + 1 == k - m + 1
        assert {minimizer(r[j:j + k], m) for j in range(len(r) - k + 1)} == {0}
    assert SKM_T < instances(seqs, k) <= 6144                                   # R = 2
    chunks = sum((max(0, len(r) - k + 1) + 1) // 2 for g in range(40) for r in records_of(seqs, g))
    assert chunks <= 3072 and sum(len(records_of(seqs, g)) for g in range(40)) <= 1024 - 112


def test_overflow_preconditions():
    k, m = 31, minimizer_len(31)
    recs = overflow_records()
    keys = set()
    for r in recs:
        assert minimizer(r[:k], m) == 0 and minimizer(r[7:7 + k], m) == 0      # A^m in the first and last window
        for j in range(8):
            c = canon_of(r[j:j + k])
            assert subset(key_hash(c), 2) == 0
            keys.add(c)
    assert len(keys) == 8 * len(recs) > SKM_T + SKM_T2 + 100 > PH_FULL
    assert 2 * PH_ROUND > 8 * len(recs) > PH_ROUND                               # R = 2 in all three kernels
    got = CO.count("N".join(recs).encode(), k).arrays()[0]
    assert sorted(int(x) for x in got[:, 0]) == sorted(keys)


@pytest.mark.parametrize("k", UH_K)
def test_top32_family_preconditions(k):
    top, codes = top32_family(k)
    assert len(set(codes)) == len(codes) > HASH_ROUNDS + UH_T2 + 100
    keys, _ = CO.count("N".join(decode(c, k) for c in codes).encode(), k).arrays()
    assert sorted(int(x) for x in keys[:, 0]) == sorted(codes)                  # canonical
    mixed = mix_np(k, np.array(codes, dtype=np.uint64).reshape(-1, 1))
    assert {int(t) for t in top32_np(k, mixed)} == {top}                        # one fine bin
    seqs, _ = top32_case(k)
    assert instances(seqs, k) <= 4096                                           # no capacity retry
    if k == 32:
        sc = special_code()
        assert int(mix_np(k, np.array([[sc]], dtype=np.uint64))[0, 0]) == (1 << 64) - 1
        assert sc > rc_code(sc, k) and sc not in codes                           # never a canonical key


# =========================================================================== GPU
KERNELS = ("skm_union", "skm_big", "skm_pack", "skm_phased", "union_tagged")


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
    return util.exp1_check(eng, capfd, seqs, group_of, k, expect, KERNELS, ("retries", "big_slots"))


UNION_ONLY = dict(skm_union=1, skm_big=0, skm_pack=0, skm_phased=0, union_tagged=0, retries=0, big_slots=0)
BIG = dict(skm_union=1, skm_big=1, skm_pack=0, skm_phased=0, union_tagged=0, retries=0, big_slots=(1, None))
FALLBACK = dict(skm_union=1, skm_pack=0, skm_phased=0, union_tagged=(1, None), retries=1)


@pytest.fixture
def skm_env(monkeypatch):
    monkeypatch.setenv("KHOICE_SKM_DEBUG", "1")
    return monkeypatch


# ---- A. k_skm_union: slot 0 within its region (a slack the planner clamps to the union's 1024 records)
@pytest.mark.gpu
@pytest.mark.parametrize("k", UNION_K)
def test_union_deep_tiers(eng, capfd, skm_env, k):
    """The wrap family (k = 32: the home-0 family with poly-A; k = 24: also the identical-H family) forces level 2 of
    the serial tail; the layout puts family keys in both mask halves, repeats them in other records of one genome
    and keeps identical records of the two halves apart."""
    skm_env.setenv("KHOICE_SKM_SLACK", "50")
    seqs, group_of = deep_case(k)
    for err in check(eng, capfd, seqs, group_of, k, UNION_ONLY):
        d = skm_line(err)
        assert (d["k"], d["m"]) == (k, minimizer_len(k))
        assert d["cap"] == 1024 and d["slot_max"] <= d["cap"] and d["overfull"] == 0 and d["errors"] == 0, d
        assert d["expanded"] <= SKM_T                                            # one round


@pytest.mark.gpu
def test_union_two_rounds(eng, capfd, skm_env):
    """R = 2 with the whole wrap family in subset 0: its level-2 walk runs in a table that was cleared for round 2."""
    skm_env.setenv("KHOICE_SKM_SLACK", "50")
    _, _, (seqs, group_of) = two_round_case()
    for err in check(eng, capfd, seqs, group_of, 31, UNION_ONLY):
        d = skm_line(err)
        assert d["cap"] == 1024 and d["overfull"] == 0 and SKM_T < d["expanded"] <= 2 * SKM_T, d


@pytest.mark.gpu
def test_union_subset_overflow(eng, capfd, skm_env):
    """More than T + T2 distinct keys in one subset of an R = 2 slot: the level-2 exit raises KH_ERR_CAPACITY, the
    call is retried once in the key-array form, and the answer is exact."""
    skm_env.setenv("KHOICE_SKM_SLACK", "50")
    seqs, group_of = overflow_case(40, 10)
    for err in check(eng, capfd, seqs, group_of, 31, dict(FALLBACK, skm_big=0, big_slots=0)):
        d = skm_line(err)
        assert d["cap"] == 1024 and d["overfull"] == 0 and d["errors"] != 0, d


# ---- B. k_skm_big: the same inputs with slot 0 above its region
@pytest.mark.gpu
@pytest.mark.parametrize("k", [24, 31, 32])
def test_big_deep_tiers(eng, capfd, skm_env, k):
    skm_env.setenv("KHOICE_SKM_SLACK", "0.3")
    seqs, group_of = deep_case(k)
    for err in check(eng, capfd, seqs, group_of, k, BIG):
        d = skm_line(err)
        assert d["overfull"] >= 1 and d["slot_max"] > d["cap"] and d["errors"] == 0, d


@pytest.mark.gpu
@pytest.mark.parametrize("big_y", [1, 2, 16])
def test_big_two_rounds(eng, capfd, skm_env, big_y):
    """two_round_case with slot 0 above its region: 4096 < N <= 6144 instances (test_two_round_preconditions) are R = 2
    rounds of k_skm_big's 3072, and no subset outgrows the tables: the slot is completed, no fall-back.  The rounds are
    shared out over KHOICE_SKM_BIG_Y workgroups: with 1 one workgroup clears the table between its two rounds, with 2
    each runs one, with 16 fourteen have no round and only flush."""
    skm_env.setenv("KHOICE_SKM_SLACK", "0.3")
    skm_env.setenv("KHOICE_SKM_BIG_Y", str(big_y))
    _, _, (seqs, group_of) = two_round_case()
    for err in check(eng, capfd, seqs, group_of, 31, BIG):
        d = skm_line(err)
        assert d["overfull"] >= 1 and d["slot_max"] > d["cap"] and d["errors"] == 0, d


@pytest.mark.gpu
def test_big_subset_overflow(eng, capfd, skm_env):
    """k_skm_big takes R = ceil(N / 3072) = 2 rounds: every key in subset 0, more than both tables hold."""
    skm_env.setenv("KHOICE_SKM_SLACK", "0.3")
    seqs, group_of = overflow_case(40, 10)
    for err in check(eng, capfd, seqs, group_of, 31, dict(FALLBACK, skm_big=1)):
        d = skm_line(err)
        assert d["overfull"] >= 1, d


# ---- C. k_skm_phased: one group of 70 genomes, sub-batches of 24 / 23 / 23 as phases.  The families come with a
# related background of 10 kb per genome: the one-GPU pack puts a phase's records through 64 cursors of part_cap / 64
# records each, and the family alone would overflow the cursor of slot 0 (the call then declines the phased form).
# The background is nearly the same in every genome, so identical records merge and slot 0 stays at one round.
PHASED = dict(skm_pack=3, skm_phased=1, union_tagged=0, retries=0)


def with_background(case, seed):
    seqs, group_of = case
    bg, _ = random_genomes(len(seqs), 10_000, seed, related=True)
    return [b + b"N" + s for b, s in zip(bg, seqs)], group_of


def random_genomes(n, length, seed, related):
    """n genomes: independent random sequence, or copies of one ancestor with one substitution per 1000 bases."""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"ACGT", dtype=np.uint8)
    anc = rng.integers(0, 4, size=length)
    out = []
    for _ in range(n):
        g = anc.copy() if related else rng.integers(0, 4, size=length)
        if related:
            at = rng.integers(0, length, size=length // 1000)
            g[at] = (g[at] + rng.integers(1, 4, size=at.size)) % 4
        out.append(alpha[g].tobytes())
    return out, [0] * n


@pytest.mark.gpu
def test_phased_deep_tiers(eng, capfd, skm_env):
    """The k = 31 wrap family over 70 genomes: its keys come in all three phases, and the second-table entries fold
    their masks into their counters phase by phase."""
    seqs, group_of = with_background(deep_case(31, 70, 70), 43)
    for err in check(eng, capfd, seqs, group_of, 31, PHASED):
        assert "70 genomes in 3 phases" in err and "overfilled" not in err and "overflowed" not in err, err


@pytest.mark.gpu
def test_phased_optimistic_novelty_unrelated(eng, capfd, skm_env):
    """KHOICE_SKM_PHASED_NOVELTY=0.05 sizes rounds for sub-batches that share nearly everything; unrelated genomes
    overfill a table, and the host launches the phased union once more with rounds for unrelated pieces."""
    skm_env.setenv("KHOICE_SKM_PHASED_NOVELTY", "0.05")
    seqs, group_of = random_genomes(70, 20_000, 41, related=False)
    for err in check(eng, capfd, seqs, group_of, 31, dict(PHASED, skm_phased=2, retries=1)):
        assert "[skm phased] a table overfilled" in err and "overflowed" not in err, err


@pytest.mark.gpu
def test_phased_optimistic_novelty_related(eng, capfd, skm_env):
    """The same knob with related sub-batches: the optimistic rounds hold, no second launch."""
    skm_env.setenv("KHOICE_SKM_PHASED_NOVELTY", "0.05")
    seqs, group_of = random_genomes(70, 20_000, 42, related=True)
    for err in check(eng, capfd, seqs, group_of, 31, PHASED):
        assert "70 genomes in 3 phases" in err and "overfilled" not in err, err


@pytest.mark.gpu
def test_phased_subset_overflow(eng, capfd, skm_env):
    """Every key of slot 0 in subset 0 of its two rounds, more than the fold's near-full check lets through, even with
    rounds for unrelated pieces: the phased union declines and the key-array sub-batches give the exact answer.  The
    pass by group (k_skm_union over the group's tag, for the across-group histogram) meets the same subset: its
    level-2 exit raises KH_ERR_CAPACITY, the one retry, and the key arrays take that pass too."""
    seqs, group_of = with_background(overflow_case(70, 70), 44)
    for err in check(eng, capfd, seqs, group_of, 31, dict(skm_pack=3, skm_phased=1, union_tagged=(1, None), retries=1)):
        assert "[skm phased] the phased union overflowed" in err, err


# ---- D. k_union_hash: the key-array form
@pytest.mark.gpu
@pytest.mark.parametrize("k", UH_K)
def test_union_hash_tier3(eng, capfd, monkeypatch, k):
    """More than 3 + 512 keys with one home: the second table fills and the rest probe the main table again."""
    monkeypatch.setenv("KHOICE_NO_SKM", "1")
    seqs, group_of = top32_case(k)
    check(eng, capfd, seqs, group_of, k, dict(skm_union=0, skm_big=0, skm_phased=0, union_tagged=(1, None), retries=0))
