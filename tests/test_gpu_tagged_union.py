"""The key-array form of the fused exp-1 step above pass C — k_union_tagged<W, false>, k_union_tagged<W, true>, the
read-out they share with k_union_hash (TagReadout, tag_slice, SlotBin, WaveGather) and the host logic around them
(exp1_fused, exp1_fused_rescaled, exp1_big_group, exp1_batches, exp1_batched, TagLayout, the key-range waves,
StatCheckpoint) — on constructed input, bit for bit against the C restatement (oracle.c_oracle).

Random genomes put some T keys of every genome into a slot, with T far below the capacity, a key or two into a fine
bin, and every genome mask into the low bits.  Here the inputs are built for what that leaves out:

  1. slots that gather exactly cap - 1, cap and cap + 1 elements (64 genomes x cap / 64 shared keys of ONE sub-range of
     one bucket): no retry up to cap, one retry with finer slots above it, both attempts lost when the keys share one
     fine bin, no second attempt above 16 / 1.15 x cap;
  2. one fine bin of a slot holding 1, 2, 3, 16 and 64 distinct keys whose copies arrive interleaved (find_leaders'
     later rounds), with keys that agree in one 64-bit word and differ in the other;
  3. genome masks with bit 63, bit 0, all bits, bits 31 | 32, every second bit, one bit per group and one whole group,
     under seven group layouts and five (cs, hist_len);
  4. the emitting form's look-back chain over empty slots (head, runs, tail), a slot that is one key 64 times, runs of
     64 equal elements across the 64-, 256- and 512-element boundaries of the sort;
  5. key-range waves that hold no key, more waves than buckets, an overfull slot in the last wave;
  6. the batch cutter at 64 | 65 genomes and 64 | 65 groups, groups of 65 .. 129 genomes at k = 15, 41, 63, 64;
  7. builds / bases / kmers / distinct of eng.stats() against the oracle's totals for every call a fused form completed.

All expected across-group sets are made in numpy from the per-genome databases of CO.count (union of the groups' key
sets, counter = groups holding the key, clamped at cs); the library's general path is never the reference.  The CPU
tests read the constants out of the sources and prove every construction on the oracle's keys (slot totals under the
engine's own S, distinct keys of the planted fine bins, empty slots and waves, the genome sets of the mask keys)."""
import functools
import math
import os
import re

import numpy as np
import pytest

from oracle import c_oracle as CO
from tests.util import (CAP, FINE_BITS, M32, MEAN, fine_bin_np, grid_sub_ranges, key_view, mix_np, mixed_from_top32,
                        planted_codes, planted_text, random_dna_np, revcomp_np, slot_np, top32_np, unmix_np, words)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "khoice_amd", "csrc")

# ---- constants of the layer (test_constants_match_sources reads them out of the sources)
TAG_MAX_OPS = 64                 # KH_TAG_MAX_OPS: width of the genome mask
TAG_MAX_BINS = 255               # KH_TAG_MAX_BINS
CAP_PAY = {1: 4096, 2: 2048}     # KH_SORT_CAP_PAY_W1 / _W2: elements a slot of k_union_tagged gathers
HASH_CAP = 4096                  # kh_union_hash_capacity()
FINE_BINS = 1 << FINE_BITS
RETRY_GROWTH, RETRY_LIMIT = 1.15, 16.0      # exp1_fused's finer-slots factor, exp1_fused_rescaled's bound
BIG = 1 << 30                    # a counter ceiling nothing here reaches
ENV_NAMES = ("KHOICE_NO_SKM", "KHOICE_NO_UNION_HASH", "KHOICE_WAVE_BASES", "KHOICE_NO_FUSED", "KHOICE_NO_SKM2",
             "KHOICE_NO_SKM_TWO_PASS", "KHOICE_SKM_MIN_K", "KHOICE_NO_BMP", "KHOICE_TILE_POS", "KHOICE_DIRECT_SCATTER")
NO_SKM = {"KHOICE_NO_SKM": "1"}
# name -> (k, environment, emitting): the four forms (the emitting one for both key widths)
FORMS = {
    "w2": (41, NO_SKM, False),                                          # k_union_tagged<2, false>
    "fine1": (31, {**NO_SKM, "KHOICE_NO_UNION_HASH": "1"}, False),      # k_union_tagged<1, false>
    "hash1": (31, NO_SKM, False),                                       # k_union_hash
    "emit1": (31, NO_SKM, True),                                        # k_union_tagged<1, true>
    "emit2": (41, NO_SKM, True),                                        # k_union_tagged<2, true>
}
PAIRS = ((5000, 80), (2, 5), (1, 2), (64, 65), (63, 64))                # (cs, hist_len)


def _src(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def test_constants_match_sources():
    com, ker, lau, eng = _src("kh_common.h"), _src("kh_kernels.hip"), _src("kh_launch.h"), _src("kh_engine.cpp")

    def num(pattern, text):
        return int(re.search(pattern, text).group(1))
    assert num(r"constexpr int KH_TAG_MAX_OPS = (\d+);", lau) == TAG_MAX_OPS
    assert num(r"constexpr int KH_TAG_MAX_BINS = (\d+);", lau) == TAG_MAX_BINS
    assert num(r"constexpr int KH_SORT_CAP_PAY_W1 = (\d+);", com) == CAP_PAY[1]
    assert num(r"constexpr int KH_SORT_CAP_PAY_W2 = (\d+);", com) == CAP_PAY[2]
    assert CAP_PAY == CAP                                               # grid_sub_ranges (tests/util.py) leans on it
    assert num(r"u32 kh_union_hash_capacity\(\) \{ return (\d+)u; \}", ker) == HASH_CAP
    assert num(r"#define KH_TUNE_FINE_BITS (\d+)", com) == FINE_BITS
    assert "constexpr int KH_FINE_BITS = KH_TUNE_FINE_BITS;" in com and "constexpr int KH_FINE_BINS = 1 << KH_FINE_BITS;" in com
    assert num(r"#define KH_TUNE_MEAN_W1 (\d+)", com) == MEAN[1]
    assert num(r"constexpr int KH_BUCKET_MEAN_W2 = (\d+);", com) == MEAN[2]
    # the retry: 1.15 x (fullest slot / capacity) more sub-ranges, once, below 16
    assert "*want_scale = s_scale * 1.15 * (double)h_ctl[1] / (double)gb.cap;" in eng
    assert "if (scale > 1.0 && scale < 16.0) {" in eng
    assert (RETRY_GROWTH, RETRY_LIMIT) == (1.15, 16.0)
    # what geometry(), sub_of() and union_bin() below restate
    assert "gb.cap = hash_form ? kh_union_hash_capacity() : (W == 1 ? KH_SORT_CAP_PAY_W1 : KH_SORT_CAP_PAY_W2);" in eng
    assert "const double zg = 5.0 * std::sqrt((double)std::max<u32>(1, grid->fan));" in eng
    assert "const u64 target = std::max<u64>(16, std::min<u64>((u64)grid->cap * 92 / 100, (u64)(x * x)));" in eng
    assert "const u64 per_bucket = (total_pos + grid_nb * nwaves - 1) / (grid_nb * nwaves);" in eng
    assert "grid->S = (u32)std::max<u64>(1, (u64)std::ceil((double)((per_bucket + target - 1) / target) * grid->s_scale));" in eng
    assert "if (lens[i] >= (u64)k) grid_nb = std::max<u64>(grid_nb, (lens[i] - k + 1 + per - 1) / per);" in eng
    assert "s.b_first = grid ? grid->wave * (u32)want_b : 0u;" in eng
    assert "job.binmul = (1u << 26) / ((KH_FINE_BINS + gb.S - 1) / gb.S);" in eng and "job.nbv = gb.nb * nwaves;" in eng
    assert "return (fine_bin<W>(key, k, nb) * S) >> KH_FINE_BITS;" in ker
    assert "kh_first_bin(u32 f, u32 S) { return (f * (u32)KH_FINE_BINS + S - 1u) / S; }" in ker
    assert "const u32 fb = (u32)(((u64)(frac - rel0) * (u64)binmul) >> 32);" in ker
    assert "if (n64 <= (u64)limit) return (u32)n64;" in ker
    assert "static u32 exp1_waves(u64 bases, u64 budget) { return (u32)std::max<u64>(1, (bases + budget - 1) / budget); }" in eng
    assert "(acc_b + gbases[g] <= budget || acc_n == 0);" in eng and "gb.fan = std::max(L.fan, fan_hint);" in eng
    assert "for (size_t i0 = 0; i0 < all.idx.size(); i0 += KH_TAG_MAX_OPS) {" in eng


# =========================================================================== the engine's slot geometry, restated
def geometry(k, lens, fan, nwaves=1, scale=1.0):
    """(buckets of one wave's grid, sub-ranges S per bucket) of a grid-mode build of texts of `lens` bases."""
    w = words(k)
    cap = CAP_PAY[w]
    npos = [max(0, n - k + 1) for n in lens]
    per = MEAN[w] * nwaves
    gnb = max([1] + [-(-p // per) for p in npos])
    zg = 5.0 * math.sqrt(max(1, fan))
    x = 0.5 * (-zg + math.sqrt(zg * zg + 4.0 * cap))
    target = max(16, min(cap * 92 // 100, int(x * x)))
    per_bucket = -(-sum(npos) // (gnb * nwaves))
    return gnb, max(1, math.ceil(float(-(-per_bucket // target)) * scale))


def retry_scale(fullest, cap):
    return 1.0 * 1.15 * float(fullest) / float(cap)


def first_bin(f, s_ranges):
    return (f * FINE_BINS + s_ranges - 1) // s_ranges


def union_bin_top(top, nbv, s_ranges):
    """(bucket, sub-range, in-slot fine bin of the union kernels: SlotBin) of keys given by the top 32 bits of their
    mixed form; nbv: buckets over all waves."""
    prod = np.asarray(top, dtype=np.uint64) * np.uint64(nbv)
    b = (prod >> np.uint64(32)).astype(np.int64)
    frac = (prod & np.uint64(M32)).astype(np.int64)
    f = ((frac >> (32 - FINE_BITS)) * s_ranges) >> FINE_BITS
    rel0 = ((f * FINE_BINS + s_ranges - 1) // s_ranges) << (32 - FINE_BITS)
    binmul = (1 << 26) // (-(-FINE_BINS // s_ranges))
    return b, f, np.minimum(((frac - rel0) * binmul) >> 32, FINE_BINS - 1)


def union_bin(k, keys, nbv, s_ranges):
    return union_bin_top(top32_np(k, mix_np(k, keys)), nbv, s_ranges)


def canonical(k, codes):
    rc = revcomp_np(k, codes)
    if words(k) == 1:
        return codes[:, 0] <= rc[:, 0]
    return (codes[:, 1] < rc[:, 1]) | ((codes[:, 1] == rc[:, 1]) & (codes[:, 0] <= rc[:, 0]))


def distinct_keys(keys):
    return np.unique(key_view(keys)).shape[0] == keys.shape[0]


def keys_in_sub(k, nbv, s_ranges, b, f, n, rng):
    """n distinct canonical keys of sub-range f of bucket b, spread over its fine bins, ascending in mixed key."""
    got = planted_codes(k, nbv, b, None, 3 * n * s_ranges + 400, rng, FINE_BITS)
    fine = fine_bin_np(k, mix_np(k, got), nbv, FINE_BITS).astype(np.int64)
    got = got[((fine * s_ranges) >> FINE_BITS) == f][:n]
    assert got.shape[0] == n, (got.shape[0], n)
    return got[np.argsort(key_view(mix_np(k, got)), kind="stable")]


# =========================================================================== a case: texts, groups, oracle answers
class Case:
    """Genome texts with their groups, and everything the oracle says about them (computed once, never changed)."""

    def __init__(self, k, seqs, group_of, **info):
        self.k, self.w, self.seqs, self.group_of = k, words(k), tuple(seqs), [int(g) for g in group_of]
        self.ngroups = max(self.group_of) + 1
        self.info = info
        self._exp1, self._across = {}, {}

    @functools.cached_property
    def counted(self):
        dbs = [CO.count(s, self.k, cs=BIG) for s in self.seqs]
        return [d.arrays()[0] for d in dbs], sum(d.kmers for d in dbs)

    @property
    def dbs(self):
        """Per genome: its distinct k-mers keys[n, W]."""
        return self.counted[0]

    def oracle(self, cs, hl):
        if (cs, hl) not in self._exp1:
            self._exp1[cs, hl] = CO.exp1(list(self.seqs), self.group_of, self.k, cs=cs, hist_len=hl)
        return self._exp1[cs, hl]

    @functools.cached_property
    def totals(self):
        """What eng.stats() must have moved by after a completed fused call: builds, bases, kmers, distinct."""
        return {"builds": len(self.seqs), "bases": sum(len(s) for s in self.seqs), "kmers": int(self.counted[1]),
                "distinct": int(sum(d.shape[0] for d in self.dbs))}

    def across(self, cs):
        """(keys[n, W] sorted by k-mer, counters): the union of the groups' key sets, counter = groups holding the key."""
        if "raw" not in self._across:
            per_group = []
            for g in range(self.ngroups):
                mine = [key_view(self.dbs[i]) for i in range(len(self.seqs)) if self.group_of[i] == g]
                per_group.append(np.unique(np.concatenate(mine)))
            v, n = np.unique(np.concatenate(per_group), return_counts=True)
            keys = np.empty((v.shape[0], self.w), dtype=np.uint64)
            if self.w == 1:
                keys[:, 0] = v
            else:
                keys[:, 0], keys[:, 1] = v["lo"], v["hi"]
            self._across["raw"] = (keys, n.astype(np.int64))
        keys, n = self._across["raw"]
        return keys, np.minimum(n, cs).astype(np.uint32)

    def slot_totals(self, nbv, s_ranges):
        """Elements every slot (bucket x sub-range) of the tagged union gathers: the genomes' distinct keys in it."""
        tot = np.zeros(nbv * s_ranges, dtype=np.int64)
        for keys in self.dbs:
            if keys.shape[0]:
                mixed = mix_np(self.k, keys)
                b = slot_np(self.k, mixed, nbv).astype(np.int64)
                f = (fine_bin_np(self.k, mixed, nbv, FINE_BITS).astype(np.int64) * s_ranges) >> FINE_BITS
                tot += np.bincount(b * s_ranges + f, minlength=tot.shape[0])
        return tot

    def lens(self):
        return [len(s) for s in self.seqs]


def texts_of(k, ngenomes, held, npos, rng):
    """held: [(keys[n, W], genomes)] -> one text of npos k-mer positions per genome with the keys it holds."""
    per = [[] for _ in range(ngenomes)]
    for keys, genomes in held:
        for g in genomes:
            per[g].append(keys)
    out = []
    for g in range(ngenomes):
        keys = np.concatenate(per[g]) if per[g] else np.zeros((0, words(k)), dtype=np.uint64)
        assert distinct_keys(keys)
        out.append(planted_text(k, keys, np.ones(keys.shape[0], dtype=np.int64), npos, rng))
    return out


def groups_of(sizes):
    return [g for g, n in enumerate(sizes) for _ in range(n)]


# =========================================================================== 1. slot fill at the capacity
NB_TEXT = 4            # buckets of a genome's text in the 64-genome cases
FILL_ODD = 5           # the genome that holds one key fewer / more
HUGE = 446             # keys per genome of the slot no retry is tried for: 64 x 446 > 16 / 1.15 x 2048 = 28494


@functools.lru_cache(maxsize=None)
def fill_case(k, kind, nwaves=1, fan=32):
    """64 genomes in 64 / fan groups that all hold the same D = cap / 64 keys of ONE sub-range of one bucket (the last
    bucket of the last wave).  kind: 'cap-1' / 'cap' / 'cap+1' (genome FILL_ODD holds one key fewer / more; the keys
    are spread over the sub-range's fine bins), 'one_bin' (D + 1 keys of one fine bin in every genome: 64 more than
    fit, in a bin no finer slot can split) or 'huge' (HUGE keys in every genome: above 16 / 1.15 x cap)."""
    w = words(k)
    cap = CAP_PAY[w]
    nper = cap // TAG_MAX_OPS
    nb_text = NB_TEXT if kind != "huge" else -(-(HUGE * (k + 1) + k) // MEAN[w])
    npos = nb_text * MEAN[w]
    lens = [npos + k - 1] * TAG_MAX_OPS
    gnb, s_ranges = geometry(k, lens, fan, nwaves)
    nbv = gnb * nwaves
    b, f = nbv - 1, s_ranges // 2
    rng = np.random.default_rng(1000 + 7 * k + nwaves + fan)
    everyone = range(TAG_MAX_OPS)
    if kind == "one_bin":
        fine = (first_bin(f, s_ranges) + first_bin(f + 1, s_ranges)) // 2
        held = [(planted_codes(k, nbv, b, fine, nper + 1, rng, FINE_BITS), everyone)]
    elif kind == "huge":
        held = [(keys_in_sub(k, nbv, s_ranges, b, f, HUGE, rng), everyone)]
    else:
        keys = keys_in_sub(k, nbv, s_ranges, b, f, nper + 1, rng)
        shared, extra = keys[:nper], keys[nper:]
        if kind == "cap":
            held = [(shared, everyone)]
        elif kind == "cap-1":
            held = [(shared[1:], everyone), (shared[:1], [g for g in everyone if g != FILL_ODD])]
        else:
            held = [(shared, everyone), (extra, [FILL_ODD])]
    seqs = texts_of(k, TAG_MAX_OPS, held, npos, rng)
    return Case(k, seqs, groups_of([fan] * (TAG_MAX_OPS // fan)), nbv=nbv, S=s_ranges, slot=b * s_ranges + f, nwaves=nwaves,
                fan=fan, gnb=gnb)


FILL_KINDS = {"cap-1": -1, "cap": 0, "cap+1": 1}


@pytest.mark.parametrize("k", (31, 41))
def test_fill_case_preconditions(k):
    cap = CAP_PAY[words(k)]
    for nwaves, fan in ((1, 32), (3, 32), (3, 64)):
        for kind, d in FILL_KINDS.items():
            c = fill_case(k, kind, nwaves, fan)
            nbv, s_ranges = c.info["nbv"], c.info["S"]
            assert (c.info["gnb"], s_ranges) == geometry(k, c.lens(), fan, nwaves)
            if nwaves == 1:      # the engine's S as the sibling module restates it, for both capacities of one-word keys
                assert nbv == NB_TEXT and s_ranges == grid_sub_ranges(k, TAG_MAX_OPS, fan, True) == grid_sub_ranges(k, TAG_MAX_OPS, fan, False)
            tot = c.slot_totals(nbv, s_ranges)
            assert tot[c.info["slot"]] == cap + d and tot.sum() == cap + d            # every other slot is empty
            assert c.info["slot"] // s_ranges // c.info["gnb"] == nwaves - 1          # the slot is in the last wave
            if d == 1:           # the finer slots of the one retry hold it
                s2 = geometry(k, c.lens(), fan, nwaves, retry_scale(cap + 1, cap))[1]
                assert s2 > s_ranges and retry_scale(cap + 1, cap) < RETRY_LIMIT
                assert 0 < c.slot_totals(nbv, s2).max() <= cap
    c = fill_case(k, "one_bin")
    tot = c.slot_totals(c.info["nbv"], c.info["S"])
    fullest = 64 * (cap // 64 + 1)
    assert tot.max() == tot.sum() == fullest == cap + 64
    s2 = geometry(k, c.lens(), 32, 1, retry_scale(fullest, cap))[1]
    assert s2 > c.info["S"] and retry_scale(fullest, cap) < RETRY_LIMIT
    assert c.slot_totals(c.info["nbv"], s2).max() == fullest                          # one fine bin: no S splits it
    for c2 in (c, fill_case(k, "cap+1")):
        assert sum(len(s) for s in c2.seqs) < 1_000_000


def test_huge_fill_case_preconditions():
    k = 33
    c = fill_case(k, "huge")
    tot = c.slot_totals(c.info["nbv"], c.info["S"])
    assert tot.max() == tot.sum() == 64 * HUGE
    assert retry_scale(64 * HUGE, CAP_PAY[2]) >= RETRY_LIMIT and 64 * HUGE > RETRY_LIMIT / RETRY_GROWTH * CAP_PAY[2]
    assert retry_scale(64 * (HUGE - 1), CAP_PAY[2]) < RETRY_LIMIT            # the smallest such slot of 64 equal genomes
    assert sum(len(s) for s in c.seqs) < 1_050_000


# =========================================================================== 2. leader search and key compare
LEAD_GENOMES, LEAD_GROUPS = 16, [4, 4, 4, 4]
LEAD_K = (31, 64)          # one-word fine-bin form; two-word keys whose top 32 bits leave 32 bits of the high word free


def bin_tops(nbv, s_ranges, b, f, where):
    """(in-slot fine bin j, every top-32 value of it) for the first / a middle / the last fine bin of slot (b, f)."""
    width = -(-FINE_BINS // s_ranges)
    binmul = (1 << 26) // width
    span = (first_bin(f + 1, s_ranges) - first_bin(f, s_ranges)) << (32 - FINE_BITS)
    last = min(((span - 1) * binmul) >> 32, FINE_BINS - 1)
    j = {"first": 0, "mid": last // 2, "last": last}[where]
    rel0 = first_bin(f, s_ranges) << (32 - FINE_BITS)
    lo, hi = -(-(j << 32) // binmul), min(span, -(-((j + 1) << 32) // binmul))
    p = (np.uint64(b) << np.uint64(32)) + np.uint64(rel0) + np.arange(lo, hi, dtype=np.uint64)
    top = np.unique((p + np.uint64(nbv - 1)) // np.uint64(nbv))
    top = top[top <= np.uint64(M32)]
    bb, ff, jj = union_bin_top(top, nbv, s_ranges)
    return j, top[(bb == b) & (ff == f) & (jj == j)]


def craft_bin(k, tops, n, rng):
    """n distinct canonical keys whose top 32 mixed bits are among `tops`: half of them share ONE top-32 value; for
    two-word keys also pairs that agree in the low word and differ in the high one, and the other way round."""
    w = words(k)

    def fresh(t):
        mixed = mixed_from_top32(k, np.asarray(t, dtype=np.uint64), rng)
        return mixed

    def keep(mixed, group):
        """rows of `mixed` in groups of `group` consecutive rows: the groups that are canonical throughout"""
        ok = canonical(k, unmix_np(k, mixed)).reshape(-1, group).all(axis=1)
        return mixed.reshape(-1, group, w)[ok].reshape(-1, w)
    out = []
    if w == 2 and n >= 2:
        npairs = 1 if n < 16 else 2
        cand = fresh(tops[rng.integers(0, tops.shape[0], size=64)])
        if n != 3:                                  # same low word, other high word (same top 32 bits: the same bin)
            a = np.repeat(cand[:32], 2, axis=0)
            a[1::2, 1] ^= rng.integers(1, 1 << 31, size=32, dtype=np.uint64)
            out.append(keep(a, 2)[:2 * npairs])
        if n >= 3:                                  # same high word, other low word
            a = np.repeat(cand[32:], 2, axis=0)
            a[1::2, 0] ^= rng.integers(1, 1 << 31, size=32, dtype=np.uint64)
            out.append(keep(a, 2)[:2 * npairs])
    have = sum(a.shape[0] for a in out)
    family = min(n - have, max(1, n // 2))
    out.append(keep(fresh(np.full(8 * family + 32, tops[rng.integers(0, tops.shape[0])])), 1)[:family])
    rest = n - have - family
    out.append(keep(fresh(tops[rng.integers(0, tops.shape[0], size=8 * rest + 32)]), 1)[:rest])
    mixed = np.concatenate(out)
    assert mixed.shape[0] == n and distinct_keys(mixed), (mixed.shape[0], n)
    return unmix_np(k, mixed)


def lead_plan(s_ranges, gnb):
    """(bucket, sub-range, which fine bin of the slot, distinct keys)"""
    return [(1, s_ranges // 2, "first", 64), (1, s_ranges // 2, "last", 16), (2, 1, "first", 3), (2, 1, "mid", 1),
            (2, 1, "last", 2), (gnb - 1, s_ranges - 1, "last", 64), (0, 0, "first", 16)]


@functools.lru_cache(maxsize=None)
def leader_case(k):
    """16 genomes in four groups; planted fine bins of 1, 2, 3, 16 and 64 distinct keys, every key held by another
    non-empty subset of the genomes, so that copies of different keys arrive interleaved in the bin."""
    w = words(k)
    nb_text = 4 if w == 1 else 8
    npos = nb_text * MEAN[w]
    lens = [npos + k - 1] * LEAD_GENOMES
    gnb, s_ranges = geometry(k, lens, max(LEAD_GROUPS))
    rng = np.random.default_rng(2000 + k)
    held, bins = [], []
    for b, f, where, n in lead_plan(s_ranges, gnb):
        j, tops = bin_tops(gnb, s_ranges, b, f, where)
        keys = craft_bin(k, tops, n, rng)
        subsets = rng.choice(np.arange(1, 1 << LEAD_GENOMES), size=n, replace=False)
        for i in range(n):
            held.append((keys[i:i + 1], [g for g in range(LEAD_GENOMES) if (int(subsets[i]) >> g) & 1]))
        bins.append((b, f, j, n))
    seqs = texts_of(k, LEAD_GENOMES, held, npos, rng)
    return Case(k, seqs, groups_of(LEAD_GROUPS), nbv=gnb, S=s_ranges, bins=bins)


@pytest.mark.parametrize("k", LEAD_K)
def test_leader_case_preconditions(k):
    c = leader_case(k)
    nbv, s_ranges = c.info["nbv"], c.info["S"]
    assert (nbv, s_ranges) == geometry(k, c.lens(), 4) and s_ranges == grid_sub_ranges(k, LEAD_GENOMES, 4, False)
    assert c.slot_totals(nbv, s_ranges).max() <= CAP_PAY[c.w] // 2
    keys, _ = c.across(BIG)
    b, f, j = union_bin(k, keys, nbv, s_ranges)
    where = (b * s_ranges + f) * FINE_BINS + j
    ids, n = np.unique(where, return_counts=True)
    want = {(bb * s_ranges + ff) * FINE_BINS + jj: nn for bb, ff, jj, nn in c.info["bins"]}
    assert dict(zip(ids.tolist(), n.tolist())) == want and sorted(want.values()) == [1, 2, 3, 16, 16, 64, 64]
    # the first fine bin of a slot and the last: of the first slot, of a middle one, of the last slot of the grid
    width = -(-FINE_BINS // s_ranges)
    for bb, ff, jj, nn in c.info["bins"]:
        span = first_bin(ff + 1, s_ranges) - first_bin(ff, s_ranges)
        assert jj in (0, (((span << 19) - 1) * ((1 << 26) // width)) >> 32, ((((span << 19) - 1) * ((1 << 26) // width)) >> 32) // 2)
    assert {(bb, ff) for bb, ff, _, _ in c.info["bins"]} >= {(0, 0), (nbv - 1, s_ranges - 1)}
    # copies interleave: in a planted bin the genomes hold different subsets of its keys
    for bb, ff, jj, nn in c.info["bins"]:
        if nn >= 3:
            sel = key_view(keys[where == (bb * s_ranges + ff) * FINE_BINS + jj])
            holders = np.array([np.isin(sel, key_view(d)) for d in c.dbs])                   # [genome, key]
            assert len({tuple(col) for col in holders.T.tolist()}) == nn and holders.any(axis=0).all()
            mixed = mix_np(k, keys[where == (bb * s_ranges + ff) * FINE_BINS + jj])
            tops, per_top = np.unique(top32_np(k, mixed), return_counts=True)
            assert per_top.max() >= nn // 2                                                   # a family sharing the top 32 bits
            if c.w == 2:
                lo, hi = mixed[:, 0], mixed[:, 1]
                same_lo = sum(1 for a in range(nn) for z in range(a) if lo[a] == lo[z] and hi[a] != hi[z])
                same_hi = sum(1 for a in range(nn) for z in range(a) if hi[a] == hi[z] and lo[a] != lo[z])
                assert same_hi >= 1 and (same_lo >= 1 or nn == 3)


# =========================================================================== 3. masks and read-out
LAYOUTS = {"64": [64], "1x64": [1] * 64, "1_62_1": [1, 62, 1], "32_32": [32, 32], "63_1": [63, 1], "1_63": [1, 63],
           "mixed": [1, 2, 30, 7, 24]}


def layout_groups(name):
    group_of = groups_of(LAYOUTS[name])
    if name == "mixed":        # callers need not pass groups in order
        group_of = [group_of[i] for i in np.random.default_rng(64).permutation(64)]
    return group_of


def mask_families(name):
    """[(keys of the family, genomes that hold them)]: the number of keys tells the families apart in a histogram."""
    group_of = layout_groups(name)
    ngroups = max(group_of) + 1
    members = [[i for i in range(64) if group_of[i] == g] for g in range(ngroups)]
    one_each = [m[(3 * g) % len(m)] for g, m in enumerate(members)]
    whole = members[ngroups // 2]
    return [(3, [63]), (4, [0]), (5, list(range(64))), (6, [31, 32]), (7, list(range(0, 64, 2))), (8, one_each), (9, whole)]


@functools.lru_cache(maxsize=None)
def mask_case(k, name):
    w = words(k)
    npos = NB_TEXT * MEAN[w]
    rng = np.random.default_rng(3000 + k + len(name))
    held = [(planted_codes(k, NB_TEXT, i % NB_TEXT, None, n, rng, FINE_BITS), genomes)
            for i, (n, genomes) in enumerate(mask_families(name))]
    return Case(k, texts_of(k, 64, held, npos, rng), layout_groups(name))


def closed_form(name, cs, hl):
    """The histograms and distinct counts of a mask case from the design alone."""
    group_of = layout_groups(name)
    ngroups = max(group_of) + 1
    within, across = np.zeros((ngroups, hl), dtype=np.uint64), np.zeros(hl, dtype=np.uint64)
    distinct = np.zeros(64, dtype=np.uint64)
    for n, genomes in mask_families(name):
        per = np.bincount([group_of[i] for i in genomes], minlength=ngroups)
        for g in np.nonzero(per)[0]:
            within[g, min(int(per[g]), cs, hl - 1)] += np.uint64(n)
        across[min(int((per > 0).sum()), cs, hl - 1)] += np.uint64(n)
        distinct[genomes] += np.uint64(n)
    return within, across, distinct


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_mask_case_preconditions(name):
    group_of = layout_groups(name)
    assert sorted(np.bincount(group_of).tolist()) == sorted(LAYOUTS[name]) and len(group_of) == 64
    fam = mask_families(name)
    assert [g for _, g in fam[:5]] == [[63], [0], list(range(64)), [31, 32], list(range(0, 64, 2))]
    assert sorted(group_of[i] for i in fam[5][1]) == list(range(max(group_of) + 1))          # one genome of every group
    assert len(set(group_of[i] for i in fam[6][1])) == 1 and len(fam[6][1]) == group_of.count(group_of[fam[6][1][0]])
    if name != "mixed":
        assert group_of == sorted(group_of)          # the genome's number is its bit of the mask: bit 63 is set
    for k in (31, 41):
        c = mask_case(k, name)
        # the genome sets of the planted keys, from the oracle's keys
        keys, _ = c.across(BIG)
        holders = np.array([np.isin(key_view(keys), key_view(d)) for d in c.dbs])           # [genome, key]
        sets = sorted((tuple(np.nonzero(col)[0].tolist()) for col in holders.T), key=lambda t: (len(t), t))
        want = sorted((tuple(sorted(g)) for n, g in fam for _ in range(n)), key=lambda t: (len(t), t))
        assert sets == want
        for cs, hl in PAIRS:
            w, a, d = closed_form(name, cs, hl)
            o = c.oracle(cs, hl)
            assert (o["within_hist"] == w).all() and (o["across_hist"] == a).all() and (o["distinct_per_seq"] == d).all()
        assert c.slot_totals(NB_TEXT, geometry(k, c.lens(), max(LAYOUTS[name]))[1]).max() < 400


# =========================================================================== 4. the emitting form
EMIT_K = (31, 32, 41, 64)
EMIT_LAYOUT = {31: [1] * 64, 32: [8] * 8, 41: [1] * 64, 64: [2] * 32}
RUN_STARTS = (40, 230, 490)      # sorted positions at which a run of 64 equal elements starts: it crosses 64, 256, 512


@functools.lru_cache(maxsize=None)
def emit_case(k):
    """64 genomes, four buckets.  Bucket 0: sub-ranges 0 .. 2 empty (the head of the chain), sub-range 3 = one key in all
    64 genomes, 4 and 5 empty, 6 / 8 / 10 = RUN_STARTS[i] single-genome keys, then a key of all 64 genomes, then ten
    single-genome keys.  Bucket 1 empty (a run of S empty slots).  Bucket 2: one sub-range of keys held by genomes
    0 .. 3 j (every counter from 1 up).  Bucket 3: one key in the middle, nothing behind it (the tail, the last slot)."""
    w = words(k)
    sizes = EMIT_LAYOUT[k]
    npos = NB_TEXT * MEAN[w]
    lens = [npos + k - 1] * 64
    gnb, s_ranges = geometry(k, lens, max(sizes))
    assert gnb == NB_TEXT and s_ranges > 12
    rng = np.random.default_rng(4000 + k)
    everyone = list(range(64))
    held = [(keys_in_sub(k, gnb, s_ranges, 0, 3, 1, rng), everyone)]
    used = {3}
    for i, start in enumerate(RUN_STARTS):
        f = 6 + 2 * i
        keys = keys_in_sub(k, gnb, s_ranges, 0, f, start + 11, rng)          # ascending in mixed key
        for j in list(range(start)) + list(range(start + 1, start + 11)):
            held.append((keys[j:j + 1], [(7 * j + i) % 64]))
        held.append((keys[start:start + 1], everyone))
        used.add(f)
    ramp = keys_in_sub(k, gnb, s_ranges, 2, s_ranges // 3, 21, rng)
    for j in range(21):
        held.append((ramp[j:j + 1], list(range(0, 3 * j + 1))))
    used.add(2 * s_ranges + s_ranges // 3)
    held.append((keys_in_sub(k, gnb, s_ranges, 3, s_ranges // 2, 1, rng), [9, 40]))
    used.add(3 * s_ranges + s_ranges // 2)
    return Case(k, texts_of(k, 64, held, npos, rng), groups_of(sizes), nbv=gnb, S=s_ranges, used=sorted(used))


@pytest.mark.parametrize("k", EMIT_K)
def test_emit_case_preconditions(k):
    c = emit_case(k)
    s_ranges = c.info["S"]
    assert (NB_TEXT, s_ranges) == geometry(k, c.lens(), max(EMIT_LAYOUT[k]))
    tot = c.slot_totals(NB_TEXT, s_ranges)
    assert np.nonzero(tot)[0].tolist() == c.info["used"]
    assert tot[:3].sum() == 0 and tot[4:6].sum() == 0 and tot[s_ranges:2 * s_ranges].sum() == 0      # head, middle, a whole bucket
    assert tot[3 * s_ranges + s_ranges // 2 + 1:].sum() == 0 and tot[-1] == 0 and tot.shape[0] == NB_TEXT * s_ranges
    assert tot[3] == 64 and tot.max() <= CAP_PAY[c.w] // 2
    assert [int(tot[6 + 2 * i]) for i in range(3)] == [start + 10 + 64 for start in RUN_STARTS]
    keys, _ = c.across(BIG)
    mixed = mix_np(k, keys)
    slot = slot_np(k, mixed, NB_TEXT).astype(np.int64) * s_ranges + \
        ((fine_bin_np(k, mixed, NB_TEXT, FINE_BITS).astype(np.int64) * s_ranges) >> FINE_BITS)
    nheld = np.array([np.isin(key_view(keys), key_view(d)) for d in c.dbs]).sum(axis=0)
    assert nheld[slot == 3].tolist() == [64]                                                # a slot that is one key 64 times
    for i, start in enumerate(RUN_STARTS):              # the run of 64 starts at sorted position `start` of its slot
        sel = slot == 6 + 2 * i
        order = np.argsort(key_view(mixed[sel]), kind="stable")
        assert nheld[sel][order].tolist() == [1] * start + [64] + [1] * 10
        assert start < (64, 256, 512)[i] < start + 64
    _, counts = c.across(5000)
    assert len(set(counts.tolist())) >= 8 and counts.min() == 1 and counts.max() == len(EMIT_LAYOUT[k])    # counters of every size


# =========================================================================== 5. key-range waves
WAVE_K = (15, 41, 64)
WAVE_COUNTS = (1, 2, 3, 7, 11)       # 11: more waves than a genome has buckets
WAVE_RANGE = (0.2976, 0.3571)        # of the key space: buckets 250 .. 299 of 840


def wave_nb_text(k):
    return 4 if words(k) == 1 else 8


@functools.lru_cache(maxsize=None)
def wave_case(k, sizes):
    """Genomes (sizes: per group) whose 240 keys all lie in WAVE_RANGE of the mixed key space, each key held by a
    random non-empty subset of the genomes; every genome has the same number of bases."""
    w = words(k)
    ngen = sum(sizes)
    npos = wave_nb_text(k) * MEAN[w]
    rng = np.random.default_rng(5000 + k + ngen)
    top = rng.integers(int(WAVE_RANGE[0] * 2**32), int(WAVE_RANGE[1] * 2**32), size=2000, dtype=np.uint64)
    codes = unmix_np(k, mixed_from_top32(k, top, rng))
    codes = codes[canonical(k, codes)]
    _, first = np.unique(key_view(codes), return_index=True)
    codes = codes[np.sort(first)][:240]
    assert codes.shape[0] == 240
    subsets = rng.integers(1, 1 << ngen, size=240)
    held = [(codes[i:i + 1], [g for g in range(ngen) if (int(subsets[i]) >> g) & 1]) for i in range(240)]
    return Case(k, texts_of(k, ngen, held, npos, rng), groups_of(sizes))


def waves_of(bases, budget):
    return max(1, -(-bases // budget))


def wave_budget(bases, nwaves):
    budget = -(-bases // nwaves)
    assert waves_of(bases, budget) == nwaves
    return budget


WAVE_LAYOUTS = ((6,), (2, 2, 2))


@pytest.mark.parametrize("k", WAVE_K)
def test_wave_case_preconditions(k):
    for sizes in WAVE_LAYOUTS:
        c = wave_case(k, sizes)
        assert len(set(c.lens())) == 1 and c.totals["distinct"] > 240
        keys, _ = c.across(BIG)
        assert keys.shape[0] == 240
        empty = {}
        for nwaves in WAVE_COUNTS:
            batch = c.lens() if len(sizes) == 1 else c.lens()[:2]       # every group of (2, 2, 2) is a batch of its own
            gnb, s_ranges = geometry(k, batch, max(sizes), nwaves)
            assert gnb == -(-wave_nb_text(k) // nwaves)
            wave = slot_np(k, mix_np(k, keys), gnb * nwaves).astype(np.int64) // gnb
            assert wave.max() < nwaves
            empty[nwaves] = nwaves - np.unique(wave).shape[0]
            assert c.slot_totals(gnb * nwaves, s_ranges).max() <= CAP_PAY[c.w] // 2
        assert empty[1] == 0 and empty[2] == 1 and empty[3] == 1 and empty[7] == 6 and empty[11] >= 9
        assert WAVE_COUNTS[-1] > wave_nb_text(k)


# =========================================================================== 6. batches and big groups
BATCH_K = (41, 63, 64, 15)
BATCH_LAYOUTS = ([64], [65], [64, 1], [1, 64], [63, 2], [128], [129], [10, 70, 3], [1] * 65, [1] * 130, [2] * 40)


@functools.lru_cache(maxsize=None)
def batch_case(k, sizes):
    """Genomes of 2 .. 5 kbp, groups interleaved: a genome is a window of its group's ancestor with a few substitutions,
    every fourth genome of the input followed by a block all groups share (in more of them it would overfill the slots
    planned for one-genome groups: test_fused_retries_with_finer_slots)."""
    rng = np.random.default_rng(6000 + k + 7 * len(sizes) + sum(sizes))
    shared = random_dna_np(rng, 200)
    seqs, group_of = [], []
    anc = [np.frombuffer(random_dna_np(rng, 6000), dtype=np.uint8) for _ in sizes]
    left = list(sizes)
    while any(left):                                     # interleaved: one genome of every group that still has one
        for g in range(len(sizes)):
            if not left[g]:
                continue
            left[g] -= 1
            n = int(rng.integers(2000, 5001 - 200))
            a = anc[g][:n].copy() if left[g] % 2 else anc[g][6000 - n:].copy()
            at = rng.integers(0, n, size=n // 300)
            a[at] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=at.shape[0])]
            seqs.append(a.tobytes() + (b"N" + shared if len(seqs) % 4 == 0 else b""))
            group_of.append(g)
    return Case(k, seqs, group_of)


def edge_group_case(k):
    """A small copy of test_big_group_edge_genomes: a group of 70 genomes with an empty one, one of k - 1 bases, an exact
    copy of a neighbour, a genome holding itself twice, a homopolymer run and an N run; a group of 66 genomes; a small
    group that shares sequence with both."""
    rng = np.random.default_rng(6500 + k)
    anc = [random_dna_np(rng, 4000), random_dna_np(rng, 4000)]

    def variant(g):
        a = np.frombuffer(anc[g], dtype=np.uint8).copy()
        n = int(rng.integers(2000, 4001))
        at = rng.integers(0, n, size=8)
        a[at] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=8)]
        return a[:n].tobytes()
    big = [variant(0) for _ in range(70)]
    big[3] = b""
    big[10] = anc[0][:k - 1]
    big[21] = big[20]
    big[30] = big[30][:1500] + b"N" + big[30][:1500]
    big[40] = big[40][:1000] + b"A" * 900 + big[40][1000:2000]
    big[69] = big[69][:1200] + b"N" * 700 + big[69][1200:2400]
    second = [variant(1) for _ in range(66)]
    small = [anc[0][500:2500] + b"N" + anc[1][1000:3000], anc[1][:2200], random_dna_np(rng, 2500)]
    seqs = big + second + small
    group_of = [0] * 70 + [1] * 66 + [2] * 3
    order = rng.permutation(len(seqs))
    return Case(k, [seqs[i] for i in order], [group_of[i] for i in order])


def test_batch_case_preconditions():
    for sizes in BATCH_LAYOUTS:
        c = batch_case(41, tuple(sizes))
        assert np.bincount(c.group_of).tolist() == list(sizes)
        assert all(2000 <= n <= 5000 for n in c.lens())
        if len(sizes) > 1 and min(sizes) > 1:
            assert c.group_of[:len(sizes)] == list(range(len(sizes)))        # interleaved
    assert {sum(s) for s in BATCH_LAYOUTS} >= {64, 65, 128, 129, 130} and [1] * 65 in BATCH_LAYOUTS
    for k in BATCH_K:            # no retry is expected: the fullest slot of a batch of 64 one-genome groups fits
        for sizes in ([1] * 65, [1] * 130):
            c = batch_case(k, tuple(sizes))
            for g0 in range(0, len(sizes) - 1, 64):
                sub = Case(k, c.seqs[g0:g0 + 64], list(range(len(c.seqs[g0:g0 + 64]))))
                assert c.group_of[g0:g0 + 64] == list(range(g0, g0 + len(sub.seqs)))
                gnb, s_ranges = geometry(k, sub.lens(), 1)
                assert sub.slot_totals(gnb, s_ranges).max() <= CAP_PAY[sub.w]
    c = batch_case(41, (10, 70, 3))
    o = c.oracle(5000, 80)
    assert o["across_hist"][2:4].sum() > 0 and o["within_hist"][1, 20:].sum() > 0      # shared across groups, and inside one
    e = edge_group_case(63)
    lens = [len(s) for s, g in zip(e.seqs, e.group_of) if g == 0]
    assert len(lens) == 70 and 0 in lens and 62 in lens and np.bincount(e.group_of).tolist() == [70, 66, 3]
    assert any(b"A" * 900 in s for s in e.seqs) and any(b"N" * 700 in s for s in e.seqs)
    assert e.oracle(5000, 80)["across_hist"][2:].sum() > 0


# =========================================================================== 7. the statistics suspicion
@functools.lru_cache(maxsize=None)
def big_group_retry_case(k=41):
    """One group of 70 genomes: the first sub-batch of exp1_big_group is the 64 genomes of fill_case(k, 'cap+1', 3 waves,
    fan 64) — it runs in three key-range waves and overflows a slot in the last one —, the second is six genomes that
    hold some of its keys."""
    first = fill_case(k, "cap+1", 3, 64)
    rng = np.random.default_rng(7000 + k)
    keys, _ = first.across(BIG)
    npos = NB_TEXT * MEAN[words(k)]
    more = [planted_text(k, keys[g::9], np.ones(keys[g::9].shape[0], dtype=np.int64), npos, rng) for g in range(6)]
    return Case(k, first.seqs + tuple(more), [0] * 70, first=first)


def test_big_group_retry_case_preconditions():
    c = big_group_retry_case()
    first = c.info["first"]
    assert c.seqs[:64] == first.seqs and len(c.seqs) == 70 and c.ngroups == 1
    bases = sum(first.lens())
    budget = wave_budget(bases, 3)
    assert waves_of(sum(c.lens()[64:]), budget) == 1                     # the second sub-batch: one wave
    # in the sub-batch every genome is a group of its own, the slots are planned for the 64 of them (fan_hint)
    gnb, s_ranges = geometry(41, first.lens(), 64, 3)
    assert (gnb, s_ranges) == (first.info["gnb"], first.info["S"])
    tot = first.slot_totals(3 * gnb, s_ranges)
    assert tot.max() == CAP_PAY[2] + 1 and int(np.argmax(tot)) // s_ranges // gnb == 2 and tot.sum() == tot.max()


# =========================================================================== GPU
@pytest.fixture(scope="module")
def E():
    from khoice_amd import build as kbuild
    from khoice_amd import engine
    if not os.environ.get("KHOICE_HIP_LIB"):
        kbuild.build_library()
    return engine


@pytest.fixture(scope="module")
def eng(E):
    e = E.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_tickets(E):
    """Second context whose ordered kernels take their parts by atomic ticket (KHOICE_TICKETS)."""
    old = os.environ.get("KHOICE_TICKETS")
    os.environ["KHOICE_TICKETS"] = "1"
    try:
        e = E.Engine(0)
    finally:
        if old is None:
            del os.environ["KHOICE_TICKETS"]
        else:
            os.environ["KHOICE_TICKETS"] = old
    yield e
    e.close()


def same_across_set(eng, kset, case, cs, what):
    """The emitted set: length, keys and counters against the oracle-derived one; strictly ascending in mixed key as
    stored; usable as an operand."""
    wkeys, wcounts = case.across(cs)
    keys, counts = kset.download_sorted()
    assert keys.shape == wkeys.shape, (what, keys.shape, wkeys.shape)
    assert (keys == wkeys).all(), what
    assert (counts == wcounts).all(), what
    stored, _ = kset.download()
    v = key_view(mix_np(case.k, stored))
    if case.w == 1:
        assert (v[1:] > v[:-1]).all(), what
    else:
        assert ((v["hi"][1:] > v["hi"][:-1]) | ((v["hi"][1:] == v["hi"][:-1]) & (v["lo"][1:] > v["lo"][:-1]))).all(), what
    assert len(eng.intersect(kset, kset)) == wkeys.shape[0], what


def run_checked(eng, monkeypatch, case, env, emit, pairs, what, launches=None, retries=0, fused=True, skm_still=True):
    """exp1_run under `env` at every (cs, hist_len) of `pairs` against the oracle; launches: by how much the profile
    entry union_tagged must move (None: it must move), retries: by how much `retries` must (None: not pinned); fused:
    a fused form completes the call, so builds / bases / kmers / distinct move by the oracle's totals."""
    for name in ENV_NAMES:
        monkeypatch.delenv(name, raising=False)
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    out = None
    for cs, hl in pairs:
        want = case.oracle(cs, hl)
        eng.profile(True)
        st0 = eng.stats()
        got = eng.exp1_run(list(case.seqs), case.group_of, case.k, cs=cs, hist_len=hl, want_across_set=emit)
        st1 = eng.stats()
        eng.profile(False)
        moved = {n: st1["kernels"][n]["launches"] - st0["kernels"][n]["launches"] for n in st1["kernels"]}
        delta = {n: st1[n] - st0[n] for n in ("builds", "bases", "kmers", "distinct", "retries")}
        print("run_checked:", what, cs, hl, "union_tagged", moved["union_tagged"], delta, "want", case.totals)
        for f in ("within_hist", "across_hist", "distinct_per_seq"):
            assert got[f].shape == want[f].shape and (got[f] == want[f]).all(), (what, cs, hl, f)
        if emit:
            same_across_set(eng, got["across_set"], case, cs, (what, cs, hl))
        if launches is None:
            assert moved["union_tagged"] > 0, (what, cs, hl)
        else:
            assert moved["union_tagged"] == launches, (what, cs, hl, moved["union_tagged"])
        if skm_still:
            assert moved["skm_union"] == moved["skm_pack"] == moved["skm_phased"] == 0, (what, moved)
        if retries is not None:
            assert delta["retries"] == retries, (what, cs, hl, delta["retries"])
        if fused:
            assert {n: delta[n] for n in case.totals} == case.totals, (what, cs, hl, delta, case.totals)
        out = got
    for name in env:
        monkeypatch.delenv(name)
    return out


# --------------------------------------------------------------------------- 1 (and 7: the statistics of every call)
@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
def test_slot_fill_at_capacity(eng, monkeypatch, form):
    k, env, emit = FORMS[form]
    pairs = PAIRS[:2]
    for kind in ("cap-1", "cap"):                        # fits: one launch, no retry
        run_checked(eng, monkeypatch, fill_case(k, kind), env, emit, pairs, (form, kind), launches=1, retries=0)
    # one element more, spread over the sub-range's fine bins: one retry, the finer slots answer
    run_checked(eng, monkeypatch, fill_case(k, "cap+1"), env, emit, pairs, (form, "cap+1"), launches=2, retries=1)
    # 64 elements more in ONE fine bin: the finer slots overflow too, the general path answers
    run_checked(eng, monkeypatch, fill_case(k, "one_bin"), env, emit, pairs, (form, "one_bin"), launches=2, retries=2, fused=False)


@pytest.mark.gpu
@pytest.mark.parametrize("emit", (False, True))
def test_slot_fill_beyond_any_retry(eng, monkeypatch, emit):
    """A slot of 64 x 446 elements asks for more than 16 x the sub-ranges: no second attempt; the general path answers.
    (Its group unions — 32 operands x 446 keys in 1 / 918 of the key space — used to end in 'a key range still overflows
    LDS after 8 re-plans': the re-plan's mean fill stopped at 16 keys, 892 ranges; it now goes down to 1.)"""
    run_checked(eng, monkeypatch, fill_case(33, "huge"), NO_SKM, emit, PAIRS[:1], ("huge", emit), launches=1, retries=None, fused=False)     # (retries also counts the re-plans of the general path's unions)


# --------------------------------------------------------------------------- 2
@pytest.mark.gpu
@pytest.mark.parametrize("k", LEAD_K)
def test_leader_search_in_full_bins(eng, monkeypatch, k):
    env = {**NO_SKM, "KHOICE_NO_UNION_HASH": "1"}
    run_checked(eng, monkeypatch, leader_case(k), env, False, PAIRS[:2], ("leaders", k), launches=1)
    # the same bins through the other read-outs: the hash form (one-word keys) and the sorted, emitting form
    if k <= 32:
        run_checked(eng, monkeypatch, leader_case(k), NO_SKM, False, PAIRS[:1], ("leaders hash", k), launches=1)
    run_checked(eng, monkeypatch, leader_case(k), NO_SKM, True, PAIRS[:1], ("leaders emit", k), launches=1)


# --------------------------------------------------------------------------- 3
@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_masks_and_readout(eng, monkeypatch, name, form):
    k, env, emit = FORMS[form]
    run_checked(eng, monkeypatch, mask_case(k, name), env, emit, PAIRS, (name, form), launches=1)


# --------------------------------------------------------------------------- 4
@pytest.mark.gpu
@pytest.mark.parametrize("tickets", (False, True))
@pytest.mark.parametrize("k", EMIT_K)
def test_emitting_form(eng, eng_tickets, monkeypatch, k, tickets):
    e = eng_tickets if tickets else eng
    env = NO_SKM if k < 64 else {}
    run_checked(e, monkeypatch, emit_case(k), env, True, PAIRS[:2] + PAIRS[3:4], ("emit", k, tickets), launches=1)
    assert e.stats()["order_fallbacks"] == 0


# --------------------------------------------------------------------------- 5
@pytest.mark.gpu
@pytest.mark.parametrize("k", WAVE_K)
def test_key_range_waves(eng, monkeypatch, k):
    base = NO_SKM if k < 64 else {}
    for sizes in WAVE_LAYOUTS:
        c = wave_case(k, sizes)
        one_batch = len(sizes) == 1
        bases = sum(c.lens()) if one_batch else sum(c.lens()[:2])           # (2, 2, 2): every group a batch of its own
        for nwaves in WAVE_COUNTS:
            env = {**base, "KHOICE_WAVE_BASES": str(wave_budget(bases, nwaves))}
            launches = nwaves * (1 if one_batch else len(sizes))
            for emit in (False, True):          # the emitted set is compared with the oracle's: the same for every wave count
                run_checked(eng, monkeypatch, c, env, emit, PAIRS[:1], ("waves", k, sizes, nwaves, emit), launches=launches)
        run_checked(eng, monkeypatch, c, base, True, PAIRS[1:2], ("waves", k, sizes, "no budget"), launches=1)


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
def test_overfull_slot_in_the_last_wave(eng, monkeypatch, form):
    """Three waves, the slot of cap + 1 elements in the last: the first attempt is lost after two good waves, the second
    runs all three with finer slots; the statistics count the batch once."""
    k, env, emit = FORMS[form]
    c = fill_case(k, "cap+1", 3, 64)                     # one group: the budget cannot cut the batch in two
    env = {**env, "KHOICE_WAVE_BASES": str(wave_budget(sum(c.lens()), 3))}
    run_checked(eng, monkeypatch, c, env, emit, PAIRS[:2], (form, "cap+1 in wave 2"), launches=6, retries=1)
    run_checked(eng, monkeypatch, fill_case(k, "cap", 3, 64), env, emit, PAIRS[:1], (form, "cap in wave 2"), launches=3, retries=0)


# --------------------------------------------------------------------------- 6
@pytest.mark.gpu
@pytest.mark.parametrize("k", BATCH_K)
def test_batches_and_big_groups(eng, monkeypatch, k):
    for sizes in BATCH_LAYOUTS:
        c = batch_case(k, tuple(sizes))
        run_checked(eng, monkeypatch, c, NO_SKM if k <= 63 else {}, False, PAIRS[:1], ("batches", k, sizes), skm_still=True)
        if max(sizes) > TAG_MAX_OPS and 32 < k <= 63:     # the pass by group may use the super-k-mer form: no word on skm_union
            run_checked(eng, monkeypatch, c, {}, False, PAIRS[1:2], ("batches, skm allowed", k, sizes), skm_still=False)
    for sizes in ([65], [10, 70, 3], [1] * 130):          # the emitted sets of the batches, summed
        c = batch_case(k, tuple(sizes))
        run_checked(eng, monkeypatch, c, NO_SKM if k <= 63 else {}, True, PAIRS[3:4], ("batches emit", k, sizes))


@pytest.mark.gpu
@pytest.mark.parametrize("k", (63, 64))
def test_big_group_edge_genomes_wide_keys(eng, monkeypatch, k):
    c = edge_group_case(k)
    for pairs in (((5000, 80),), ((7, 9),)):
        run_checked(eng, monkeypatch, c, NO_SKM if k <= 63 else {}, False, pairs, ("edge genomes", k), retries=None)
        run_checked(eng, monkeypatch, c, NO_SKM if k <= 63 else {}, True, pairs, ("edge genomes emit", k), retries=None)
    run_checked(eng, monkeypatch, c, {}, False, ((7, 9),), ("edge genomes, skm allowed", k), retries=None, skm_still=False)


# --------------------------------------------------------------------------- 7
@pytest.mark.gpu
def test_big_group_statistics_after_a_retry(eng, monkeypatch):
    """A group of 70 genomes at k = 41 whose first sub-batch runs in three waves and overflows a slot in the last one:
    the retry with finer slots succeeds, and builds / bases / kmers / distinct must count every genome once.
    (Before exp1_big_group rolled failed attempts back, this call counted the first sub-batch's 64 builds and its
    bases twice, and the k-mers and distinct keys of the two good waves of the lost attempt on top.)"""
    c = big_group_retry_case()
    budget = str(wave_budget(sum(c.info["first"].lens()), 3))
    # the emitted group set: exp1_batched alone — (3 + 3) launches of the first sub-batch, 1 of the second
    run_checked(eng, monkeypatch, c, {**NO_SKM, "KHOICE_WAVE_BASES": budget}, True, PAIRS[:1], "big group retry, emit",
                launches=7, retries=1)
    # histograms only: the two-pass form gives up at its pass by group (no super-k-mer form), exp1_batched starts over
    run_checked(eng, monkeypatch, c, {**NO_SKM, "KHOICE_WAVE_BASES": budget}, False, PAIRS[:2], "big group retry",
                launches=14, retries=2)
    # and with the super-k-mer form allowed for the pass by group (whether it takes it is not this module's business)
    run_checked(eng, monkeypatch, c, {"KHOICE_WAVE_BASES": budget}, False, PAIRS[:1], "big group retry, two-pass",
                retries=None, skm_still=False)
