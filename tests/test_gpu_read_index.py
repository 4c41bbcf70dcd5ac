"""The merged mask index (kh_index.hip: k_index_dir, k_index_tag, k_index_member, k_read_index) through Engine.mask_index,
MaskIndex, Engine.read_votes_index and the index form of kh_exp6_run (KHOICE_EXP6_INDEX=1), against plain Python over
Python sets (tests/read_level_oracle.py for the votes, compared as float64 with ==), against numpy on constructed
mixed keys, and against the set form of the same calls.  The unmarked test proves on the oracle and numpy alone that
the inputs hold what the GPU tests rely on."""
import functools
import gzip
import json
import os
import random

import numpy as np
import pytest

from khoice_amd import merge_lists as ML
from oracle import kmer_oracle as O
from tests import read_level_oracle as RL
from tests.util import distinct_raw, key_view, mix_np, mixed_from_top32, slot_np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "merge_lists_read_level.json")))["cases"]
TILE = 256                      # positions per workgroup of k_read_index
KH_E_ARG, KH_E_KMISMATCH = -1, -5
CONTENT_KS = (5, 13, 16, 31, 32, 33, 41, 63, 64)
CONTENT_NSETS = (1, 2, 3, 64, 65, 66, 130)
VOTE_KS = (5, 13, 31, 32, 33, 63, 64)
VOTE_NSETS = (1, 3, 64, 66)
EXP6_KS = (13, 16, 17, 31, 32, 33, 63, 64)
EXP6_GROUPS = (1, 3, 65)
BUCKET_KEYS = (1, 4, 4096)      # KHOICE_INDEX_BUCKET_KEYS: a bucket per key, the default, one bucket for everything
EDGE_KS = (31, 41)              # one-word and two-word keys
EDGE_NSETS = 66                 # set 0: every key; 1: every 2nd; 2: every 3rd; 65: every 5th; the others empty
PATTERNS = (0x00, 0x41, 0x63, 0xFF)
CS, HIST_LEN = 5000, 64
COMP = str.maketrans("ACGT", "TGCA")


@pytest.fixture(scope="module")
def eng():
    from khoice_amd import build as kbuild
    from khoice_amd import engine as E
    kbuild.build_library()
    e = E.Engine(0)
    yield e
    e.close()


# ---------------------------------------------------------------- helpers (restated, not imported from a test file)
def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def canon(w):
    """The canonical form of an upper-case ACGT window (RL.canonical without its character loop)."""
    rc = w.translate(COMP)[::-1]
    return w if w < rc else rc


def kmers_of(text, k):
    """The canonical k-mers of a text as a build sees it: case folded, a window with any other byte left out."""
    t = text.upper()
    return {canon(t[i:i + k]) for i in range(len(t) - k + 1) if not t[i:i + k].strip("ACGT")}


def layout(reads):
    text = "".join(r + "\n" for r in reads).encode()
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    if reads:
        off[1:] = np.cumsum([len(r) + 1 for r in reads])
    return text, off


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
    d = {n: st1["kernels"][n]["launches"] - st0["kernels"][n]["launches"] for n in st1["kernels"]}
    d["poisoned_bytes"] = st1["poisoned_bytes"] - st0["poisoned_bytes"]
    return out, d


def key_ints(keys):
    """keys[n, W] uint64 -> Python ints."""
    return [int(r[0]) | (int(r[1]) << 64 if len(r) == 2 else 0) for r in keys]


def mask_ints(masks):
    return [sum(int(w) << (64 * j) for j, w in enumerate(r)) for r in masks]


# ---------------------------------------------------------------- the texts of tests 1 and 3
@functools.lru_cache(maxsize=None)
def base_text(k):
    """5600 random bases; an even k gets reverse-complement palindromes of length k planted every 500 bases."""
    rng = random.Random(100 + k)
    t = list(rand_seq(rng, 5600))
    if k % 2 == 0:
        for at in range(100, 5000, 500):
            half = rand_seq(rng, k // 2)
            t[at:at + k] = half + O.reverse_complement(half)
    return "".join(t)


def slice_text(k, d):
    """Set d's text: overlapping 2800-base slices of the base text, so that position x of it lies in 1, 2, .. 7, 6, .. 1,
    0 of the first seven sets as x grows; later sets are the same slices moved by a few bases."""
    lo = (d % 7) * 400 + (d // 7) * 37
    return base_text(k)[lo:lo + 2800]


def set_texts(k, nsets):
    """Set 1 is empty and the last set is set 0 again (ties of two)."""
    texts = [slice_text(k, d) for d in range(nsets)]
    if nsets >= 2:
        texts[-1] = texts[0]
    if nsets >= 3:
        texts[1] = ""
    return texts


@functools.lru_cache(maxsize=None)
def slice_kmers(k, d):
    return frozenset(kmers_of(slice_text(k, d), k))


def set_kmers(k, nsets):
    """The Python sets of set_texts(k, nsets), shared between the cases."""
    out = [slice_kmers(k, d) for d in range(nsets)]
    if nsets >= 2:
        out[-1] = out[0]
    if nsets >= 3:
        out[1] = frozenset()
    return out


def device_sets(eng, k, nsets):
    w = 1 if k <= 32 else 2
    return [eng.build(t.encode(), k, with_counts=False) if len(t) >= k else eng.upload(k, np.zeros((0, w), dtype=np.uint64), None)
            for t in set_texts(k, nsets)]


@functools.lru_cache(maxsize=None)
def reads_for(k):
    """300 reads of one call: the lengths 0, k-1, k, k+1; 63 .. 129 windows; 5000 bases over every depth of the slices;
    a read whose newline is the first byte of a 256-position tile and the read that starts the next tile; reads of
    random sequence; the rest short cuts of the base text."""
    rng = random.Random(200 + k)
    base = base_text(k)
    reads, special = [], {}

    def cut(n):
        at = rng.randrange(0, 5200 - n)
        return base[at:at + n]

    def total():
        return sum(len(r) + 1 for r in reads)
    for n in (0, k - 1, k, k + 1):
        reads.append(cut(n))
    for w in (63, 64, 65, 127, 128, 129):
        reads.append(cut(w + k - 1))
    special["long"] = len(reads)
    reads.append(base[400:5400])
    n = (-total() - 1) % TILE + 1                  # its newline is the first byte of a tile
    while n < k + 5:
        n += TILE
    special["ends_at_tile"] = len(reads)
    reads.append(cut(n))
    n = (-total() - 1) % TILE                      # the read behind it is cut so that the NEXT read starts a tile
    while n < k + 5:
        n += TILE
    reads.append(cut(n))
    special["opens_tile"] = len(reads)
    reads.append(cut(2 * k + 70))
    for i in range(6):
        special.setdefault("random", len(reads))
        reads.append(rand_seq(rng, (k + 90, k, 3 * k, 200, k + 1, 64 + k)[i]))
    while len(reads) < 300:
        reads.append(cut(rng.randrange(0, 2 * k + 12)))
    return tuple(reads), special


@functools.lru_cache(maxsize=None)
def want_for(k, nsets):
    """The oracle's answer for reads_for(k) against set_texts(k, nsets): computed once, shared, left unchanged."""
    return tuple(RL.reads_votes(reads_for(k)[0], k, set_kmers(k, nsets)))


def compare(got, want, nsets, what):
    n = len(want)
    votes = np.array([[float(v) for v in w[0]] for w in want], dtype=np.float64).reshape(n, nsets)
    unm = np.array([w[2] for w in want], dtype=np.uint32)
    assert got["votes"].shape == votes.shape and got["votes"].dtype == np.float64
    bad = np.argwhere(got["votes"] != votes)
    assert bad.size == 0, (what, bad[:6].tolist(), [(got["votes"][tuple(b)], votes[tuple(b)]) for b in bad[:6]])
    assert (got["tie_masks"] == RL.tie_masks(want, nsets)).all(), what
    assert (got["unmatched"] == unm).all(), what


def same_votes(a, b):
    for f in ("votes", "tie_masks", "unmatched"):
        assert a[f].shape == b[f].shape and (a[f] == b[f]).all(), f


# ---------------------------------------------------------------- the constructed keys of test 2
def edge_buckets(n, bucket_keys):
    """nb of kh_index_build: clamp(ceil(n / B), 1, 2^31)."""
    return min(1 << 31, max(1, -(-n // bucket_keys)))


@functools.lru_cache(maxsize=None)
def edge_keys(name, k):
    """Distinct mixed keys[n, W], ascending, of a named construction."""
    rng = np.random.default_rng(sum(map(ord, name)) * 100 + k)
    top = 1 << 32
    if name == "slot0":                 # 200 keys below 2^32 / 400: slot 0 even with a bucket per key
        mixed = mixed_from_top32(k, rng.integers(0, top // 400, size=200, dtype=np.uint64), rng)
    elif name == "last_slot":           # ... in the last 1 / 400 of the key space
        mixed = mixed_from_top32(k, np.uint64(top - top // 400) + rng.integers(0, top // 400, size=200, dtype=np.uint64), rng)
    elif name == "ends":                # the mixed keys 0 and 2^(2k) - 1
        m = (1 << (2 * k)) - 1
        mixed = np.array([[v & (2**64 - 1), v >> 64][:1 if k <= 32 else 2] for v in (0, m)], dtype=np.uint64)
    elif name == "same_top":            # 1000 keys that share their top 32 bits and nothing else
        mixed = mixed_from_top32(k, np.full(1000, 0x9E3779B9, dtype=np.uint64), rng)
    elif name == "one":
        mixed = mixed_from_top32(k, np.array([0x12345678], dtype=np.uint64), rng)
    elif name == "two_clusters":        # every bucket between the clusters is empty
        lo = rng.integers(0, 1 << 20, size=100, dtype=np.uint64)
        hi = np.uint64(top - (1 << 20)) + rng.integers(0, 1 << 20, size=100, dtype=np.uint64)
        mixed = mixed_from_top32(k, np.concatenate([lo, hi]), rng)
    else:
        raise KeyError(name)
    ints = sorted(set(key_ints(mixed)))
    return np.array([[v & (2**64 - 1), v >> 64][:1 if k <= 32 else 2] for v in ints], dtype=np.uint64)


EDGE_NAMES = ("slot0", "last_slot", "ends", "same_top", "one", "two_clusters")


def edge_membership(n):
    """[n] masks as Python ints: what EDGE_NSETS sets hold of key i."""
    return [1 | (i % 2 == 0) << 1 | (i % 3 == 0) << 2 | (i % 5 == 0) << 65 for i in range(n)]


@functools.lru_cache(maxsize=None)
def edge_probe(name, k):
    """Distinct mixed keys: every indexed key, its two neighbours in mixed order, and 64 keys spread over the key space
    (keys of empty buckets for every construction here)."""
    m = (1 << (2 * k)) - 1
    ints = key_ints(edge_keys(name, k))
    rng = np.random.default_rng(7 + k)
    spread = key_ints(mixed_from_top32(k, rng.integers(0, 1 << 32, size=64, dtype=np.uint64), rng))
    probe = sorted({v + d for v in ints for d in (-1, 0, 1) if 0 <= v + d <= m} | set(spread))
    return np.array([[v & (2**64 - 1), v >> 64][:1 if k <= 32 else 2] for v in probe], dtype=np.uint64)


# ---------------------------------------------------------------- the genomes and reads of test 4
@functools.lru_cache(maxsize=None)
def exp6_case(k, ngroups):
    """ngroups groups of one or two genomes of 2000 - 3000 bases: overlapping slices of one 4000-base text and a tail
    of their own, with stretches in lower case and an N in every genome (legal there).  With three groups and more,
    group 1's genomes are shorter than k (an empty dataset) and the last group is group 0 again (ties of two).  Two
    pivots of 60 and 40 clean reads."""
    rng = random.Random(3000 + 10 * k + ngroups)
    base = rand_seq(rng, 4000)
    if k % 2 == 0:
        base = list(base)
        for at in range(100, 3900, 400):
            half = rand_seq(rng, k // 2)
            base[at:at + k] = half + O.reverse_complement(half)
        base = "".join(base)
    groups = []
    for g in range(ngroups):
        lo = (g * 211) % 1500
        gs = [base[lo:lo + 2000 + (g * 97) % 500] + rand_seq(rng, 200)]
        if g % 2 == 0:
            gs.append(base[lo + 300:lo + 2400] + rand_seq(rng, 100))
        groups.append(gs)
    def spoil(text):
        t = list(text)
        for _ in range(5):
            at = rng.randrange(0, len(t) - 40)
            t[at:at + 30] = "".join(t[at:at + 30]).lower()
        t[rng.randrange(0, len(t))] = "N"
        return "".join(t)
    groups = [[spoil(t) for t in gs] for gs in groups]
    if ngroups >= 3:
        groups[1] = [rand_seq(rng, k - 1), rand_seq(rng, k - 1)]
        groups[-1] = list(groups[0])
    genomes = [t for gs in groups for t in gs]
    group_of = [g for g, gs in enumerate(groups) for _ in gs]
    clean = [t.upper().replace("N", "A") for t in genomes if len(t) >= 2000]

    def cut(n):
        src = clean[rng.randrange(len(clean))]
        at = rng.randrange(0, len(src) - n)
        return src[at:at + n]
    reads = [cut(n) for n in (0, k - 1, k, k + 1)] + [cut(w + k - 1) for w in (63, 64, 65, 129)]
    reads += [rand_seq(rng, n) for n in (k + 90, k, 3 * k)] + [base[500:1500]]
    while len(reads) < 60:
        reads.append(cut(rng.randrange(0, 2 * k + 40)))
    second = [cut(rng.randrange(0, 150)) if i % 5 else rand_seq(rng, k + i) for i in range(40)]
    return tuple(genomes), tuple(group_of), (tuple(reads), tuple(second))


def group_sets(genomes, group_of, k):
    sets = [set() for _ in range(max(group_of) + 1)]
    for text, g in zip(genomes, group_of):
        sets[g] |= kmers_of(text, k)
    return sets


@functools.lru_cache(maxsize=None)
def exp6_wanted(k, ngroups):
    """The oracle's (tie masks, unmatched) per pivot: computed once, shared, left unchanged."""
    genomes, group_of, pivots = exp6_case(k, ngroups)
    sets = group_sets(genomes, group_of, k)
    out = []
    for reads in pivots:
        want = RL.reads_votes(reads, k, sets)
        out.append((RL.tie_masks(want, len(sets)), np.array([w[2] for w in want], dtype=np.uint32)))
    return out


def run6(eng, case, k):
    genomes, group_of, pivots = case
    return eng.exp6_run([g.encode() for g in genomes], group_of, [layout(p) for p in pivots], k, cs=CS, hist_len=HIST_LEN)


def same_outputs(a, b):
    assert (a["within_hist"] == b["within_hist"]).all() and (a["distinct_per_seq"] == b["distinct_per_seq"]).all()
    assert len(a["tie_masks"]) == len(b["tie_masks"])
    for p in range(len(a["tie_masks"])):
        assert a["tie_masks"][p].shape == b["tie_masks"][p].shape and (a["tie_masks"][p] == b["tie_masks"][p]).all(), p
        assert (a["unmatched"][p] == b["unmatched"][p]).all(), p


def check_exp6(res, k, ngroups):
    for p, (ties, unm) in enumerate(exp6_wanted(k, ngroups)):
        assert res["tie_masks"][p].shape == ties.shape and (res["tie_masks"][p] == ties).all(), (k, ngroups, p)
        assert (res["unmatched"][p] == unm).all(), (k, ngroups, p)


def index_form(d, pairs):
    assert d["index_dir"] == 1 and d["index_tag"] == 1 and d["read_index"] == pairs and d["read_fold"] == pairs, d
    assert d["read_masks"] == 0 and d["read_lookup"] == 0, d


def set_form(d, pairs):
    assert d["index_dir"] == 0 and d["index_tag"] == 0 and d["read_index"] == 0 and d["read_lookup"] == 0, d
    assert d["read_masks"] == pairs and d["read_fold"] == pairs, d


# ---------------------------------------------------------------- 6. the inputs hold what they claim (no GPU)
def test_the_inputs_hold_what_the_gpu_tests_rely_on():
    from khoice_amd import engine as E
    assert all(hasattr(E.MaskIndex, m) for m in ("info", "download", "masks_of", "close", "__enter__", "__exit__"))
    assert hasattr(E.Engine, "mask_index") and hasattr(E.Engine, "read_votes_index")
    assert {"kh_index_build", "kh_index_free", "kh_index_info", "kh_index_download", "kh_index_masks",
            "kh_read_votes_index"} <= set(E.ABI_SYMBOLS)
    for k in (13, 32, 33, 64):
        reads, special = reads_for(k)
        text, off = layout(reads)
        assert len(reads) == 300
        assert [len(r) for r in reads[:4]] == [0, k - 1, k, k + 1]
        assert [len(r) - k + 1 for r in reads[4:10]] == [63, 64, 65, 127, 128, 129] and len(reads[special["long"]]) == 5000
        e, s = special["ends_at_tile"], special["opens_tile"]
        assert (int(off[e + 1]) - 1) % TILE == 0 and len(reads[e]) >= k      # its newline is a tile's first byte
        assert int(off[s]) % TILE == 0 and len(reads[s]) >= k               # the first base opens a tile
        assert batches_of(off, len(text) // 4) >= 3                          # test 3's cut
        for nsets in (1, 3, 66) if k in (13, 33) else (3,):
            want = want_for(k, nsets)
            sets = set_kmers(k, nsets)
            sizes = {len(w[1]) for w in want}
            if nsets >= 3:
                assert (2 in sizes) if nsets == 3 else any(2 < n < nsets for n in sizes), sizes   # ties of two (three sets) and of more
                assert not sets[1] and sets[0] == sets[-1]
            assert len(want[0][1]) == nsets and want[0][2] == 0              # no window: every set ties
            r = special["random"]
            assert len(want[r][1]) == nsets and want[r][2] == len(reads[r]) - k + 1     # a read with 0 matches
            if nsets <= 3:                                                   # a read whose every k-mer every non-empty set holds
                assert any(len(rd) >= k and all(all(canon(w) in s for s in sets if s) for w in O.windows(rd, k)) for rd in reads)
        depths = {sum(canon(w) in s for s in set_kmers(k, 9)) for w in O.windows(reads[special["long"]], k)}
        assert depths >= set(range(0, 8))                                    # len(M) = 1 .. 7 inside one read, and none
    for k in EDGE_KS:
        for name in EDGE_NAMES:
            mixed = edge_keys(name, k)
            n = mixed.shape[0]
            assert n == {"slot0": 200, "last_slot": 200, "ends": 2, "same_top": 1000, "one": 1, "two_clusters": 200}[name]
            view = key_view(mixed)
            assert (np.sort(view) == view).all() and len(np.unique(view)) == n
            assert (mix_np(k, distinct_raw(k, mixed)) == mixed).all()        # what upload takes, in the index's order
            probe = key_ints(edge_probe(name, k))
            assert set(key_ints(mixed)) <= set(probe) and len(probe) > n
            for b in BUCKET_KEYS:
                nb = edge_buckets(n, b)
                assert nb == {1: n, 4: -(-n // 4), 4096: 1}[b]
                slots = slot_np(k, mixed, nb).astype(np.int64)
                pslots = slot_np(k, edge_probe(name, k), nb).astype(np.int64)
                if name == "slot0":
                    assert (slots == 0).all()
                elif name == "last_slot":
                    assert (slots == nb - 1).all()
                elif name == "ends":
                    assert slots.tolist() == [0, nb - 1]
                elif name in ("same_top", "one"):
                    assert len(set(slots.tolist())) == 1
                else:
                    assert set(slots.tolist()) == ({0, nb - 1} if nb > 1 else {0}) and (slots[:100] == 0).all()
                if nb > 2 and name != "ends":
                    assert set(pslots.tolist()) - set(slots.tolist()), "the probe has keys of empty buckets"
    for k, ngroups in ((13, 3), (33, 65)):
        genomes, group_of, pivots = exp6_case(k, ngroups)
        assert max(group_of) + 1 == ngroups
        long = [g for g in genomes if len(g) >= k]
        assert all(2000 <= len(g) <= 3000 and "N" in g and any(c in g for c in "acgt") for g in long)
        sets = group_sets(genomes, group_of, k)
        assert not sets[1] and sets[0] == sets[-1] and all(len(p) <= 300 for p in pivots)
        seen = {sum(canon(w) in s for s in sets) for r in pivots[0] + pivots[1] for w in O.windows(r, k)}
        assert {0, 2} <= seen and (len(seen) >= 4 or ngroups == 3)      # no group, the identical pair, (65 groups) more


# ---------------------------------------------------------------- 1. index contents
@pytest.mark.gpu
@pytest.mark.parametrize("nsets", CONTENT_NSETS)
@pytest.mark.parametrize("k", CONTENT_KS)
def test_index_contents(eng, k, nsets):
    sets = device_sets(eng, k, nsets)
    py = [{O.encode(m) for m in s} for s in set_kmers(k, nsets)]
    with eng.mask_index(sets) as ix:
        for s in sets:
            s.free()                                               # the index outlives its sets
        keys, masks = ix.download()
        info = ix.info()
    union = eng.union_sum(device_sets(eng, k, nsets), CS)
    ukeys, _ = union.download()
    assert keys.shape == ukeys.shape and (keys == ukeys).all()
    n, mw = keys.shape[0], max(1, (nsets + 63) // 64)
    assert info == {"n": n, "k": k, "nsets": nsets, "mask_words": mw, "buckets": max(1, -(-n // 4))}, info
    assert n == len(set().union(*py)) and masks.shape == (n, mw)
    want = [sum(1 << d for d in range(nsets) if code in py[d]) for code in key_ints(keys)]
    assert mask_ints(masks) == want
    if nsets >= 3:
        assert all(not (m >> 1) & 1 and (m & 1) == (m >> (nsets - 1)) & 1 for m in want)


@pytest.mark.gpu
@pytest.mark.parametrize("k", (13, 33))
def test_an_index_of_empty_sets(eng, k):
    w = 1 if k <= 32 else 2
    sets = [eng.upload(k, np.zeros((0, w), dtype=np.uint64), None) for _ in range(3)]
    rng = random.Random(k)
    with eng.mask_index(sets) as ix:
        assert ix.info() == {"n": 0, "k": k, "nsets": 3, "mask_words": 1, "buckets": 1}
        keys, masks = ix.download()
        assert keys.shape == (0, w) and masks.shape == (0, 1)
        text, off = layout([rand_seq(rng, 200)])
        got = eng.read_votes_index(text, off, ix, want_votes=True, want_unmatched=True)
        assert got["unmatched"].tolist() == [200 - k + 1] and got["tie_masks"].tolist() == [[7]]
        assert (got["votes"] == 0.0).all()
        probe = eng.build(rand_seq(rng, 300).encode(), k, with_counts=False)
        assert not ix.masks_of(probe).any()


# ---------------------------------------------------------------- 2. directory and search edges
@pytest.mark.gpu
@pytest.mark.parametrize("bucket_keys", BUCKET_KEYS)
@pytest.mark.parametrize("name", EDGE_NAMES)
@pytest.mark.parametrize("k", EDGE_KS)
def test_directory_and_search_edges(eng, k, name, bucket_keys, monkeypatch):
    w = 1 if k <= 32 else 2
    mixed = edge_keys(name, k)
    n = mixed.shape[0]
    member = edge_membership(n)

    def upload(rows):
        return eng.upload(k, distinct_raw(k, rows) if rows.shape[0] else np.zeros((0, w), dtype=np.uint64), None)
    sets = [upload(mixed[[i for i in range(n) if (member[i] >> d) & 1]]) for d in range(EDGE_NSETS)]
    monkeypatch.setenv("KHOICE_INDEX_BUCKET_KEYS", str(bucket_keys))
    with eng.mask_index(sets) as ix:
        monkeypatch.delenv("KHOICE_INDEX_BUCKET_KEYS")
        assert ix.info() == {"n": n, "k": k, "nsets": EDGE_NSETS, "mask_words": 2, "buckets": edge_buckets(n, bucket_keys)}
        keys, masks = ix.download()
        assert (mix_np(k, keys) == mixed).all() and mask_ints(masks) == member
        probe = upload(edge_probe(name, k))
        got = ix.masks_of(probe)
        pmixed = mix_np(k, probe.download()[0])                    # the probe's storage order
    assert (pmixed == edge_probe(name, k)).all()
    held = dict(zip(key_ints(mixed), member))
    want = np.array([[held.get(v, 0) & (2**64 - 1), held.get(v, 0) >> 64] for v in key_ints(pmixed)], dtype=np.uint64)
    assert got.shape == want.shape and (got == want).all(), np.argwhere(got != want)[:5]
    assert (want != 0).any(axis=1).sum() == n


# ---------------------------------------------------------------- 3. votes
@pytest.mark.gpu
@pytest.mark.parametrize("nsets", VOTE_NSETS)
@pytest.mark.parametrize("k", VOTE_KS)
def test_votes_ties_and_unmatched_bit_for_bit(eng, k, nsets, monkeypatch):
    reads, special = reads_for(k)
    want = want_for(k, nsets)
    text, off = layout(reads)
    sets = device_sets(eng, k, nsets)
    with eng.mask_index(sets) as ix:
        got, d = measured(eng, lambda: eng.read_votes_index(text, off, ix, want_votes=True, want_unmatched=True))
        assert d["read_index"] == 1 and d["read_masks"] == 0 and d["read_fold"] == 1, d
        compare(got, want, nsets, (k, nsets))
        same_votes(got, eng.read_votes(text, off, k, sets, want_votes=True, want_unmatched=True))
        only = eng.read_votes_index(text, off, ix)                 # the optional outputs left out
        assert set(only) == {"tie_masks"} and (only["tie_masks"] == got["tie_masks"]).all()
        max_pos = len(text) // 4
        nbatches = batches_of(off, max_pos)
        assert nbatches >= 3
        monkeypatch.setenv("KHOICE_READS_MAX_POS", str(max_pos))
        many, d = measured(eng, lambda: eng.read_votes_index(text, off, ix, want_votes=True, want_unmatched=True))
        assert d["read_index"] == nbatches and d["read_fold"] == nbatches, d
        same_votes(got, many)
    if k >= 13:
        r = special["random"]
        assert len(want[r][1]) == nsets and want[r][2] == len(reads[r]) - k + 1   # nothing matched: every set ties


@pytest.mark.gpu
@pytest.mark.parametrize("k", (31, 33))
def test_check_set(eng, k):
    from khoice_amd import engine as E
    reads = list(reads_for(k)[0][:10])
    sets = device_sets(eng, k, 3)
    per_read = [kmers_of(r, k) for r in reads]
    everything = set().union(*per_read)
    only7 = sorted(per_read[7] - set().union(*(s for i, s in enumerate(per_read) if i != 7)))
    assert only7
    w = 1 if k <= 32 else 2

    def upload(kmers):
        keys = np.array([[(O.encode(m) >> (64 * j)) & (2**64 - 1) for j in range(w)] for m in sorted(kmers)], dtype=np.uint64)
        return eng.upload(k, keys.reshape(-1, w), None)
    text, off = layout(reads)
    with eng.mask_index(sets) as ix:
        full = eng.read_votes_index(text, off, ix, check=upload(everything), want_votes=True, want_unmatched=True)
        compare(full, RL.reads_votes(reads, k, set_kmers(k, 3), everything), 3, "check")
        texts = []
        for call in (lambda c: eng.read_votes_index(text, off, ix, check=c), lambda c: eng.read_votes(text, off, k, sets, check=c)):
            with pytest.raises(E.KhoiceError) as ei:
                call(upload(everything - {only7[0]}))
            assert ei.value.code == KH_E_ARG and "read 7 " in str(ei.value), str(ei.value)
            texts.append(str(ei.value))
        assert texts[0] == texts[1], texts
        with pytest.raises(E.KhoiceError) as ei:
            eng.read_votes_index(text, off, ix, check=device_sets(eng, k + 1, 1)[0])
        assert ei.value.code == KH_E_KMISMATCH


@pytest.mark.gpu
@pytest.mark.parametrize("k", (21, 41))
def test_bad_symbols_and_arguments(eng, k):
    from khoice_amd import engine as E
    reads = list(reads_for(k)[0][:12])
    sets = device_sets(eng, k, 3)
    assert len(reads[4]) >= k and len(reads[9]) >= k and len(reads[6]) >= k and len(reads[1]) == k - 1
    with_n = list(reads)
    with_n[9] = with_n[9][:3] + "N" + with_n[9][4:]
    with_n[4] = with_n[4][:-1] + "N"
    lower = list(reads)
    lower[6] = lower[6][:5] + lower[6][5].lower() + lower[6][6:]
    lower[9] = lower[9].lower()
    with eng.mask_index(sets) as ix:
        for bad, lowest in ((with_n, 4), (lower, 6)):
            text, off = layout(bad)
            texts = []
            for call in (lambda: eng.read_votes_index(text, off, ix), lambda: eng.read_votes(text, off, k, sets)):
                with pytest.raises(E.KhoiceError) as ei:
                    call()
                assert ei.value.code == KH_E_ARG and f"read {lowest} " in str(ei.value), str(ei.value)
                texts.append(str(ei.value))
            assert texts[0] == texts[1], texts
        short = list(reads)
        short[1] = "n" * (k - 1)                                   # shorter than k: no k-mer, no error
        text, off = layout(short)
        got = eng.read_votes_index(text, off, ix, want_votes=True, want_unmatched=True)
        compare(got, RL.reads_votes(short, k, set_kmers(k, 3)), 3, "short n")
        got = eng.read_votes_index(b"", np.zeros(1, dtype=np.uint64), ix, want_votes=True, want_unmatched=True)
        assert got["tie_masks"].shape == (0, 1) and got["votes"].shape == (0, 3) and got["unmatched"].shape == (0,)
    with pytest.raises(E.KhoiceError) as ei:
        eng.mask_index([])
    assert ei.value.code == KH_E_ARG
    with pytest.raises(E.KhoiceError) as ei:
        eng.mask_index(sets + device_sets(eng, k + 1, 1))
    assert ei.value.code == KH_E_KMISMATCH
    with pytest.raises(E.KhoiceError) as ei:
        eng.mask_index(sets[:1] * 1025)
    assert ei.value.code == KH_E_ARG and "1024" in str(ei.value)


# ---------------------------------------------------------------- 4. exp6_run
@pytest.mark.gpu
@pytest.mark.parametrize("ngroups", EXP6_GROUPS)
@pytest.mark.parametrize("k", EXP6_KS)
def test_exp6_run_takes_the_form_and_the_set_form_agrees(eng, k, ngroups, monkeypatch):
    case = exp6_case(k, ngroups)
    monkeypatch.setenv("KHOICE_EXP6_INDEX", "1")
    res, d = measured(eng, lambda: run6(eng, case, k))
    index_form(d, 2)
    check_exp6(res, k, ngroups)
    monkeypatch.setenv("KHOICE_EXP6_INDEX", "0")
    ref, d = measured(eng, lambda: run6(eng, case, k))
    set_form(d, 2)
    same_outputs(res, ref)
    assert res["within_hist"].sum() > 0 and res["tie_masks"][0].shape[1] == max(1, (ngroups + 63) // 64)


@pytest.mark.gpu
def test_k12_still_takes_the_bitmap_form(eng, monkeypatch):
    genomes, group_of, pivots = exp6_case(13, 3)
    monkeypatch.setenv("KHOICE_EXP6_INDEX", "1")
    res, d = measured(eng, lambda: run6(eng, (genomes, group_of, pivots), 12))
    assert d["read_lookup"] == 2 and d["bmp_group_masks"] == 1 and d["read_index"] == 0 and d["index_dir"] == 0 and d["read_masks"] == 0, d
    sets = group_sets(genomes, group_of, 12)
    for p, reads in enumerate(pivots):
        want = RL.reads_votes(reads, 12, sets)
        assert (res["tie_masks"][p] == RL.tie_masks(want, 3)).all()
        assert (res["unmatched"][p] == np.array([w[2] for w in want], dtype=np.uint32)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("k,ngroups", [(17, 3), (33, 65)])
def test_too_small_a_budget_declines(eng, k, ngroups, monkeypatch):
    case = exp6_case(k, ngroups)
    monkeypatch.setenv("KHOICE_EXP6_INDEX", "1")
    res = run6(eng, case, k)
    monkeypatch.setenv("KHOICE_INDEX_MAX_BYTES", "1")
    ref, d = measured(eng, lambda: run6(eng, case, k))
    set_form(d, 2)
    same_outputs(res, ref)
    check_exp6(ref, k, ngroups)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", PATTERNS, ids=lambda p: f"p{p:02X}")
def test_poisoned_pool(eng, pattern, monkeypatch):
    monkeypatch.setenv("KHOICE_EXP6_INDEX", "1")
    for k, ngroups in ((16, 3), (33, 65)):
        case = exp6_case(k, ngroups)
        monkeypatch.delenv("KHOICE_DEBUG_POISON", raising=False)
        clean, d0 = measured(eng, lambda: run6(eng, case, k))
        assert d0["poisoned_bytes"] == 0, d0
        monkeypatch.setenv("KHOICE_DEBUG_POISON", str(pattern))
        got, d1 = measured(eng, lambda: run6(eng, case, k))
        monkeypatch.delenv("KHOICE_DEBUG_POISON")
        assert d1["poisoned_bytes"] > 0, d1
        index_form(d1, 2)
        same_outputs(got, clean)
        check_exp6(got, k, ngroups)


# ---------------------------------------------------------------- 5. the reference's files
def case_id(c):
    return f"n{c['num_datasets']}_k{c['k']}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", GOLDEN, ids=case_id)
def test_exp6_run_gives_the_references_files(eng, case, tmp_path, monkeypatch):
    monkeypatch.setenv("KHOICE_EXP6_INDEX", "1")
    n, k = case["num_datasets"], case["k"]
    seqs = [g.encode() for gs in case["rest_of_set"] for g in gs]
    group_of = [d for d, gs in enumerate(case["rest_of_set"]) for _ in gs]
    reads = []
    for p, text in enumerate(case["reads_files"]):
        path = tmp_path / f"pivot_{p + 1}.fa"
        path.write_text(text)
        reads.append(ML.read_level_reads(str(path)))
    res, d = measured(eng, lambda: eng.exp6_run(seqs, group_of, reads, k, cs=5000, hist_len=64))
    if k <= 12:
        assert d["read_lookup"] > 0 and d["read_index"] == 0 and d["read_masks"] == 0, d
    else:
        assert d["read_index"] > 0 and d["index_dir"] == 1 and d["read_lookup"] == 0 and d["read_masks"] == 0, d
    random.seed(case["seed"])
    assert ML.read_level_outputs(res["tie_masks"], n, str(k)) == case["outputs"]
    sets = [set().union(*(kmers_of(g, k) for g in gs)) for gs in case["rest_of_set"]]
    for p in range(n):
        want = RL.reads_votes(RL.file_reads(case["reads_files"][p]), k, sets)
        assert (res["tie_masks"][p] == RL.tie_masks(want, n)).all(), p
        assert (res["unmatched"][p] == np.array([w[2] for w in want], dtype=np.uint32)).all(), p


@pytest.mark.gpu
def test_run_batched_on_a_tiny_tree(tmp_path, monkeypatch):
    from khoice_amd.workflow import exp_type_6 as X6
    monkeypatch.setenv("KHOICE_EXP6_INDEX", "1")
    rng = random.Random(66)
    nd, seed, ks = 2, 4242, (7, 21)
    genomes, reads = {}, {}
    shared = rand_seq(rng, 500)
    for num in (1, 2):
        d = tmp_path / f"exp6_input/rest_of_set/dataset_{num}"
        os.makedirs(d)
        anc = shared + rand_seq(rng, 1500)
        for g in range(2):
            seq = "".join(c if rng.random() > 0.01 else rng.choice("ACGT") for c in anc)
            genomes[(num, f"genome_{g}")] = seq
            with gzip.open(d / f"genome_{g}.fna.gz", "wb") as fh:
                fh.write(f">genome_{g}\n{seq}\n".encode())
    for rt, n in (("illumina", 60), ("ont", 400)):
        d = tmp_path / f"exp6_input/pivot_reads_subset/{rt}"
        os.makedirs(d)
        for num in (1, 2):
            src = genomes[(num, "genome_0")]
            rs = []
            for i in range(40):
                m = rng.randrange(0, n)
                at = rng.randrange(0, len(src) - m)
                rs.append(src[at:at + m] if i % 6 else rand_seq(rng, m))
            reads[(rt, num)] = rs
            (d / f"pivot_{num}.fa").write_text("".join(f">r{i}\n{r}\n" for i, r in enumerate(rs)))
    res = X6.run_batched(str(tmp_path), ks, nd, seed)
    assert res["processes"] == 0
    for rt in ("illumina", "ont"):
        values = ""
        for k in sorted(str(k) for k in ks):
            sets = []
            for num in (1, 2):
                names = X6.rest_of_set(str(tmp_path), num)
                sets.append(set().union(*(kmers_of(genomes[(num, g)], int(k)) for g in names)))
            ties = [RL.tie_masks(RL.reads_votes(reads[(rt, num)], int(k), sets), nd) for num in (1, 2)]
            random.seed(seed)
            for name, text in ML.read_level_outputs(ties, nd, k).items():
                assert (tmp_path / f"exp6_accuracies/{rt}" / name).read_text() == text, (rt, name)
                if name.startswith("values/"):
                    values += text
        name = {"illumina": "short", "ont": "long"}[rt]
        assert open(res[f"{name}_acc"]).read() == X6.CSV_HEADER + values
