"""The fused forms on device-resident texts, read where they lie: kh_exp1_run (bitmaps, one- and two-word super-k-mers,
key arrays, emitted sets, a group of more than 64 genomes), kh_exp2_run (bitmaps and sets, pivots included) and
kh_skm_pack take (device pointer, length) pairs.  A text at a multiple of 16 is read in place — every segment with a
base pointer of its own, the bytes behind its end someone else's — anything else is packed into the batch buffer first.

Every case lies in one arena of random bases (tests/util.py: Arena) and runs in three mixes: all texts aligned (nothing
is packed: the pack buffer is its 256-byte stand-in), all unaligned, and both alternating within every group.  Each
run is compared with the oracle, with the run of the same texts as host bytes (results and every statistic but
`text_packed`, the pool size and the kernel times), with the bytes `text_packed` must show for the mix, and the arena
is read back: the library writes nothing into the caller's texts.

The unmarked tests at the end prove on the CPU that a green GPU run cannot be green by missing its target: reading one
base too many or one too few changes a distinct count of every text long enough to have one.

k <= 8: the texts stay at 300 bases or fewer (an unsaturated code space is what makes those two conditions possible),
so the three texts around 8192 positions are part of the cases of k > 8 only."""
import functools

import numpy as np
import pytest

from oracle import c_oracle as CO
from tests.util import ARENA_ALIGNED, ARENA_MAX, ARENA_TAIL, ARENA_UNALIGNED, Arena, canon_positions, random_dna_np

MIXES = ("aligned", "unaligned", "mixed")
TILE, SPLIT = 64, 192            # KHOICE_BMP_TILE_POS / KHOICE_BMP_SPLIT_POS of the "small" bitmap runs: several splits per text
CS, HL = 5000, 96                # more bins than any count a case can reach (at most 73 genomes)
RESIDUALS = {0, 1, 8, 15}
SUBTILE = 8192                   # positions of a scatter sub-tile
EXP1_FIELDS = ("within_hist", "across_hist", "distinct_per_seq")
EXP2_FIELDS = ("within_hist", "across_hist", "within_only", "across_only", "distinct_per_seq", "distinct_per_pivot")
# every statistic a host run and a device run must share: all but text_packed, pool_bytes (the pack buffer is pool
# memory) and the kernel times
STATS = ("builds", "bases", "kmers", "distinct", "setops", "setop_in", "setop_out", "retries", "order_fallbacks",
         "skm_records", "big_slots")

K_BMP, K_EXP2_BMP, K_EXP2_SETS = (5, 8, 12), (8, 12), (13, 31)
K_SKM1, K_SKM2, K_KEYS, K_BIG = (17, 24, 31, 32), (33, 41, 63), (13, 16, 64), (31, 41)
K_SETS = K_PACK = 31


@pytest.fixture(scope="module")
def eng():
    from khoice_amd import build as kbuild
    from khoice_amd import engine as E
    kbuild.build_library()
    e = E.Engine(0)
    yield e
    e.close()


# ---------------------------------------------------------------- the cases
def body_lengths(k):
    """Lengths whose residuals mod 16 are 0, 1, 8 and 15 (twice each, the `rest` of a case included)."""
    if k <= 8:
        return [96, 113, 200, 287, 256, 257, 296, 175]
    return [400, 785, 1208, 2991, 1504, 2225, 648, 335]


def exp1_lengths(k):
    """None: the text given as (0, 0).  0: a valid pointer with length 0.  11: shorter than one 16-byte word."""
    edge = [11, k - 1, k, k + 1, 0, None]
    if k > 8:
        edge += [SUBTILE + k - 2, SUBTILE + k - 1, SUBTILE + k]
    body = body_lengths(k)
    out = []
    for i in range(max(len(edge), len(body))):          # interleaved: every group gets both kinds
        out += body[i:i + 1] + edge[i:i + 1]
    return out


def draw_text(rng, anc, length, k, rate):
    """A piece of the ancestor (every base replaced with probability `rate`) whose last k-mer occurs nowhere else in it, and the byte to put behind it: the
    k-mer of its last k - 1 bases and that byte is no k-mer of the text.  Both are re-derived by the CPU tests."""
    if length < k - 1:
        s = int(rng.integers(0, 33))
        return bytes(anc[s:s + length]), None
    for _ in range(2000):
        s = int(rng.integers(0, 33))
        t = anc[s:s + length].copy()
        hit = rng.random(length) < rate
        t[hit] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(hit.sum()))]
        t = t.tobytes()
        codes = canon_positions(t, k)
        if length >= k and codes.count(codes[-1]) != 1:
            continue
        have = set(codes)
        for f in rng.permutation(np.frombuffer(b"ACGT", dtype=np.uint8)):
            if canon_positions(t[length - (k - 1):] + bytes([f]), k)[0] not in have:
                return t, int(f)
    raise AssertionError(f"no text of {length} bases for k = {k} with a free byte behind it")


class Case:
    """texts (None: given as (0, 0)), behind (the byte behind each text), group_of; for kh_exp2_run the last `npivots`
    texts are the pivots (pivot_group).  The three arenas hold the same texts."""

    def __init__(self, k, lengths, group_of, seed, pivot_group=(), rate=0.01):
        self.k, self.group_of, self.pivot_group = k, list(group_of), list(pivot_group)
        self.npivots = len(self.pivot_group)
        rng = np.random.default_rng(seed)
        anc = np.frombuffer(random_dna_np(rng, max(n or 0 for n in lengths) + 64), dtype=np.uint8)
        drawn = [(None, None) if n is None else draw_text(rng, anc, n, k, rate) for n in lengths]
        self.texts, self.behind = [t for t, _ in drawn], [f for _, f in drawn]
        self.seed = seed
        assert len(self.texts) == len(self.group_of) + self.npivots

    @property
    def host_texts(self):
        return [t if t is not None else b"" for t in self.texts]

    def aligned(self, mix):
        """Per text: is it placed where the library reads it in place?"""
        if mix != "mixed":
            return [mix == "aligned"] * len(self.texts)
        seen, out = {}, []
        for g in self.group_of:                          # alternating within every group
            out.append(seen.get(g, 0) % 2 == 0)
            seen[g] = seen.get(g, 0) + 1
        return out + [p % 2 == 0 for p in range(self.npivots)]

    @functools.lru_cache(maxsize=None)
    def arena(self, mix):
        al, un, classes = 0, 0, []
        for a in self.aligned(mix):
            if a:
                classes.append(ARENA_ALIGNED[al % len(ARENA_ALIGNED)])
                al += 1
            else:
                classes.append(ARENA_UNALIGNED[un % len(ARENA_UNALIGNED)])
                un += 1
        return Arena(self.texts, classes, self.behind, self.seed + 1 + MIXES.index(mix))

    def packed_bytes(self, mix):
        """What text_packed must grow by when every text is read once."""
        a = self.arena(mix)
        return sum(len(t) for t, at in zip(a.texts, a.at) if t is not None and at % 16 != 0)

    def total(self):
        return sum(len(t) for t in self.host_texts)

    @functools.lru_cache(maxsize=None)
    def scrub_texts(self):
        """Other texts of the same lengths, as host bytes: a call on them leaves the library's cached pack buffer
        holding bases that are not the case's, so a kernel that reads the buffer where it should read a text in place
        cannot find the right text there, left behind by the host run."""
        rng = np.random.default_rng(self.seed + 7)
        return [random_dna_np(rng, len(t)) for t in self.host_texts]

    def split(self, seqs):
        n = len(self.group_of)
        return seqs[:n], seqs[n:]


def spread_groups(n, ng):
    return [i % ng for i in range(n)]


@functools.lru_cache(maxsize=None)
def exp1_case(k):
    lengths = exp1_lengths(k)
    return Case(k, lengths, spread_groups(len(lengths), 4), 1000 + k)


@functools.lru_cache(maxsize=None)
def big_case(k):
    """One group of 70 genomes of about 700 bases and a second group of 3."""
    lengths = [(688, 689, 696, 703, 704, 705, 712, 719)[i % 8] for i in range(70)] + [400, 785, 1208]
    return Case(k, lengths, [0] * 70 + [1] * 3, 2000 + k, rate=0.001)


@functools.lru_cache(maxsize=None)
def exp2_case(k):
    """3 groups of 3 / 1 / 2 genomes; one pivot per group and a second pivot for group 0.  (In the mixed arena every
    second text of a group and every second pivot is unaligned: the long ones among them.)"""
    if k <= 8:
        genomes, pivots = [96, 287, 0, 113, k + 1, 200], [257, 120, 11, k]
    else:
        genomes, pivots = [785, SUBTILE + k - 1, 0, 1208, k + 1, 2991], [400, 1505, 11, k]
    return Case(k, genomes + pivots, [0, 0, 0, 1, 2, 2], 3000 + k, pivot_group=[0, 1, 2, 0])


@functools.lru_cache(maxsize=None)
def exp1_oracle(kind, k):
    case = big_case(k) if kind == "big" else exp1_case(k)
    return CO.exp1(case.host_texts, case.group_of, k, cs=CS, hist_len=HL)


@functools.lru_cache(maxsize=None)
def exp2_oracle(k):
    from tests.test_gpu_exp2_bmp import oracle
    case = exp2_case(k)
    seqs, pivots = case.split(case.host_texts)
    return oracle(seqs, case.group_of, pivots, case.pivot_group, k, CS, HL)


@functools.lru_cache(maxsize=None)
def oracle_group_sets(k):
    """(keys, counters) of the group sets of exp1_case(k): the -cs union of its genomes' plain sets."""
    case = exp1_case(k)
    out = []
    for g in range(max(case.group_of) + 1):
        dbs = [CO.count(t, k).set_counts(1) for t, h in zip(case.host_texts, case.group_of) if h == g]
        out.append(CO.union_sum(dbs, CS).arrays())
    return out


# ---------------------------------------------------------------- running and comparing
def measured(eng, call):
    """(what call() returns, {statistic or 'kernel class': growth during the call})"""
    eng.profile(True)
    st0 = eng.stats()
    got = call()
    st1 = eng.stats()
    eng.profile(False)
    d = {n: st1["kernels"][n]["launches"] - st0["kernels"][n]["launches"] for n in st1["kernels"] if n != "copy_in"}
    for n in STATS + ("text_packed",):
        d[n] = st1[n] - st0[n]
    return got, d


def same(got, want, fields, what):
    for f in fields:
        if want[f] is None:
            assert got[f] is None, (what, f)
            continue
        assert got[f].shape == want[f].shape, (what, f)
        assert (got[f] == want[f]).all(), (what, f, np.argwhere(got[f] != want[f])[:8].tolist())


_host_runs = {}


def check(eng, key, case, mix, call, fields, want, form, passes=1, extra=None):
    """call(texts) on the case's texts as host bytes (once per key, kept) and as pointers into the arena of `mix`:
    both the oracle's answer, the same statistics, text_packed as the mix dictates, the arena untouched.
    form(d): the launches that say which form ran.  passes: how often the form reads every text."""
    if key not in _host_runs:
        _host_runs[key] = measured(eng, lambda: call(case.host_texts))
        if extra:
            extra(_host_runs[key][0])
    host, hd = _host_runs[key]
    same(host, want, fields, (key, "host"))
    form(hd)
    assert hd["retries"] == 0, hd
    assert hd["text_packed"] == passes * case.total(), (key, hd["text_packed"], passes, case.total())
    arena = case.arena(mix)
    seqs = arena.upload()
    call(case.scrub_texts())
    got, d = measured(eng, lambda: call(seqs))
    print(key, mix, "text_packed", d["text_packed"], "of", passes * case.total(), {n: v for n, v in d.items() if v})
    same(got, want, fields, (key, mix))
    same(got, host, fields, (key, mix, "against host"))
    if extra:
        extra(got)
    form(d)
    assert {n: v for n, v in d.items() if n != "text_packed"} == {n: v for n, v in hd.items() if n != "text_packed"}, (d, hd)
    assert d["text_packed"] == passes * case.packed_bytes(mix), (key, mix, d["text_packed"], passes, case.packed_bytes(mix))
    assert (arena.download() == arena.host).all(), (key, mix, "the arena was written to")
    arena.dev = None


def exp1_call(eng, case, **kw):
    return lambda texts: eng.exp1_run(texts, case.group_of, case.k, cs=CS, hist_len=HL, **kw)


def exp2_call(eng, case):
    def call(texts):
        seqs, pivots = case.split(texts)
        return eng.exp2_run(seqs, case.group_of, pivots, case.pivot_group, case.k, cs=CS, hist_len=HL)
    return call


def form_bmp(d):
    assert d["bmp_build"] >= 1 and d["bmp_readout"] == 1 and d["union_tagged"] == 0 and d["skm_union"] == 0, d


def form_skm(d):
    assert d["skm_scatter"] == 1 and d["skm_union"] == 1 and d["union_tagged"] == 0 and d["bmp_build"] == 0, d
    assert d["skm_records"] > 0, d


def form_keys(d):
    assert d["union_tagged"] >= 1 and d["extract_scatter"] == 1 and d["skm_union"] == 0 and d["bmp_build"] == 0, d


def form_sets(d):
    assert d["extract_scatter"] >= 1 and d["setop"] >= 1, d
    assert d["union_tagged"] == 0 and d["skm_union"] == 0 and d["skm_scatter"] == 0 and d["bmp_build"] == 0, d


def form_exp2_bmp(d):
    assert d["bmp_build"] >= 1 and d["bmp_pivot"] == 1 and d["bmp_readout"] == 0 and d["setop"] == 0, d


# ---------------------------------------------------------------- the forms of kh_exp1_run
@pytest.mark.gpu
@pytest.mark.parametrize("mix", MIXES)
@pytest.mark.parametrize("tiles", ("default", "small"))
@pytest.mark.parametrize("k", K_BMP)
def test_bitmaps(eng, monkeypatch, k, tiles, mix):
    if tiles == "small":
        monkeypatch.setenv("KHOICE_BMP_TILE_POS", str(TILE))
        monkeypatch.setenv("KHOICE_BMP_SPLIT_POS", str(SPLIT))
    case = exp1_case(k)
    check(eng, ("bmp", k, tiles), case, mix, exp1_call(eng, case), EXP1_FIELDS, exp1_oracle("exp1", k), form_bmp)


@pytest.mark.gpu
@pytest.mark.parametrize("mix", MIXES)
@pytest.mark.parametrize("k", K_SKM1 + K_SKM2)
def test_super_kmers(eng, k, mix):
    case = exp1_case(k)
    check(eng, ("skm", k), case, mix, exp1_call(eng, case), EXP1_FIELDS, exp1_oracle("exp1", k), form_skm)


@pytest.mark.gpu
@pytest.mark.parametrize("mix", MIXES)
@pytest.mark.parametrize("k", K_KEYS)
def test_key_arrays(eng, k, mix):
    case = exp1_case(k)
    check(eng, ("keys", k), case, mix, exp1_call(eng, case), EXP1_FIELDS, exp1_oracle("exp1", k), form_keys)


@pytest.mark.gpu
@pytest.mark.parametrize("mix", MIXES)
def test_emitted_sets(eng, mix):
    k = K_SETS
    case = exp1_case(k)

    def sets_too(got):
        for g, (wkeys, wcounts) in enumerate(oracle_group_sets(k)):
            keys, counts = got["group_sets"][g].download_sorted()
            assert keys.shape == wkeys.shape and (keys == wkeys).all() and (counts == wcounts).all(), g

    check(eng, ("sets", k), case, mix, exp1_call(eng, case, want_sets=True), EXP1_FIELDS, exp1_oracle("exp1", k),
          form_sets, extra=sets_too)


@pytest.mark.gpu
@pytest.mark.parametrize("mix", MIXES)
@pytest.mark.parametrize("across", (True, False))
@pytest.mark.parametrize("k", K_BIG)
def test_group_of_more_than_64(eng, k, across, mix):
    """The passes over a group wider than the genome mask slice the pointer array (seqs + first[p]).  One-word keys:
    phases of up to 32 genomes (k_skm_pack, k_skm_phased); two-word keys: key-array sub-batches of up to 64.  The
    across-group histogram is one more pass over every text with the group as the tag, so each text is read twice."""
    case = big_case(k)
    want = dict(exp1_oracle("big", k))
    if not across:
        want["across_hist"] = None

    def form(d):
        assert d["bmp_build"] == 0, d
        if k <= 32:
            assert d["skm_pack"] >= 3 and d["skm_phased"] >= 1 and d["union_tagged"] == 0, d
        else:
            assert d["union_tagged"] >= 2 and d["skm_pack"] == 0, d
        assert d["skm_union"] == (2 if across else 1), d           # the group of 3, and the across-group pass

    check(eng, ("big", k, across), case, mix, exp1_call(eng, case, across=across), EXP1_FIELDS, want, form,
          passes=2 if across else 1)


# ---------------------------------------------------------------- kh_exp2_run: genomes and pivots
@pytest.mark.gpu
@pytest.mark.parametrize("mix", MIXES)
@pytest.mark.parametrize("k", K_EXP2_BMP)
def test_exp2_bitmaps(eng, k, mix):
    case = exp2_case(k)
    check(eng, ("exp2", k), case, mix, exp2_call(eng, case), EXP2_FIELDS, exp2_oracle(k), form_exp2_bmp)


@pytest.mark.gpu
@pytest.mark.parametrize("mix", MIXES)
@pytest.mark.parametrize("k", K_EXP2_SETS)
def test_exp2_sets(eng, k, mix):
    case = exp2_case(k)

    def form(d):
        assert d["bmp_build"] == 0 and d["bmp_pivot"] == 0 and d["extract_scatter"] >= 1 and d["setop"] >= 1, d

    check(eng, ("exp2", k), case, mix, exp2_call(eng, case), EXP2_FIELDS, exp2_oracle(k), form)


# ---------------------------------------------------------------- kh_skm_pack
def pack_ranks(case):
    """The texts of exp1_case as two ranks (texts [0, 9) and [9, ...)), a rank's tag = the text's group."""
    half = len(case.texts) // 2
    cut = [(0, half), (half, len(case.texts))]
    return cut, [(case.host_texts[a:b], case.group_of[a:b]) for a, b in cut]


@pytest.mark.gpu
@pytest.mark.parametrize("mix", MIXES)
def test_skm_pack(eng, mix):
    """Two ranks, two parts each: the parts and per-slot tables of a pack of device texts are those of the pack of
    host texts, and the pieces give the oracle's across-group histogram."""
    import torch
    from tests.test_gpu_skm_exchange import Job
    k = K_PACK
    case = exp1_case(k)
    cut, ranks = pack_ranks(case)
    key = ("pack", k)
    if key not in _host_runs:
        _host_runs[key] = measured(eng, lambda: Job(eng, ranks, k))
    host, hd = _host_runs[key]
    arena = case.arena(mix)
    seqs = arena.upload()
    scrub = case.scrub_texts()
    Job(eng, [(scrub[a:b], tags) for (a, b), (_, tags) in zip(cut, ranks)], k)
    job, d = measured(eng, lambda: Job(eng, ranks, k, feed=[seqs[a:b] for a, b in cut]))
    print(key, mix, d)
    assert hd["skm_pack"] >= 2 and hd["retries"] == 0 and hd["text_packed"] == case.total(), hd
    assert job.part_n == host.part_n and job.R == 2
    for r in range(2):
        assert torch.equal(job.cnt[r], host.cnt[r]), (r, "count_out")
        assert sorted(job.part_n[r]) != [0, 0]
    assert {n: v for n, v in d.items() if n != "text_packed"} == {n: v for n, v in hd.items() if n != "text_packed"}, (d, hd)
    assert d["text_packed"] == case.packed_bytes(mix), (d["text_packed"], case.packed_bytes(mix))
    want = job.oracle_hist(CS, HL)
    # (a rank's tags are its own: the oracle numbers rank 1's groups behind rank 0's)
    assert (job.hist(CS, HL) == want).all() and (host.hist(CS, HL) == want).all()
    assert want[1:].sum() > 0
    assert (arena.download() == arena.host).all(), "the arena was written to"
    arena.dev = None


# ---------------------------------------------------------------- preconditions, without a GPU
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def plain_kmers(text, k):
    """The canonical k-mers of a text of ACGT as strings, position by position."""
    return [min(text[i:i + k], text[i:i + k][::-1].translate(COMP)) for i in range(len(text) - k + 1)]


def check_case(case, lengths_seen=None):
    k = case.k
    kmers = [None if t is None else plain_kmers(t, k) for t in case.texts]
    for t, km in zip(case.texts, kmers):
        if t is not None and len(t) >= k:                                # under-read: the last k-mer occurs once
            assert km.count(km[-1]) == 1, (k, len(t))
    classes_seen = set()
    for mix in MIXES:
        a = case.arena(mix)
        n = a.host.shape[0]
        assert n < ARENA_MAX and set(np.unique(a.host).tolist()) <= set(b"ACGT")
        placed = sorted((at, len(t)) for t, at in zip(a.texts, a.at) if t is not None)
        assert all(p[0] + p[1] < q[0] for p, q in zip(placed, placed[1:]))         # apart, a byte at least between them
        assert placed[-1][0] + placed[-1][1] + ARENA_TAIL <= n
        mods = []
        for t, at, km, al in zip(a.texts, a.at, kmers, case.aligned(mix)):
            if t is None:
                assert at is None
                continue
            assert a.host[at:at + len(t)].tobytes() == t
            assert (at % 16 == 0) == al and at % 256 in ARENA_ALIGNED + ARENA_UNALIGNED
            mods.append(at % 16)
            if len(t) >= k - 1:                                          # over-read: one more base is one more k-mer
                over = t[len(t) - (k - 1):] + bytes([a.host[at + len(t)]])
                assert plain_kmers(over, k)[0] not in set(km), (k, mix, len(t))
        want = {"aligned": {0}, "unaligned": {1, 8, 15}, "mixed": {0, 1, 8, 15}}[mix]
        assert set(mods) == want, (mix, mods)
        if mix != "unaligned":
            assert {at % 256 for t, at in zip(a.texts, a.at) if t is not None and at % 16 == 0} == set(ARENA_ALIGNED)
        if mix == "mixed":                                               # both kinds in every group of two or more
            for g in set(case.group_of):
                al = [x for x, h in zip(case.aligned(mix), case.group_of) if h == g]
                assert len(al) < 2 or (True in al and False in al), g
            assert case.packed_bytes(mix) not in (0, case.total())
        classes_seen |= set(mods)
    assert classes_seen == {0, 1, 8, 15}
    assert case.packed_bytes("aligned") == 0 and case.packed_bytes("unaligned") == case.total()


@pytest.mark.parametrize("k", sorted(set(K_BMP + K_SKM1 + K_SKM2 + K_KEYS + (K_SETS, K_PACK))))
def test_exp1_cases_hold_their_edges(k):
    case = exp1_case(k)
    check_case(case)
    lens = [None if t is None else len(t) for t in case.texts]
    for n in (0, None, 11, k - 1, k, k + 1) + ((SUBTILE + k - 2, SUBTILE + k - 1, SUBTILE + k) if k > 8 else ()):
        assert n in lens, n
    body = body_lengths(k)
    assert {n % 16 for n in body} == RESIDUALS and all(n in lens for n in body)
    assert all(n <= 300 for n in lens if n) or k > 8
    assert all(200 < n <= 3000 for n in body) or k <= 8
    if k > 8:                                                            # the sub-tile boundary lies inside these texts
        assert [n - k + 1 for n in lens if n and n > SUBTILE] == [SUBTILE - 1, SUBTILE, SUBTILE + 1]
    want = exp1_oracle("exp1", k)
    assert [int(x) for x in want["distinct_per_seq"]] == [len(set(plain_kmers(t, k))) for t in case.host_texts]
    assert int(want["within_hist"][:, 2:].sum()) > 0 and int(want["across_hist"][2:].sum()) > 0
    assert int(want["within_hist"][:, HL - 1].sum()) == 0                # nothing clamps at the last bin
    if k == K_PACK:
        cut, ranks = pack_ranks(case)
        assert all(len(set(tags)) > 1 and max(tags) < 32 for _, tags in ranks)
    if k == K_SETS:
        assert [len(keys) for keys, _ in oracle_group_sets(k)] == [int(want["within_hist"][g].sum()) for g in range(4)]


@pytest.mark.parametrize("k", K_BIG)
def test_big_cases_hold_their_edges(k):
    case = big_case(k)
    check_case(case)
    assert case.group_of.count(0) == 70 and case.group_of.count(1) == 3 and len(case.texts) <= 75
    assert {len(t) % 16 for t in case.texts} == RESIDUALS
    want = exp1_oracle("big", k)
    assert [int(x) for x in want["distinct_per_seq"]] == [len(set(plain_kmers(t, k))) for t in case.host_texts]
    assert int(want["within_hist"][0, 65:71].sum()) > 0                  # k-mers of more genomes than the mask is wide
    assert int(want["across_hist"][2]) > 0


@pytest.mark.parametrize("k", K_EXP2_BMP + K_EXP2_SETS)
def test_exp2_cases_hold_their_edges(k):
    case = exp2_case(k)
    check_case(case)
    assert [case.group_of.count(g) for g in range(3)] == [3, 1, 2] and sorted(case.pivot_group) == [0, 0, 1, 2]
    pivot_classes = {case.arena(mix).at[-4 + p] % 16 for mix in MIXES for p in range(4)}
    assert pivot_classes == {0, 1, 8, 15}                                # the pivots in every offset class
    want = exp2_oracle(k)
    seqs, pivots = case.split(case.host_texts)
    assert [int(x) for x in want["distinct_per_seq"]] == [len(set(plain_kmers(t, k))) for t in seqs]
    assert [int(x) for x in want["distinct_per_pivot"]] == [len(set(plain_kmers(t, k))) for t in pivots]
    assert int(want["within_hist"].sum()) > 0 and int(want["across_hist"].sum()) > 0
