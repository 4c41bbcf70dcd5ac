"""The set forms of kh_exp2_run, kh_exp3_run and kh_exp4_run (exp2_sets, exp3_sets, exp4_sets in kh_engine.cpp: what
answers for every k above the presence bitmaps and whenever they decline), the output subsets of the four kh_exp*_run
calls through the C ABI, and the k = 13 bitmaps behind KHOICE_BMP_MAX_K.

Everything is compared with the k-independent restatements of the neighbouring modules (tests/test_gpu_exp2_bmp.py,
tests/test_gpu_exp3.py, tests/test_gpu_exp4.py: `oracle`, over oracle/kmer_oracle.py and oracle/merge_oracle.py), type
1 with the C restatement (oracle/c_oracle.py): integers equal, `rows` equal as float64.  A case that goes through the
set form also shows it in the statistics: no bmp_* launch, set-operation launches, no retry, and every text built once.

  A  the shapes the bitmap forms are tested on, at k = 13, 16, 32, 33 and 64 (the first k above the bitmaps, the last k
     of the directly addressed tables, the one-word limit, the first two-word k, the widest)
  B  cs x hist_len (x pivot_cs) in the set form, one-word and two-word keys
  C  what only the set form meets: a group without k-mers, nothing but such groups, a group of 130 genomes (fan-in above
     KH_MAX_INPUT_SETS = 128), 130 and 258 groups of one genome (a rest-of-groups union of 129 and of 257 operands, the
     second with counters above 255), membership masks of two and three words
  D  the order of the type-4 sum with one-word and two-word keys
  E  every output NULL on its own, present on its own, all present, all NULL, into arrays filled with 0xA5 and followed by
     guards, for kh_exp1_run .. kh_exp4_run in every form
  F  KHOICE_BMP_MAX_K = 13 and = 14, KHOICE_BMP_RANGE_BITS = 16, 17, 19

The unmarked tests at the end prove on the CPU, on the oracle's sets, that the cases are what they claim."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import c_oracle as CO
from oracle import kmer_oracle as O
from tests import test_gpu_bmp as X1
from tests import test_gpu_exp2_bmp as X2
from tests import test_gpu_exp3 as X3
from tests import test_gpu_exp4 as X4

SET_K = (13, 16, 32, 33, 64)
CORNER_K = (21, 41)
ONE_WORD = 32                    # k <= 32: one 64-bit word per key
LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def eng():
    from khoice_amd import build as kbuild
    from khoice_amd import engine as E
    kbuild.build_library()
    e = E.Engine(0)
    yield e
    e.close()


# ---------------------------------------------------------------- the set form, as the statistics show it
def set_form(d, ntexts, launches=True):
    """No bitmap kernel, set-operation launches, nothing planned twice, every text built once.  launches = False: the
    case holds no k-mer at all, so every set operation of the form is answered without a launch; the operations
    themselves are still counted (`setops`)."""
    assert all(v == 0 for n, v in d.items() if n.startswith("bmp_")), d
    assert d["union_tagged"] == 0 and d["skm_union"] == 0, d
    if launches:
        assert d["setop"] > 0, d
    else:
        assert d["setop"] == 0 and d["setops"] > 0 and d["setop_in"] == 0, d
    assert d["retries"] == 0 and d["builds"] == ntexts, d


def sets2(eng, case, k, launches=True, **kw):
    seqs, group_of, pivots, pivot_group = case
    got, d = (X2.by_sets if launches else X2.run)(eng, seqs, group_of, pivots, pivot_group, k, **kw)
    set_form(d, len(seqs) + len(pivots), launches)
    return got


def sets3(eng, case, k, launches=True, **kw):
    seqs, group_of, pivots = case[:3]
    got, d = (X3.by_sets if launches else X3.run)(eng, seqs, group_of, pivots, k, **kw)
    set_form(d, len(seqs) + len(pivots), launches)
    return got


def sets4(eng, case, k, launches=True, **kw):
    seqs, group_of, pivots = case
    got, d = (X4.by_sets if launches else X4.run)(eng, seqs, group_of, pivots, k, **kw)
    set_form(d, len(seqs) + len(pivots), launches)
    return got


def top_bin(hist):
    hit = np.flatnonzero(hist)
    return int(hit.max()) if hit.size else 0


# ---------------------------------------------------------------- A. the bitmap forms' shapes at every key width
EXP2_SHAPES = [("counter_widths", 16), ("counter_widths", 33), ("two_and_none", 13), ("two_and_none", 64),
               ("one_group", 32), ("one_group", 64), ("groups65", 13), ("groups65", 33), ("many_pivots", 32),
               ("many_pivots", 64)]
EXP3_READ_SHAPED = SET_K
EXP3_WALKS = [(6, 16), (6, 33), (15, 32), (15, 33)]
EXP4_SHAPES = [("one_group", 13), ("one_group", 33), ("one_pivot", 16), ("one_pivot", 64), ("five_pivots", 32),
               ("five_pivots", 33), ("no_pivot", 13), ("no_pivot", 64), ("counter_widths", 16), ("counter_widths", 33),
               ("groups64", 32), ("groups64", 64), ("groups65", 13), ("groups65", 64)]
SHAPE_LENGTH = 3_000


@pytest.mark.gpu
@pytest.mark.parametrize("name,k", EXP2_SHAPES)
def test_exp2_set_form_shapes(eng, name, k):
    got = sets2(eng, X2.shape_case(name, SHAPE_LENGTH), k)
    if name == "counter_widths":
        assert (got["within_hist"][5] == 0).all() and got["within_only"][5] == 0 and got["distinct_per_pivot"][5] == 0
        assert got["within_only"][1] == 0                                   # the pivot that is a genome of its group
        assert top_bin(got["within_hist"][4]) > 1 + 17                      # counts only the group of 70 can give
    if name == "one_group":
        assert (got["across_hist"] == 0).all() and (got["across_only"] == got["distinct_per_pivot"]).all()
    if name == "groups65":
        assert min(top_bin(h) for h in got["across_hist"]) > 1 + 2          # k-mers in several of the 64 other groups


@pytest.mark.gpu
@pytest.mark.parametrize("k", EXP3_READ_SHAPED)
def test_exp3_set_form_read_shaped_pivots(eng, k):
    seqs, group_of, pivots, names = X3.read_shaped_case(k)
    got = sets3(eng, (seqs, group_of, pivots), k)
    assert got["distinct_per_pivot"][names.index("empty")] == 0 and got["distinct_per_pivot"][names.index("shorter_than_k")] == 0
    assert (got["inter_hist"][names.index("empty")] == 0).all()
    assert got["distinct_per_pivot"][names.index("edge_records")] > 0
    p = names.index("a_genome")                                           # identical to a genome of group 1: every k-mer of it is met there
    assert got["inter_hist"][p, 1].sum() == got["distinct_per_pivot"][p] == got["distinct_per_seq"][2] > 0
    none, d = X3.run(eng, seqs, group_of, [], k)                          # no pivots: the genomes are built, nothing else runs
    assert all(v == 0 for n, v in d.items() if n.startswith("bmp_")) and d["retries"] == 0 and d["builds"] == len(seqs), d
    assert none["inter_hist"].shape == (0, 3, 5001) and (none["distinct_per_seq"] == got["distinct_per_seq"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("npiv,k", EXP3_WALKS)
def test_exp3_set_form_walks(eng, npiv, k):
    got = sets3(eng, X3.walk_case(npiv), k)
    assert got["inter_hist"][:, 3, 2:19].sum() > 0 and got["inter_hist"][:, 4, 18:35].sum() > 0   # as in the bitmap test


@pytest.mark.gpu
@pytest.mark.parametrize("name,k", EXP4_SHAPES)
def test_exp4_set_form_shapes(eng, name, k):
    got = sets4(eng, X4.shape_case(name), k)
    if name == "five_pivots":
        for p in (0, 1):
            assert (got["rows"][p] == 0).all() and got["unique"][p] == 0 and got["distinct_per_pivot"][p] == 0
        assert got["unique"][2] == 0 and got["rows"][2, 1] > 0             # the pivot that is a genome of group 1
    if name == "no_pivot":
        assert got["rows"].shape == (0, 3) and got["unique"].shape == (0,)
    if name == "counter_widths":
        assert top_bin(got["within_hist"][3]) > 17                         # counts only the group of 70 can give
    if name in ("groups64", "groups65"):
        assert (got["rows"][:, int(name[-2:]) - 1] > 0).all()              # bit 63 of word 0, bit 0 of word 1


# ---------------------------------------------------------------- B. clamps in the set form
CLAMPS = [(cs, hl) for cs in (1, 2, 3, 5000) for hl in (2, 3, 4, 5001)]
PIVOT_CS = (1, 2, 255, 2 ** 32 - 1)
PLANT_MULTS = (2, 3, 255, 256, 301)


def clean_piece(text, at, n):
    """n bases of a text from `at` on, or from the first place behind it where no record ends."""
    while not set(text[at:at + n]) <= set(b"ACGT"):
        at += n
    assert at + n <= len(text)
    return text[at:at + n]


@functools.lru_cache(maxsize=None)
def clamp_case4(k):
    """species(8_000) of tests/test_gpu_exp4.py and a fourth pivot of planted records: a k-base record repeated 2, 3,
    255, 256 and 301 times (taken from genomes of the three groups in turn, so the rows feel every pivot_cs), one that
    no group holds 300 times (the unique count feels it), and a stretch of single k-mers; N between the records."""
    seqs, group_of, pivots = X4.species(8_000)
    rng = np.random.default_rng(500 + k)
    recs = []
    for j, m in enumerate(PLANT_MULTS):
        recs += [clean_piece(seqs[(3 * j) % len(seqs)], 500 + 200 * j, k)] * m
    recs += [LETTERS[rng.integers(0, 4, k)].tobytes()] * 300
    recs += [clean_piece(pivots[0], 2_000, 4 * k)]
    recs = [recs[i] for i in rng.permutation(len(recs))]
    return seqs, group_of, pivots + [b"N".join(recs)]


@pytest.mark.gpu
@pytest.mark.parametrize("cs,hist_len", CLAMPS)
@pytest.mark.parametrize("k", CORNER_K)
def test_exp2_set_form_clamps(eng, k, cs, hist_len):
    sets2(eng, X2.species(8_000), k, cs=cs, hist_len=hist_len)


@pytest.mark.gpu
@pytest.mark.parametrize("cs,hist_len", CLAMPS)
@pytest.mark.parametrize("k", CORNER_K)
def test_exp3_set_form_clamps(eng, k, cs, hist_len):
    sets3(eng, X3.species(8_000), k, cs=cs, hist_len=hist_len)


@pytest.mark.gpu
@pytest.mark.parametrize("cs,hist_len", CLAMPS)
@pytest.mark.parametrize("k", CORNER_K)
def test_exp4_set_form_clamps(eng, k, cs, hist_len):
    rows = []
    for pivot_cs in PIVOT_CS:
        got = sets4(eng, clamp_case4(k), k, cs=cs, hist_len=hist_len, pivot_cs=pivot_cs)
        rows.append(got["rows"][3].tobytes() + got["unique"][3].tobytes())
    assert len(set(rows)) == len(PIVOT_CS)                                 # every pivot_cs, another answer


# ---------------------------------------------------------------- C. corners only the set form has
NO_KMERS = (b"ACGTACGT", b"N" * 50)      # shorter than any k here, and nothing but N
WHERE = {"first": 0, "middle": 2, "last": 3}


@functools.lru_cache(maxsize=None)
def empty_group_case(where):
    """3 groups x 2 related genomes and, as group `where` of the four, one whose genomes hold no k-mer; a pivot per
    group, the last one the empty group's.  Returns seqs, group_of, pivots, pivot_group."""
    rng = np.random.default_rng(610 + where)
    fam = [X2.related(rng, 3, SHAPE_LENGTH) for _ in range(3)]
    groups = [f[:2] for f in fam]
    groups.insert(where, list(NO_KMERS))
    full = [g for g in range(4) if g != where]
    return ([t for g in groups for t in g], [g for g, m in enumerate(groups) for _ in m],
            [f[2] for f in fam] + [fam[0][2][:1_500]], full + [where])


@functools.lru_cache(maxsize=None)
def all_empty_case():
    """Three groups of genomes without k-mers and three pivots without: empty, short, nothing but N."""
    return list(NO_KMERS) * 3, [0, 0, 1, 1, 2, 2], [b"", b"ACGTAC", b"N" * 25], [0, 1, 2]


@functools.lru_cache(maxsize=None)
def big_group_case():
    """One group of 130 genomes of 1 kbp, close enough to their ancestor that k-mers lie in 129 and in all 130 of them;
    two pivots of the same ancestor."""
    fam = X2.related(np.random.default_rng(620), 132, 1_000, rate=0.0003)
    return fam[:130], [0] * 130, fam[130:], [0, 0]


@functools.lru_cache(maxsize=None)
def many_groups_case(ngroups):
    """ngroups groups of one genome of one ancestor, pivots held out of the first, a middle and the last group: the union
    of the other groups takes ngroups - 1 operands, and k-mers lie in all of them."""
    fam = X2.related(np.random.default_rng(630 + ngroups), ngroups + 3, 1_000 if ngroups < 200 else 400, rate=0.0003)
    return fam[:ngroups], list(range(ngroups)), fam[ngroups:], [0, ngroups // 2, ngroups - 1]


@functools.lru_cache(maxsize=None)
def wide_mask_case(ngroups):
    """ngroups groups of one genome of one ancestor; the last genome also holds a text of its own.  Both pivots hold
    k-mers of the ancestor that every group holds, the first also k-mers of that private text."""
    rng = np.random.default_rng(640 + ngroups)
    fam = X2.related(rng, ngroups + 1, 1_000, rate=0.0003)
    private = LETTERS[rng.integers(0, 4, 400)].tobytes()
    seqs = fam[:ngroups - 1] + [fam[ngroups - 1] + b"N" + private]
    return seqs, list(range(ngroups)), [fam[ngroups][:700] + b"N" + private[20:380], fam[ngroups][300:]]


@pytest.mark.gpu
@pytest.mark.parametrize("k", CORNER_K)
@pytest.mark.parametrize("where", list(WHERE))
def test_exp2_set_form_empty_group(eng, where, k):
    got = sets2(eng, empty_group_case(WHERE[where]), k)
    assert (got["within_hist"][3] == 0).all() and got["within_only"][3] == got["distinct_per_pivot"][3] > 0
    assert got["across_hist"][3].sum() > 0 and (got["within_hist"][:3].sum(axis=1) > 0).all()   # the empty group's pivot
                                                                          # meets the group of its own ancestor across


@pytest.mark.gpu
@pytest.mark.parametrize("k", CORNER_K)
@pytest.mark.parametrize("where", list(WHERE))
def test_exp3_set_form_empty_group(eng, where, k):
    g = WHERE[where]
    got = sets3(eng, empty_group_case(g), k)
    assert (got["inter_hist"][:, g] == 0).all() and all(got["inter_hist"][:, h].sum() > 0 for h in range(4) if h != g)


@pytest.mark.gpu
@pytest.mark.parametrize("k", CORNER_K)
@pytest.mark.parametrize("where", list(WHERE))
def test_exp4_set_form_empty_group(eng, where, k):
    g = WHERE[where]
    got = sets4(eng, empty_group_case(g)[:3], k)
    assert (got["rows"][:, g] == 0).all() and (got["within_hist"][g] == 0).all()
    assert all((got["rows"][:, h] > 0).any() and got["within_hist"][h].sum() > 0 for h in range(4) if h != g)


@pytest.mark.gpu
@pytest.mark.parametrize("k", CORNER_K)
def test_set_forms_without_any_kmer(eng, k):
    seqs, group_of, pivots, pivot_group = all_empty_case()
    got = sets2(eng, (seqs, group_of, pivots, pivot_group), k, launches=False)
    assert all((got[f] == 0).all() for f in X2.FIELDS)
    got = sets3(eng, (seqs, group_of, pivots), k, launches=False)
    assert all((got[f] == 0).all() for f in X3.FIELDS)
    got = sets4(eng, (seqs, group_of, pivots), k, launches=False)
    assert all((got[f] == 0).all() for f in X4.FIELDS)
    got = sets3(eng, X3.species(8_000)[:2] + (pivots,), k)                 # every pivot empty, the groups are not
    assert (got["inter_hist"] == 0).all() and (got["distinct_per_pivot"] == 0).all() and (got["distinct_per_seq"] > 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("cs", (5000, 100))
@pytest.mark.parametrize("k", CORNER_K)
def test_set_forms_group_of_130_genomes(eng, k, cs):
    seqs, group_of, pivots, pivot_group = big_group_case()
    over = slice(130, None) if cs == 5000 else slice(100, 101)            # 1 + 129 and 1 + 130; both saturate at cs = 100
    got = sets2(eng, (seqs, group_of, pivots, pivot_group), k, cs=cs)
    assert (got["within_hist"][:, over].sum(axis=1) > 0).all() and (got["across_hist"] == 0).all()
    got = sets3(eng, (seqs, group_of, pivots), k, cs=cs)
    assert (got["inter_hist"][:, 0, over].sum(axis=1) > 0).all()
    got = sets4(eng, (seqs, group_of, pivots), k, cs=cs)
    assert got["within_hist"][0, slice(129, None) if cs == 5000 else slice(100, 101)].sum() > 0
    if cs == 100:
        assert (got["within_hist"][0, 101:] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("k", CORNER_K)
@pytest.mark.parametrize("ngroups", (130, 258))
def test_exp2_set_form_many_groups(eng, ngroups, k):
    got = sets2(eng, many_groups_case(ngroups), k)
    assert (got["across_hist"][:, ngroups - 1:].sum(axis=1) > 0).all()     # k-mers in ngroups - 2 and - 1 other groups


@pytest.mark.gpu
@pytest.mark.parametrize("k", CORNER_K)
@pytest.mark.parametrize("ngroups", (65, 129))
def test_exp4_set_form_wide_masks(eng, ngroups, k):
    got = sets4(eng, wide_mask_case(ngroups), k)
    assert (got["rows"] > 0).all() and got["rows"][0, ngroups - 1] > got["rows"][0, :ngroups - 1].max()


# ---------------------------------------------------------------- D. the order of the type-4 sum
@pytest.mark.gpu
@pytest.mark.parametrize("k", CORNER_K)
def test_exp4_set_form_sums_in_key_order(eng, k):
    sets4(eng, X4.order_case(), k)


# ---------------------------------------------------------------- E. output subsets and dirty buffers through the C ABI
FILL, GUARD = 0xA5, 8
ABI_HIST_LEN = 96
OUTPUTS = {1: ("within_hist", "across_hist", "distinct_per_seq", "group_sets", "across_set"),
           2: X2.FIELDS, 3: X3.FIELDS, 4: X4.FIELDS}
HANDLES = ("group_sets", "across_set")


class Out:
    """An array handed to the library: every byte 0xA5, and a guard of 8 more elements of the same fill behind it."""

    def __init__(self, shape, dtype):
        self.shape, self.dtype = shape, np.dtype(dtype)
        self.nbytes = int(np.prod(shape)) * self.dtype.itemsize
        self.raw = np.full(self.nbytes + GUARD * self.dtype.itemsize, FILL, dtype=np.uint8)

    def arg(self, ctype):
        return C.cast(self.raw.ctypes.data, C.POINTER(ctype))

    def value(self):
        return self.raw[:self.nbytes].view(self.dtype).reshape(self.shape)

    def guard_intact(self):
        return bool((self.raw[self.nbytes:] == FILL).all())


def abi_call(eng, kind, case, k, present, cs=5000, hist_len=ABI_HIST_LEN, pivot_cs=X4.KMC_CS):
    """kh_exp{kind}_run on the engine's library handle and context with the outputs in `present` and NULL for the others.
    Returns the return code and {name: Out}."""
    lib, ctx = eng._lib, eng._ctx
    seqs, group_of, pivots = case[0], case[1], (case[2] if kind != 1 else [])
    n, npv, ng = len(seqs), len(pivots), max(group_of) + 1
    ptrs, lens, on_dev, keep = eng._seq_args(seqs)
    gof = (C.c_int * n)(*group_of)
    if kind != 1:
        pptrs, plens, _, pkeep = eng._seq_args(pivots)
    shapes = {1: {"within_hist": (ng, hist_len), "across_hist": (hist_len,), "distinct_per_seq": (n,), "group_sets": (ng,),
                  "across_set": (1,)},
              2: {"within_hist": (npv, hist_len), "across_hist": (npv, hist_len), "within_only": (npv,), "across_only": (npv,),
                  "distinct_per_seq": (n,), "distinct_per_pivot": (npv,)},
              3: {"inter_hist": (npv, ng, hist_len), "distinct_per_seq": (n,), "distinct_per_pivot": (npv,)},
              4: {"rows": (npv, ng), "unique": (npv,), "within_hist": (ng, hist_len), "distinct_per_seq": (n,),
                  "distinct_per_pivot": (npv,)}}[kind]
    assert set(shapes) == set(OUTPUTS[kind]) >= set(present)
    outs = {name: Out(shapes[name], np.float64 if name == "rows" else np.uint64) for name in present}

    def a(name):
        if name not in outs:
            return None
        return outs[name].arg(C.c_double if name == "rows" else C.c_void_p if name in HANDLES else C.c_uint64)

    u64 = lambda arr: arr.ctypes.data_as(C.POINTER(C.c_uint64))
    if kind == 1:
        rc = lib.kh_exp1_run(ctx, n, ptrs, u64(lens), on_dev, gof, ng, k, cs, a("within_hist"), a("across_hist"), hist_len,
                             a("distinct_per_seq"), a("group_sets"), a("across_set"))
    elif kind == 2:
        pgof = (C.c_int * npv)(*case[3])
        rc = lib.kh_exp2_run(ctx, n, ptrs, u64(lens), on_dev, gof, ng, npv, pptrs, u64(plens), pgof, k, cs, a("within_hist"),
                             a("across_hist"), hist_len, a("within_only"), a("across_only"), a("distinct_per_seq"),
                             a("distinct_per_pivot"))
    elif kind == 3:
        rc = lib.kh_exp3_run(ctx, n, ptrs, u64(lens), on_dev, gof, ng, npv, pptrs, u64(plens), k, cs, a("inter_hist"), hist_len,
                             a("distinct_per_seq"), a("distinct_per_pivot"))
    else:
        rc = lib.kh_exp4_run(ctx, n, ptrs, u64(lens), on_dev, gof, ng, npv, pptrs, u64(plens), k, cs, pivot_cs,
                             a("within_hist"), hist_len, a("rows"), a("unique"), a("distinct_per_seq"), a("distinct_per_pivot"))
    return rc, outs


def handle_histograms(eng, out, hist_len):
    """The counter histograms of the sets an output of handles holds; the sets are freed."""
    hists = []
    for h in out.value().tolist():
        hist = np.zeros(hist_len, dtype=np.uint64)
        rc = eng._lib.kh_histogram(eng._ctx, C.c_void_p(h), hist.ctypes.data_as(C.POINTER(C.c_uint64)), hist_len)
        eng._lib.kh_set_free(C.c_void_p(h))
        assert rc == 0, rc
        hists.append(hist)
    return np.array(hists)


def output_subsets(names, all_null):
    """Everything, each output NULL on its own, each present on its own, and nothing at all."""
    yield tuple(names)
    for name in names:
        yield tuple(n for n in names if n != name)
    for name in names:
        yield (name,)
    if all_null:
        yield ()


def abi_check(eng, kind, case, k, want, bmp=None, hist_len=ABI_HIST_LEN):
    """Every subset of the outputs: the call returns 0, what was asked for is the oracle's, no guard is touched.  bmp:
    whether k_bmp_build must (True) or must not (False) have run in every call."""
    eng.profile(True)
    try:
        for present in output_subsets(OUTPUTS[kind], kind in (1, 4)):
            b0 = eng.stats()["kernels"]["bmp_build"]["launches"]
            rc, outs = abi_call(eng, kind, case, k, present, hist_len=hist_len)
            assert rc == 0, (kind, k, present, rc, eng._lib.kh_last_error())
            launched = eng.stats()["kernels"]["bmp_build"]["launches"] - b0
            if bmp is not None:
                assert (launched > 0) == bmp, (kind, k, present, launched)
            for name, out in outs.items():
                assert out.guard_intact(), (kind, k, present, name)
                if name == "group_sets":
                    got, ref = handle_histograms(eng, out, hist_len), want["within_hist"]
                elif name == "across_set":
                    got, ref = handle_histograms(eng, out, hist_len)[0], want["across_hist"]
                else:
                    got, ref = out.value(), want[name]
                assert got.shape == ref.shape and got.dtype == ref.dtype, (kind, k, present, name, got.shape, ref.shape)
                assert (got == ref).all(), (kind, k, present, name, np.argwhere(got != ref)[:8].tolist())
    finally:
        eng.profile(False)


@functools.lru_cache(maxsize=None)
def two_pass_case():
    """One group of 70 genomes of 2 kbp next to two groups of two: more than the 64 genomes of one fused batch."""
    rng = np.random.default_rng(650)
    fam = [X2.related(rng, n, 2_000) for n in (2, 70, 2)]
    return [t for f in fam for t in f], [g for g, f in enumerate(fam) for _ in f]


@pytest.mark.gpu
@pytest.mark.parametrize("k", (9, 15, 21, 31, 41))
@pytest.mark.parametrize("shape", ("species", "two_pass"))
def test_abi_exp1_output_subsets(eng, shape, k):
    seqs, group_of = X1.species(8_000) if shape == "species" else two_pass_case()
    want = CO.exp1(seqs, group_of, k, cs=5000, hist_len=ABI_HIST_LEN)
    abi_check(eng, 1, (seqs, group_of), k, want)
    got = eng.exp1_run(seqs, group_of, k, cs=5000, hist_len=ABI_HIST_LEN)  # and the context still answers
    assert all((got[f] == want[f]).all() for f in X1.FIELDS)


@pytest.mark.gpu
@pytest.mark.parametrize("k", (9, 21))
def test_abi_exp2_output_subsets(eng, k):
    case = X2.species(8_000)
    abi_check(eng, 2, case, k, X2.oracle(*case, k, hist_len=ABI_HIST_LEN), bmp=k <= 12)
    X2.run(eng, *case, k)


@pytest.mark.gpu
@pytest.mark.parametrize("k", (9, 21))
def test_abi_exp3_output_subsets(eng, k):
    case = X3.species(8_000)
    abi_check(eng, 3, case, k, X3.oracle(*case, k, hist_len=ABI_HIST_LEN), bmp=k <= 12)
    X3.run(eng, *case, k)


@pytest.mark.gpu
@pytest.mark.parametrize("k", (9, 21))
def test_abi_exp4_output_subsets(eng, k):
    case = X4.species(8_000)
    abi_check(eng, 4, case, k, X4.oracle(*case, k, hist_len=ABI_HIST_LEN), bmp=k <= 12)
    X4.run(eng, *case, k)


# ---------------------------------------------------------------- F. k = 13 bitmaps behind the documented switch
@pytest.fixture
def bmp13(monkeypatch):
    monkeypatch.setenv("KHOICE_BMP_MAX_K", "13")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ("species", "range_edges"))
def test_bmp13_exp1(eng, bmp13, case):
    if case == "species":
        seqs, group_of = X1.species()
        X1.check(eng, seqs, group_of, 13)
    else:
        seqs, group_of, codes, subsets = X1.range_case(13)
        got, _ = X1.check(eng, seqs, group_of, 13, hist_len=8)
        assert int(got["distinct_per_seq"].sum()) == sum(bin(m).count("1") for m in subsets)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ("species", "many_pivots"))
def test_bmp13_exp2(eng, bmp13, case):
    X2.check(eng, *(X2.species() if case == "species" else X2.shape_case("many_pivots", SHAPE_LENGTH)), 13)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ("species", "walk7"))
def test_bmp13_exp3(eng, bmp13, case):
    X3.check(eng, *(X3.species() if case == "species" else X3.walk_case(7)), 13)


@pytest.mark.gpu
def test_bmp13_exp4_one_pivot(eng, bmp13):
    got, _ = X4.check(eng, *X4.shape_case("one_pivot"), 13)
    assert got["rows"][0, 1] > 0 and got["unique"][0] > 0                  # a further genome of group 1's ancestor


@pytest.mark.gpu
def test_bmp_max_k_14_leaves_k14_to_the_other_forms(eng, monkeypatch):
    monkeypatch.setenv("KHOICE_BMP_MAX_K", "14")
    seqs, group_of = X1.species(8_000)
    X1.not_taken(eng, seqs, group_of, 14, None, True)
    sets2(eng, X2.species(8_000), 14)
    sets3(eng, X3.species(8_000), 14)
    sets4(eng, X4.species(8_000), 14)
    X1.check(eng, seqs, group_of, 13)                                      # 13 itself is inside the switch's range


@pytest.mark.gpu
@pytest.mark.parametrize("range_bits", (16, 17, 19))
def test_bmp_range_bits_at_k12(eng, monkeypatch, range_bits):
    """Ranges of 2^16 codes: 256 of them, picked by four leading bases; 2^17 and 2^19: odd numbers of leading bits, so 128
    and 32 ranges without the pre-filter."""
    monkeypatch.setenv("KHOICE_BMP_RANGE_BITS", str(range_bits))
    seqs, group_of, codes, subsets = X1.range_case(12)
    got, _ = X1.check(eng, seqs, group_of, 12, hist_len=8)
    assert int(got["distinct_per_seq"].sum()) == sum(bin(m).count("1") for m in subsets)


# ---------------------------------------------------------------- preconditions, without a GPU
def test_every_shape_at_both_key_widths_and_every_k_in_every_type():
    for shapes in (EXP2_SHAPES, EXP4_SHAPES, [(f"walk{n}", k) for n, k in EXP3_WALKS]):
        for name in {n for n, _ in shapes}:
            ks = [k for n, k in shapes if n == name]
            assert min(ks) <= ONE_WORD < max(ks), name
    assert {n for n, _ in EXP2_SHAPES} == {"counter_widths", "two_and_none", "one_group", "groups65", "many_pivots"}
    assert {n for n, _ in EXP4_SHAPES} == {"one_group", "one_pivot", "five_pivots", "no_pivot", "counter_widths", "groups64",
                                           "groups65"}
    assert {n for n, _ in EXP3_WALKS} == {6, 15}
    assert {k for _, k in EXP2_SHAPES} == {k for _, k in EXP4_SHAPES} == set(EXP3_READ_SHAPED) == set(SET_K)
    for k in SET_K:                                                        # the read-shaped pivots are what they were at k <= 12
        seqs, group_of, pivots, names = X3.read_shaped_case(k)
        recs = pivots[names.index("edge_records")].split(b"\n")
        assert [len(r) for r in recs[:4]] == [k - 1, k, k + 1, 0] and set(recs[4]) == {ord("N")} and recs[5].islower()
        assert pivots[names.index("empty")] == b"" and len(pivots[names.index("shorter_than_k")]) == k - 1
        assert pivots[names.index("a_genome")] == seqs[2] and pivots[names.index("reads")].count(b"\n") == 29


@pytest.mark.parametrize("k", CORNER_K)
def test_clamp_pivot_holds_every_multiplicity(k):
    seqs, group_of, pivots = clamp_case4(k)
    raw = X4.counted(pivots[3], k, 1 << 40)
    mults = set(raw.values())
    assert mults >= {1, 2, 3, 255, 256, 300, 301} and max(mults) > 300
    group_sets = [set().union(*[set(X4.plain_set(t, k)) for t, g in zip(seqs, group_of) if g == h]) for h in range(3)]
    held = {m: [g for g in range(3) if code in group_sets[g]] for code, m in raw.items() if m > 1}
    assert all(held[m] for m in PLANT_MULTS) and held[300] == []           # in a group each, and the one no group holds
    assert {g for m in PLANT_MULTS for g in held[m]} == {0, 1, 2}
    answers = set()
    for pivot_cs in PIVOT_CS:
        want = X4.oracle(seqs, group_of, pivots, k, pivot_cs=pivot_cs)
        assert set(X4.counted(pivots[3], k, pivot_cs).values()) == {min(m, pivot_cs) for m in mults}
        answers.add(want["rows"][3].tobytes() + want["unique"][3].tobytes())
    assert len(answers) == len(PIVOT_CS)                                   # every pivot_cs changes rows or unique count


@pytest.mark.parametrize("k", CORNER_K)
def test_corner_cases_are_what_they_claim(k):
    for where in WHERE.values():
        seqs, group_of, pivots, pivot_group = empty_group_case(where)
        sizes = [sum(len(X2.plain_set(t, k)) for t, g in zip(seqs, group_of) if g == h) for h in range(4)]
        assert [s == 0 for s in sizes] == [h == where for h in range(4)] and group_of.count(where) == 2
        assert pivot_group[3] == where and sorted(pivot_group) == [0, 1, 2, 3] and all(len(X2.plain_set(p, k)) for p in pivots)
    seqs, group_of, pivots, pivot_group = all_empty_case()
    assert not any(X2.plain_set(t, k) for t in seqs + pivots) and max(len(t) for t in seqs + pivots) >= k
    # the group of 130 genomes: counters of 129 and 130, and both pivots hold such k-mers
    seqs, group_of, pivots, pivot_group = big_group_case()
    assert len(seqs) == 130 > 128 and set(group_of) == {0}
    union = O.union_sum([X2.plain_set(t, k) for t in seqs], 5000)
    assert {129, 130} <= set(union.values())
    for p in pivots:
        assert {union.get(code, 0) for code in X2.plain_set(p, k)} >= {129, 130}
    # many groups: every pivot has k-mers in ngroups - 2 and in all ngroups - 1 other groups (129 and 257 operands; 257 > 255)
    for ngroups in (130, 258):
        seqs, group_of, pivots, pivot_group = many_groups_case(ngroups)
        assert group_of == list(range(ngroups)) and pivot_group == [0, ngroups // 2, ngroups - 1]
        sets = [X2.plain_set(t, k) for t in seqs]
        for p, g in zip(pivots, pivot_group):
            others = O.union_sum([s for h, s in enumerate(sets) if h != g], 5000)
            assert {others.get(code, 0) for code in X2.plain_set(p, k)} >= {ngroups - 2, ngroups - 1}
    # wide masks: k-mers of the first pivot that the last group alone holds, and that every group holds
    for ngroups in (65, 129):
        seqs, group_of, pivots = wide_mask_case(ngroups)
        assert group_of == list(range(ngroups)) and (ngroups + 63) // 64 == {65: 2, 129: 3}[ngroups]
        sets = [X4.plain_set(t, k) for t in seqs]
        holders = [[g for g, s in enumerate(sets) if code in s] for code in X4.plain_set(pivots[0], k)]
        assert sum(h == [ngroups - 1] for h in holders) >= 300 and sum(len(h) == ngroups for h in holders) >= 10
        assert any(len([g for g, s in enumerate(sets) if code in s]) == ngroups for code in X4.plain_set(pivots[1], k))


def test_two_pass_case_has_a_group_above_one_batch():
    seqs, group_of = two_pass_case()
    assert [group_of.count(g) for g in range(3)] == [2, 70, 2] and all(len(t) == 2_000 for t in seqs)


def test_range_case_13_holds_every_block_edge():
    k = 13
    seqs, group_of, codes, subsets = X1.range_case(k)
    nblocks = 4 ** k >> X1.BLOCK_BITS
    assert nblocks == 1024 and len(codes) == 2 * nblocks and len(set(codes)) == len(codes)
    for b in range(nblocks):
        first, last = codes[2 * b], codes[2 * b + 1]
        lo, hi = b << X1.BLOCK_BITS, ((b + 1) << X1.BLOCK_BITS) - 1
        assert lo <= first < last <= hi and first <= X1.revcomp_code(first, k) and last <= X1.revcomp_code(last, k)
        assert all(c > X1.revcomp_code(c, k) for c in range(lo, first))
        assert all(c > X1.revcomp_code(c, k) for c in range(last + 1, hi + 1))
    assert codes[0] == 0
    plants = [(c, {g for g in range(4) if (m >> g) & 1}) for c, m in zip(codes, subsets)]
    want = CO.exp1(seqs, group_of, k, hist_len=8)
    mine = X1.planted_histograms(group_of, plants, 5000, 8)
    for f in X1.FIELDS:
        assert (want[f] == mine[f]).all(), f
