"""The presence-bitmap forms (khoice_amd/csrc/kh_bmp.hip: k_bmp_readout, k_bmp_pivot, k_bmp_cross, k_bmp_present and
k_bmp_member, driven by exp1_bmp .. exp4_bmp of kh_engine.cpp) at the limits their contract states: up to KH_BMP_MAX_COUNT
genomes per group and as many groups, KH_BMP_MAX_BINS bins, KH_BMP_CROSS_PIVOTS pivots a launch.  Every slice of the
bit-sliced counters c[] and a[] holds a bit here, both sides of each of the four bins rules are met exactly, the
four-wave hand-over of k = 11 and 12 sees long groups that end on and off a round, the histograms are folded above
255, and the replicas are taken modulo a count that is no power of two.

Every input is planted: a text is a list of distinct canonical k-mers joined by N, and each code occurs in exactly the
genomes, groups and pivots its case says.  Every GPU test is bit-exact against the oracle of its form (CO.exp1 for type
1, the oracle() of tests/test_gpu_exp2_bmp.py, test_gpu_exp3.py and test_gpu_exp4.py for types 2 to 4) and reads from
the statistics that the bitmap kernels, and only they, did the work; a declining shape gives the same answer without
a bitmap launch and without a retry.  The unmarked tests at the end prove the cases on the CPU: the codes are canonical
and distinct, every text holds exactly the intended set, every group has the intended size, every edge count occurs,
and the bins rules, restated here, give the values the case names claim."""
import functools
import os
import random
import re

import pytest

from oracle import c_oracle as CO
from tests import test_gpu_bmp as B1
from tests import test_gpu_exp2_bmp as X2
from tests import test_gpu_exp3 as X3
from tests import test_gpu_exp4 as X4
from tests.test_gpu_bmp import canonical_codes, edge_counts, kmer_text, planted_histograms, revcomp_code

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "khoice_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def _constant(text, decl):
    return int(re.search(decl + r" = (\d+);", text).group(1))


MAX_COUNT = _constant(_src("kh_launch.h"), "constexpr u32 KH_BMP_MAX_COUNT")
MAX_BINS = _constant(_src("kh_launch.h"), "constexpr u32 KH_BMP_MAX_BINS")
CROSS_PIVOTS = _constant(_src("kh_launch.h"), "constexpr u32 KH_BMP_CROSS_PIVOTS")
MEMBER_GROUPS = _constant(_src("kh_launch.h"), "constexpr u32 KH_BMP_MEMBER_GROUPS")
SLICES = _constant(_src("kh_bmp.hip"), "constexpr int BMP_SLICES")

BMP_KERNELS = ("bmp_build", "bmp_readout", "bmp_pivot", "bmp_cross", "bmp_count", "bmp_present", "bmp_member")
FIELDS1 = B1.FIELDS
# (cs, hist_len): neither clamps; cs inside the counts; the last bin inside the counts; both at the largest count and one
# below it; both at the bottom
SATURATIONS = ((5000, 5001), (300, 5001), (5000, 257), (MAX_COUNT, MAX_COUNT + 1), (MAX_COUNT - 1, MAX_COUNT), (2, 3))


@pytest.fixture(scope="module")
def eng():
    from khoice_amd import build as kbuild
    from khoice_amd import engine as E
    kbuild.build_library()
    e = E.Engine(0)
    yield e
    e.close()


# ---------------------------------------------------------------- the statistics
def launches(eng):
    st = eng.stats()
    d = {n: v["launches"] for n, v in st["kernels"].items()}
    d["retries"] = st["retries"]
    return d


def taken(eng, call, **want):
    """call() (a check of the form's own test file) ran these bitmap kernels this often, no other kernel, no retry."""
    d0 = launches(eng)
    out = call()
    d1 = launches(eng)
    d = {n: d1[n] - d0[n] for n in d1 if d1[n] != d0[n] and n != "copy_in"}
    assert d.pop("bmp_build", 0) >= 1, d
    assert d == want, (d, want)
    return out


def declined(eng, call):
    """call() (a run of the form's own test file: the oracle's answer) launched no bitmap kernel and counted no retry."""
    d0 = launches(eng)
    out = call()
    d1 = launches(eng)
    assert all(d1[n] == d0[n] for n in BMP_KERNELS) and d1["retries"] == d0["retries"], {n: d1[n] - d0[n] for n in d1}
    return out


# ---------------------------------------------------------------- planting
def pool(k, seed, blocks=0):
    """Distinct canonical codes in a seeded order; blocks: code i lies in block i % blocks of the code space."""
    rng, used, i = random.Random(seed), set(), 0
    span = 4 ** k // blocks if blocks else 4 ** k
    while True:
        c = (i % blocks) * span + rng.randrange(span) if blocks else rng.randrange(span)
        if c <= revcomp_code(c, k) and c not in used:
            used.add(c)
            i += 1
            yield c


def texts_of(codes_of_text, k):
    return ["N".join(kmer_text(c, k) for c in codes).encode() for codes in codes_of_text]


def genome_texts(plants, n, k):
    """plants: [(code, genomes, ...)]"""
    held = [[] for _ in range(n)]
    for code, genomes, *_ in plants:
        for i in sorted(genomes):
            held[i].append(code)
    return texts_of(held, k)


def layout(sizes):
    """group_of in group-major order and every group's first genome"""
    group_of = [g for g, n in enumerate(sizes) for _ in range(n)]
    first = [0] * len(sizes)
    for g in range(1, len(sizes)):
        first[g] = first[g - 1] + sizes[g - 1]
    return group_of, first


def within_plants(codes, sizes):
    """Per group one code present in exactly c of its genomes for every edge count c, the members rotated."""
    _, first = layout(sizes)
    return [(next(codes), frozenset(first[g] + (3 * j + i) % n for i in range(c)))
            for g, n in enumerate(sizes) for j, c in enumerate(edge_counts(n))]


def across_plants(codes, sizes):
    """One code present in exactly c groups (in the first genome of each) for every edge count c of the group count."""
    _, first = layout(sizes)
    ng = len(sizes)
    return [(next(codes), frozenset(first[(5 * j + i) % ng] for i in range(c))) for j, c in enumerate(edge_counts(ng))]


def shuffled(group_of, plants, seed):
    """The caller's genome order shuffled: group_of is interleaved."""
    order = list(range(len(group_of)))
    random.Random(seed).shuffle(order)
    new_of = {old: new for new, old in enumerate(order)}
    return [group_of[o] for o in order], [(c, frozenset(new_of[i] for i in gen)) for c, gen in plants]


def group_sizes(group_of):
    return tuple(group_of.count(g) for g in range(max(group_of) + 1))


# ================================================================ type 1
def bins1(sizes):
    """exp1_bmp: one bin per count 0 .. size of every group, one per count 0 .. ngroups of groups"""
    return sum(sizes) + 2 * len(sizes) + 1


def reps_max(nb):
    return max(1, min(64, 65536 // nb))


@functools.lru_cache(maxsize=None)
def exp1_case(k, sizes, within=True, across=False, blocks=0, fill=0):
    """seqs, group_of, plants = [(code, genomes)].  fill: further codes of one genome each."""
    codes = pool(k, 1000 + k + len(sizes), blocks)
    group_of, _ = layout(sizes)
    plants = (within_plants(codes, sizes) if within else []) + (across_plants(codes, sizes) if across else [])
    plants += [(next(codes), frozenset([(7 * i) % len(group_of)])) for i in range(fill)]
    group_of, plants = shuffled(group_of, plants, 7 + len(sizes))
    return genome_texts(plants, len(group_of), k), group_of, plants


@functools.lru_cache(maxsize=None)
def want1(k, sizes, cs, hist_len, **kw):
    seqs, group_of, _ = exp1_case(k, sizes, **kw)
    return CO.exp1(seqs, group_of, k, cs=cs, hist_len=hist_len)


def check1(eng, k, sizes, cs=5000, hist_len=5001, **kw):
    seqs, group_of, _ = exp1_case(k, sizes, **kw)
    want = want1(k, sizes, cs, hist_len, **kw)
    return taken(eng, lambda: B1.check(eng, seqs, group_of, k, cs=cs, hist_len=hist_len, want=want), bmp_readout=1)


def declined1(eng, k, sizes, **kw):
    seqs, group_of, _ = exp1_case(k, sizes, **kw)
    return declined(eng, lambda: B1.not_taken(eng, seqs, group_of, k, want1(k, sizes, 5000, 5001, **kw), False))


GENOME_SLICES = tuple(v for j in range(SLICES - 3, SLICES) for v in ((1 << j) - 1, 1 << j)) + (MAX_COUNT,)
HAND_OVER = {11: (MAX_COUNT, (MAX_COUNT + 1) // 2, 4, 8, 5, 3), 12: ((MAX_COUNT + 1) // 4, 3, 1)}
GROUP_SLICES = tuple(v for j in range(SLICES - 2, SLICES) for v in ((1 << j) - 1, 1 << j)) + (MAX_COUNT,)


def bins_edge_sizes(nseq):
    """MAX_COUNT groups of nseq genomes in all: one of MAX_COUNT genomes, one that takes the rest, all others of one."""
    rest = nseq - MAX_COUNT - (MAX_COUNT - 1)
    assert 0 <= rest < MAX_COUNT
    return (MAX_COUNT, 1 + rest) + (1,) * (MAX_COUNT - 2)


BINS1_NSEQ = MAX_BINS - 2 * MAX_COUNT - 1                      # bins1 == MAX_BINS with MAX_COUNT groups
# nbins + nseq of the read-out's replicas: 2 (nseq + ngroups) + 1, an odd number whatever the shape
REPLICA_SHAPES = ((300, 200, 4, 3), (300, 200, 5, 3), (1000, 400, 90, 6))
REPLICA_K, REPLICA_BLOCKS = 9, 64                               # 4^9 / 64 words in 64 blocks of 64: a grid of 64 workgroups


@pytest.mark.gpu
@pytest.mark.parametrize("cs,hist_len", SATURATIONS)
def test_exp1_genome_slices(eng, cs, hist_len):
    """Groups of 127 .. 1023 genomes in one call: counters c[] of 7 to 10 slices, every edge count of each."""
    check1(eng, 7, GENOME_SLICES, cs, hist_len)


@pytest.mark.gpu
@pytest.mark.parametrize("k", sorted(HAND_OVER))
def test_exp1_four_wave_hand_over(eng, k):
    """k = 11 and 12: four operands a round, two buffers in turn; group ends on a multiple of four operands and off it."""
    check1(eng, k, HAND_OVER[k])


@pytest.mark.gpu
@pytest.mark.parametrize("ngroups", GROUP_SLICES)
def test_exp1_group_slices(eng, ngroups):
    """The counter a[] over groups with 8 to 10 slices, every edge count of the group count."""
    for cs, hist_len in SATURATIONS:
        check1(eng, 7, (1,) * ngroups, cs, hist_len, within=False, across=True)


@pytest.mark.gpu
def test_exp1_group_slices_four_waves(eng):
    check1(eng, 11, (1,) * MAX_COUNT, within=False, across=True)


@pytest.mark.gpu
def test_exp1_limit_group_size(eng):
    check1(eng, 7, (MAX_COUNT,))
    declined1(eng, 7, (MAX_COUNT + 1,))


@pytest.mark.gpu
def test_exp1_limit_group_count(eng):
    check1(eng, 7, (1,) * MAX_COUNT, within=False, across=True)
    declined1(eng, 7, (1,) * (MAX_COUNT + 1), within=False, across=True)


@pytest.mark.gpu
def test_exp1_limit_bins(eng):
    """nseq + 2 ngroups + 1 == KH_BMP_MAX_BINS is taken, one genome more is declined."""
    check1(eng, 7, bins_edge_sizes(BINS1_NSEQ), across=True)
    declined1(eng, 7, bins_edge_sizes(BINS1_NSEQ + 1), across=True)


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", REPLICA_SHAPES, ids=lambda s: f"nb{bins1(s) + sum(s)}")
def test_exp1_replicas(eng, sizes):
    """The replicas of the bins by BmpRun::reps_max, max(1, min(64, 65536 // nb)) with nb = nbins + nseq, in a grid of 64
    workgroups (k = 9): nb = 1023 gives 64, nb = 1025 gives 63 and nb = 3001 gives 21, so blockIdx.x % reps runs with a
    modulus that is no power of two.  (nb = 2 (nseq + ngroups) + 1 is odd for every shape of type 1: 1024 itself
    cannot occur, 1023 is the nearest count that still gives 64.)  Planted codes lie in each of the 64 blocks."""
    check1(eng, REPLICA_K, sizes, across=True, blocks=REPLICA_BLOCKS, fill=2 * REPLICA_BLOCKS)


# ================================================================ type 2
def bins2(sizes, pivot_group):
    """exp2_bmp: per pivot one bin per count 0 .. size of its group and one per count of other groups, then one distinct
    counter per operand"""
    return sum(sizes[g] + 1 + len(sizes) for g in pivot_group) + sum(sizes) + len(pivot_group)


def case2(k, sizes, pivot_group, plants):
    """plants: [(code, genomes, pivots)] -> seqs, group_of, pivots, pivot_group, plants"""
    group_of, _ = layout(sizes)
    held = [[] for _ in pivot_group]
    for code, _, pivots in plants:
        for p in pivots:
            held[p].append(code)
    return genome_texts(plants, len(group_of), k), group_of, texts_of(held, k), list(pivot_group), plants


@functools.lru_cache(maxsize=None)
def exp2_big(k):
    """A group of MAX_COUNT genomes with two pivots and one of 2 with one: each pivot's codes lie in exactly v genomes of
    its own group, v = 0 and every edge count; every other one also in a genome of the other group.  One code per group
    lies in all its genomes and in no pivot."""
    sizes, pivot_group = (MAX_COUNT, 2), (0, 0, 1)
    _, first = layout(sizes)
    codes = pool(k, 2000 + k)
    plants = []
    for p, g in enumerate(pivot_group):
        n, h = sizes[g], 1 - g
        for j, v in enumerate([0] + edge_counts(n)):
            genomes = {first[g] + (3 * j + p + i) % n for i in range(v)}
            if j % 2:
                genomes.add(first[h] + j % sizes[h])
            plants.append((next(codes), frozenset(genomes), (p,)))
    plants += [(next(codes), frozenset(range(first[g], first[g] + n)), ()) for g, n in enumerate(sizes)]
    return case2(k, sizes, pivot_group, plants)


@functools.lru_cache(maxsize=None)
def exp2_groups(k=7):
    """MAX_COUNT groups of one genome, a pivot in group 1 and one in the last group: each pivot's codes lie in exactly v
    OTHER groups, v = 0 and every edge count up to all others, once with the pivot's own group holding the code and once
    without."""
    ng = MAX_COUNT
    sizes, pivot_group = (1,) * ng, (1, ng - 1)
    codes = pool(k, 2100 + k)
    plants = []
    for p, own in enumerate(pivot_group):
        others = [g for g in range(ng) if g != own]
        for j, v in enumerate([0] + edge_counts(ng - 1)):
            for with_own in (False, True):
                genomes = {others[(7 * j + p + i) % (ng - 1)] for i in range(v)} | ({own} if with_own else set())
                plants.append((next(codes), frozenset(genomes), (p,)))
    return case2(k, sizes, pivot_group, plants)


BINS2_SIZES = (1, 2)
BINS2_PIVOTS = {MAX_BINS: (815, 3), MAX_BINS + 1: (814, 4)}      # pivots held out of the two groups


@functools.lru_cache(maxsize=None)
def exp2_bins(nbins, k=7):
    """Groups of 1 and 2 genomes with 815 and 3 pivots (814 and 4), the pivots of the second group spread among those of
    the first in the caller's order.  The r-th pivot of a group holds a code that r % (size + 1) genomes of its group hold, and
    pivot q one that the other group holds when q is odd."""
    sizes = BINS2_SIZES
    n0, n1 = BINS2_PIVOTS[nbins]
    _, first = layout(sizes)
    at = {(i + 1) * (n0 + n1) // (n1 + 1) for i in range(n1)}
    pivot_group = tuple(1 if q in at else 0 for q in range(n0 + n1))
    codes = pool(k, 2200 + k)
    plants, rank = [], [0, 0]
    for q, g in enumerate(pivot_group):
        n, h = sizes[g], 1 - g
        plants.append((next(codes), frozenset(first[g] + (q + i) % n for i in range(rank[g] % (n + 1))), (q,)))
        rank[g] += 1
        plants.append((next(codes), frozenset([first[h] + q % sizes[h]] if q % 2 else []), (q,)))
    return case2(k, sizes, pivot_group, plants)


@functools.lru_cache(maxsize=None)
def want2(name, arg=None, hist_len=5001):
    """arg: the k of "big", the bins of "bins" (k = 7, as "groups")"""
    case = CASES2[name]() if arg is None else CASES2[name](arg)
    return X2.oracle(*case[:4], arg if name == "big" else 7, hist_len=hist_len)


CASES2 = {"big": exp2_big, "groups": exp2_groups, "bins": exp2_bins}


def check2(eng, case, k, want, hist_len=5001):
    return taken(eng, lambda: X2.check(eng, *case[:4], k, hist_len=hist_len, want=want), bmp_pivot=1)


@pytest.mark.gpu
@pytest.mark.parametrize("k", (7, 11))
def test_exp2_big_group(eng, k):
    got, _ = check2(eng, exp2_big(k), k, want2("big", k))
    assert (got["within_only"] == 1).all()                               # v = 0: the pivot alone holds it


@pytest.mark.gpu
def test_exp2_many_groups(eng):
    check2(eng, exp2_groups(), 7, want2("groups"))


@pytest.mark.gpu
def test_exp2_limit_bins(eng):
    """Sum of npiv_g (size_g + 1 + ngroups) + nseq + npiv == KH_BMP_MAX_BINS is taken; one more, and the set form answers."""
    check2(eng, exp2_bins(MAX_BINS), 7, want2("bins", MAX_BINS, hist_len=16), hist_len=16)
    case = exp2_bins(MAX_BINS + 1)
    declined(eng, lambda: X2.by_sets(eng, *case[:4], 7, hist_len=16, want=want2("bins", MAX_BINS + 1, hist_len=16)))


# ================================================================ type 3
def bins3(nseq, npiv):
    """exp3_bmp: a launch of one pivot has nseq bins and 1 + nseq distinct counters; without pivots only the counters"""
    return nseq + (nseq + 1 if npiv else 0)


def cross_launches(nseq, npiv):
    """exp3_bmp: a batch holds as many pivots as fit the bins and the LDS kept for their words"""
    assert bins3(nseq, npiv) <= MAX_BINS
    if not npiv:
        return 1
    batch = min((MAX_BINS - nseq) // (nseq + 1), CROSS_PIVOTS, npiv)
    return (npiv + batch - 1) // batch


def case3(k, sizes, npiv, plants):
    """plants: [(code, genomes, pivots)] -> seqs, group_of, pivots, plants"""
    group_of, _ = layout(sizes)
    held = [[] for _ in range(npiv)]
    for code, _, pivots in plants:
        for p in pivots:
            held[p].append(code)
    return genome_texts(plants, len(group_of), k), group_of, texts_of(held, k), plants


BIG3_SIZES, BIG3_PIVOTS = (MAX_COUNT, 3), 5


@functools.lru_cache(maxsize=None)
def exp3_big(k):
    """Groups of MAX_COUNT and 3 genomes, five pivots: every pivot has codes of its own in exactly v genomes of the big
    group, v = 0 and every edge count, and in 0 .. 3 genomes of the small one."""
    sizes = BIG3_SIZES
    _, first = layout(sizes)
    codes = pool(k, 3000 + k)
    plants = []
    for p in range(BIG3_PIVOTS):
        for j, v in enumerate([0] + edge_counts(sizes[0])):
            genomes = {first[0] + (3 * j + p + i) % sizes[0] for i in range(v)}
            genomes |= {first[1] + (j + i) % sizes[1] for i in range((j + p) % (sizes[1] + 1))}
            plants.append((next(codes), frozenset(genomes), (p,)))
    return case3(k, sizes, BIG3_PIVOTS, plants)


CAP3_K, CAP3_SIZES = 9, (3, 3, 3)
CAP3_PIVOTS = (CROSS_PIVOTS, CROSS_PIVOTS + 1, 2 * CROSS_PIVOTS + 1)


@functools.lru_cache(maxsize=None)
def exp3_cap(npiv):
    """9 genomes in 3 groups.  Pivot q has two codes of its own: one held by (q, q / 4, q / 16) % 4 genomes of the three
    groups, one by q % 3 + 1 genomes of group q % 3 — a pivot word at another row of LDS is another answer."""
    sizes = CAP3_SIZES
    _, first = layout(sizes)
    codes = pool(CAP3_K, 3100)
    plants = []
    for q in range(npiv):
        vec = (q % 4, q // 4 % 4, q // 16 % 4)
        plants.append((next(codes), frozenset(first[g] + (q + i) % 3 for g in range(3) for i in range(vec[g])), (q,)))
        plants.append((next(codes), frozenset(first[q % 3] + (q // 3 + i) % 3 for i in range(q % 3 + 1)), (q,)))
    return case3(CAP3_K, sizes, npiv, plants)


def full_groups(nseq):
    """nseq genomes in groups of MAX_COUNT and one that takes the rest"""
    return (MAX_COUNT,) * (nseq // MAX_COUNT) + ((nseq % MAX_COUNT,) if nseq % MAX_COUNT else ())


BINS3 = {"pivot": ((MAX_BINS - 1) // 2, 1), "no_pivot": (MAX_BINS, 0)}   # (nseq, npiv) of the fitting shape


@functools.lru_cache(maxsize=None)
def exp3_bins(nseq, npiv, k=7):
    """Every edge count of every group; the pivot (if any) holds every other code and one of its own."""
    sizes = full_groups(nseq)
    codes = pool(k, 3200 + nseq)
    plants = [(c, gen, (0,) if npiv and j % 2 else ()) for j, (c, gen) in enumerate(within_plants(codes, sizes))]
    if npiv:
        plants.append((next(codes), frozenset(), (0,)))
    return case3(k, sizes, npiv, plants)


@functools.lru_cache(maxsize=None)
def want3(name, *args):
    case = CASES3[name](*args)
    return X3.oracle(*case[:3], {"big": args[0], "cap": CAP3_K, "bins": 7}[name])


CASES3 = {"big": exp3_big, "cap": exp3_cap, "bins": exp3_bins}


def check3(eng, case, k, want, batches):
    return taken(eng, lambda: X3.check(eng, *case[:3], k, want=want, batches=batches), bmp_cross=batches)


@pytest.mark.gpu
@pytest.mark.parametrize("k", (7, 11))
def test_exp3_big_group(eng, k):
    """Five pivots, two to a launch by the bins: three launches, the last with one pivot."""
    case = exp3_big(k)
    check3(eng, case, k, want3("big", k), cross_launches(len(case[0]), BIG3_PIVOTS))


@pytest.mark.gpu
@pytest.mark.parametrize("npiv", CAP3_PIVOTS)
def test_exp3_pivot_cap(eng, npiv):
    """KH_BMP_CROSS_PIVOTS pivots: one launch with every row of pw in use; one more: two launches; twice and one: three."""
    check3(eng, exp3_cap(npiv), CAP3_K, want3("cap", npiv), cross_launches(sum(CAP3_SIZES), npiv))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(BINS3))
def test_exp3_limit_bins(eng, name):
    """2 nseq + 1 bins with a pivot, nseq without: KH_BMP_MAX_BINS (or the last count below it) is taken, one genome more is
    declined."""
    nseq, npiv = BINS3[name]
    check3(eng, exp3_bins(nseq, npiv), 7, want3("bins", nseq, npiv), 1)
    case = exp3_bins(nseq + 1, npiv)
    if npiv:
        declined(eng, lambda: X3.by_sets(eng, *case[:3], 7, want=want3("bins", nseq + 1, npiv)))
    else:                                                                # nothing to intersect: the set form only builds
        _, d = declined(eng, lambda: X3.run(eng, *case[:3], 7, want=want3("bins", nseq + 1, npiv)))
        assert d["builds"] == nseq + 1, d


# ================================================================ type 4
def bins4(sizes, npiv):
    """exp4_bmp: one bin per count 0 .. size of every group, then one distinct counter per operand"""
    return 2 * sum(sizes) + len(sizes) + npiv


def case4(k, sizes, npiv, plants, seed):
    """plants: [(code, genomes, {pivot: multiplicity})] -> seqs, group_of, pivots, plants; a pivot's occurrences shuffled"""
    group_of, _ = layout(sizes)
    held = [[] for _ in range(npiv)]
    for code, _, mults in plants:
        for p, m in mults.items():
            held[p] += [code] * m
    rng = random.Random(seed)
    for h in held:
        rng.shuffle(h)
    return genome_texts(plants, len(group_of), k), group_of, texts_of(held, k), plants


BIG4_SIZES, BIG4_MULTS = (MAX_COUNT, (MAX_COUNT + 1) // 2, (MAX_COUNT + 1) // 4, 3), (1, 2, 255, 256)


@functools.lru_cache(maxsize=None)
def exp4_big(k):
    """Groups of 1023, 512, 256 and 3 genomes, two pivots.  Every edge count of every group (two in three of those codes
    also in a pivot); and per pivot and multiplicity a code that 0 .. 4 of the groups hold, in one genome each."""
    sizes = BIG4_SIZES
    _, first = layout(sizes)
    ng = len(sizes)
    codes = pool(k, 4000 + k)
    plants = [(c, gen, {j % 3: 1 + j % 2} if j % 3 < 2 else {}) for j, (c, gen) in enumerate(within_plants(codes, sizes))]
    i = 0
    for p in range(2):
        for mult in BIG4_MULTS:
            for size in range(ng + 1):
                genomes = frozenset(first[g] + i % sizes[g] for g in ((i + j) % ng for j in range(size)))
                plants.append((next(codes), genomes, {p: mult}))
                i += 1
    return case4(k, sizes, 2, plants, 40 + k)


BINS4_GROUPS = 2


@functools.lru_cache(maxsize=None)
def exp4_bins(npiv, k=7):
    """Two groups, 2 nseq + ngroups + 2 == KH_BMP_MAX_BINS; npiv = 2 fits, a third pivot is one bin too many."""
    nseq = (MAX_BINS - BINS4_GROUPS - 2) // 2
    sizes = (MAX_COUNT, nseq - MAX_COUNT)
    codes = pool(k, 4100 + k)
    plants = [(c, gen, {j % npiv: 1 + j % 2}) for j, (c, gen) in enumerate(within_plants(codes, sizes))]
    return case4(k, sizes, npiv, plants, 41)


@functools.lru_cache(maxsize=None)
def want4(name, arg):
    case = CASES4[name](arg)
    return X4.oracle(*case[:3], arg if name == "big" else 7)


CASES4 = {"big": exp4_big, "bins": exp4_bins}


def check4(eng, case, k, want):
    return taken(eng, lambda: X4.check(eng, *case[:3], k, want=want), bmp_count=1, bmp_present=1, bmp_member=1)


@pytest.mark.gpu
@pytest.mark.parametrize("k", (7, 11))
def test_exp4_big_groups(eng, k):
    check4(eng, exp4_big(k), k, want4("big", k))


@pytest.mark.gpu
def test_exp4_limit_bins(eng):
    """2 nseq + ngroups + npiv == KH_BMP_MAX_BINS is taken; one pivot more, and the set form answers."""
    check4(eng, exp4_bins(2), 7, want4("bins", 2))
    case = exp4_bins(3)
    declined(eng, lambda: X4.by_sets(eng, *case[:3], 7, want=want4("bins", 3)))


# ================================================================ preconditions, without a GPU
def test_constants_match_sources():
    assert 2 ** SLICES - 1 == MAX_COUNT
    assert edge_counts(MAX_COUNT)[-3:] == [2 ** (SLICES - 1) - 1, 2 ** (SLICES - 1), MAX_COUNT]   # up to the last slice
    assert MAX_BINS > 2 * MAX_COUNT + 1 and CROSS_PIVOTS >= 1 and MEMBER_GROUPS >= len(BIG4_SIZES)
    engine = _src("kh_engine.cpp")
    assert "static u32 reps_max(u32 nb) { return std::max<u32>(1, std::min<u32>(64, 65536u / nb)); }" in engine
    assert "(max_bins - (u64)nseq) / ((u64)nseq + 1), KH_BMP_CROSS_PIVOTS), (u64)npiv)" in engine


def holds_exactly(k, texts, plants, member):
    """Every planted code is canonical and distinct; text i holds exactly the codes whose plant names i."""
    codes = [pl[0] for pl in plants]
    assert len(set(codes)) == len(codes) and all(c <= revcomp_code(c, k) for c in codes)
    want = [set() for _ in texts]
    for pl in plants:
        for i in member(pl):
            want[i].add(pl[0])
    for text, w in zip(texts, want):
        assert canonical_codes(text, k) == w


def every_edge_count(sizes, group_of, plants):
    """Per group, among the codes that lie in that group alone: every edge count 2^j - 1 and 2^j up to the size."""
    counts = [set() for _ in sizes]
    for _, genomes, *_ in plants:
        groups = {group_of[i] for i in genomes}
        if len(groups) == 1:
            counts[groups.pop()].add(len(genomes))
    for n, have in zip(sizes, counts):
        assert have >= set(edge_counts(n)), (n, sorted(set(edge_counts(n)) - have))


def every_group_count(group_of, plants):
    ng = max(group_of) + 1
    have = {len({group_of[i] for i in genomes}) for _, genomes, *_ in plants}
    assert have >= set(edge_counts(ng)), sorted(set(edge_counts(ng)) - have)


EXP1_CASES = ([(7, GENOME_SLICES, {}, SATURATIONS)] + [(k, s, {}, SATURATIONS[:1]) for k, s in sorted(HAND_OVER.items())]
              + [(7, (1,) * n, dict(within=False, across=True), SATURATIONS) for n in GROUP_SLICES + (MAX_COUNT + 1,)]
              + [(11, (1,) * MAX_COUNT, dict(within=False, across=True), SATURATIONS[:1])]
              + [(7, (MAX_COUNT,), {}, SATURATIONS[:1]), (7, (MAX_COUNT + 1,), {}, SATURATIONS[:1])]
              + [(7, bins_edge_sizes(BINS1_NSEQ + d), dict(across=True), SATURATIONS[:1]) for d in (0, 1)]
              + [(REPLICA_K, s, dict(across=True, blocks=REPLICA_BLOCKS, fill=2 * REPLICA_BLOCKS), SATURATIONS[:1])
                 for s in REPLICA_SHAPES])


@pytest.mark.parametrize("k,sizes,kw,saturations", EXP1_CASES,
                         ids=[f"k{k}_{len(s)}groups_{sum(s)}genomes" for k, s, _, _ in EXP1_CASES])
def test_exp1_cases_hold_every_count(k, sizes, kw, saturations):
    seqs, group_of, plants = exp1_case(k, sizes, **kw)
    assert group_sizes(group_of) == sizes and (len(sizes) == 1 or group_of != sorted(group_of))   # interleaved
    holds_exactly(k, seqs, plants, lambda pl: pl[1])
    if kw.get("within", True):
        every_edge_count(sizes, group_of, plants)
    if kw.get("across"):
        every_group_count(group_of, plants)
    for cs, hist_len in saturations:                                      # two independent references agree
        want, mine = want1(k, sizes, cs, hist_len, **kw), planted_histograms(group_of, plants, cs, hist_len)
        for f in FIELDS1:
            assert want[f].shape == mine[f].shape and (want[f] == mine[f]).all(), (f, cs, hist_len)


def test_exp1_shapes_are_what_they_claim():
    assert GENOME_SLICES == (127, 128, 255, 256, 511, 512, 1023) and sum(GENOME_SLICES) == 2812 and bins1(GENOME_SLICES) == 2827
    assert HAND_OVER == {11: (1023, 512, 4, 8, 5, 3), 12: (256, 3, 1)} and GROUP_SLICES == (255, 256, 511, 512, 1023)
    ends = [sum(HAND_OVER[11][:i + 1]) % 4 for i in range(6)]             # four operands a round: ends on and off a round
    assert 0 in ends and set(ends) - {0} and [sum(HAND_OVER[12][:i + 1]) % 4 for i in range(3)] == [0, 3, 0]
    assert SATURATIONS[3:5] == ((1023, 1024), (1022, 1023))
    assert all(cs <= MAX_COUNT or hl - 1 <= MAX_COUNT for cs, hl in SATURATIONS[1:])   # cs or the last bin inside the counts
    fit, over = bins_edge_sizes(BINS1_NSEQ), bins_edge_sizes(BINS1_NSEQ + 1)
    assert (BINS1_NSEQ, len(fit), bins1(fit), bins1(over)) == (2049, MAX_COUNT, MAX_BINS, MAX_BINS + 1)
    assert max(fit) == max(over) == MAX_COUNT and sum(over) == sum(fit) + 1
    assert bins1((MAX_COUNT + 1,)) <= MAX_BINS and bins1((1,) * (MAX_COUNT + 1)) <= MAX_BINS   # declined for the count alone
    nb = [bins1(s) + sum(s) for s in REPLICA_SHAPES]
    assert nb == [1023, 1025, 3001] and [reps_max(n) for n in nb] == [64, 63, 21] and reps_max(1024) == 64
    assert 4 ** REPLICA_K // 64 // 64 == REPLICA_BLOCKS                   # words / 64: the read-out's grid
    span = 4 ** REPLICA_K // REPLICA_BLOCKS
    for s in REPLICA_SHAPES:
        _, _, plants = exp1_case(REPLICA_K, s, across=True, blocks=REPLICA_BLOCKS, fill=2 * REPLICA_BLOCKS)
        assert {c // span for c, _ in plants} == set(range(REPLICA_BLOCKS))


def pivot_codes(plants, p):
    return [pl for pl in plants if p in pl[2]]


@pytest.mark.parametrize("k", (7, 11))
def test_exp2_big_case(k):
    seqs, group_of, pivots, pivot_group, plants = exp2_big(k)
    assert group_sizes(group_of) == (MAX_COUNT, 2) and pivot_group == [0, 0, 1]
    assert bins2(group_sizes(group_of), pivot_group) <= MAX_BINS
    holds_exactly(k, seqs, plants, lambda pl: pl[1])
    holds_exactly(k, pivots, plants, lambda pl: pl[2])
    want = want2("big", k)
    for p, g in enumerate(pivot_group):
        n = group_sizes(group_of)[g]
        mine = [sum(group_of[i] == g for i in gen) for _, gen, _ in pivot_codes(plants, p)]
        assert sorted(mine) == [0] + edge_counts(n)
        assert want["within_only"][p] == 1 and all(want["within_hist"][p, v + 1] == 1 for v in edge_counts(n))
        assert want["across_only"][p] > 0 and want["across_hist"][p, 2] > 0


def test_exp2_groups_case():
    k = 7
    seqs, group_of, pivots, pivot_group, plants = exp2_groups()
    ng = MAX_COUNT
    assert group_sizes(group_of) == (1,) * ng and pivot_group == [1, ng - 1]
    assert bins2(group_sizes(group_of), pivot_group) <= MAX_BINS
    holds_exactly(k, seqs, plants, lambda pl: pl[1])
    holds_exactly(k, pivots, plants, lambda pl: pl[2])
    want = want2("groups")
    for p, own in enumerate(pivot_group):
        mine = sorted((len(gen - {own}), own in gen) for _, gen, _ in pivot_codes(plants, p))
        assert mine == sorted((v, w) for v in [0] + edge_counts(ng - 1) for w in (False, True))
        assert edge_counts(ng - 1)[-1] == ng - 1 and {2 ** j for j in range(SLICES)} <= set(edge_counts(ng - 1))
        assert want["across_only"][p] == 2 and all(want["across_hist"][p, v + 1] == 2 for v in edge_counts(ng - 1))
        assert want["within_only"][p] == want["within_hist"][p, 2] == len(mine) // 2


@pytest.mark.parametrize("nbins", sorted(BINS2_PIVOTS))
def test_exp2_bins_case(nbins):
    k = 7
    seqs, group_of, pivots, pivot_group, plants = exp2_bins(nbins)
    assert group_sizes(group_of) == BINS2_SIZES
    assert (pivot_group.count(0), pivot_group.count(1)) == BINS2_PIVOTS[nbins]
    assert bins2(BINS2_SIZES, pivot_group) == nbins and nbins in (4096, 4097)
    assert 0 < pivot_group.index(1) and pivot_group[-1] == 0                # the second group's pivots among the first's
    holds_exactly(k, seqs, plants, lambda pl: pl[1])
    holds_exactly(k, pivots, plants, lambda pl: pl[2])
    want = want2("bins", nbins, hist_len=16)
    assert want["within_hist"][:, 2:4].sum(axis=0).all() and want["across_hist"][:, 2].sum() > 0   # counts 1 and 2 within


@pytest.mark.parametrize("k", (7, 11))
def test_exp3_big_case(k):
    seqs, group_of, pivots, plants = exp3_big(k)
    assert group_sizes(group_of) == BIG3_SIZES and len(pivots) == BIG3_PIVOTS
    assert bins3(len(seqs), 1) <= MAX_BINS and cross_launches(len(seqs), BIG3_PIVOTS) == 3   # two pivots a launch
    holds_exactly(k, seqs, plants, lambda pl: pl[1])
    holds_exactly(k, pivots, plants, lambda pl: pl[2])
    want = want3("big", k)
    for p in range(BIG3_PIVOTS):
        mine = sorted(sum(group_of[i] == 0 for i in gen) for _, gen, _ in pivot_codes(plants, p))
        assert mine == [0] + edge_counts(MAX_COUNT)
        assert all(want["inter_hist"][p, 0, v + 1] == 1 for v in edge_counts(MAX_COUNT))
        assert {sum(group_of[i] == 1 for i in gen) for _, gen, _ in pivot_codes(plants, p)} == {0, 1, 2, 3}


@pytest.mark.parametrize("npiv", CAP3_PIVOTS)
def test_exp3_cap_case(npiv):
    seqs, group_of, pivots, plants = exp3_cap(npiv)
    assert group_sizes(group_of) == CAP3_SIZES and len(pivots) == npiv and CAP3_PIVOTS == (64, 65, 129)
    assert cross_launches(len(seqs), npiv) == {64: 1, 65: 2, 129: 3}[npiv]
    holds_exactly(CAP3_K, seqs, plants, lambda pl: pl[1])
    holds_exactly(CAP3_K, pivots, plants, lambda pl: pl[2])
    assert all(len(pivot_codes(plants, q)) == 2 for q in range(npiv))       # codes of its own
    rows = want3("cap", npiv)["inter_hist"]
    first = [r.tobytes() for r in rows[:CROSS_PIVOTS]]
    assert len(set(first)) == CROSS_PIVOTS                                  # no two pivots of a launch share an answer


@pytest.mark.parametrize("name", sorted(BINS3))
def test_exp3_bins_case(name):
    k = 7
    nseq, npiv = BINS3[name]
    assert (nseq, npiv) == {"pivot": (2047, 1), "no_pivot": (4096, 0)}[name]
    assert bins3(nseq, npiv) == {"pivot": MAX_BINS - 1, "no_pivot": MAX_BINS}[name] and bins3(nseq + 1, npiv) == MAX_BINS + 1
    for n in (nseq, nseq + 1):
        seqs, group_of, pivots, plants = exp3_bins(n, npiv)
        assert group_sizes(group_of) == full_groups(n) and sum(full_groups(n)) == n and max(full_groups(n)) == MAX_COUNT
        assert len(pivots) == npiv and (n > nseq or cross_launches(n, npiv) == 1)
        holds_exactly(k, seqs, plants, lambda pl: pl[1])
        holds_exactly(k, pivots, plants, lambda pl: pl[2])
        every_edge_count(full_groups(n), group_of, plants)


@pytest.mark.parametrize("k", (7, 11))
def test_exp4_big_case(k):
    seqs, group_of, pivots, plants = exp4_big(k)
    assert group_sizes(group_of) == BIG4_SIZES == (1023, 512, 256, 3) and len(pivots) == 2
    assert bins4(BIG4_SIZES, 2) <= MAX_BINS and len(BIG4_SIZES) <= MEMBER_GROUPS
    holds_exactly(k, seqs, plants, lambda pl: pl[1])
    holds_exactly(k, pivots, plants, lambda pl: pl[2])
    every_edge_count(BIG4_SIZES, group_of, plants)
    for p in range(2):
        raw = X4.counted(pivots[p], k, 1 << 30)
        assert raw == {c: m[p] for c, _, m in plants if p in m}              # exactly the planted multiplicities
        assert {(m[p], len({group_of[i] for i in gen})) for _, gen, m in plants if p in m} \
            >= {(mult, size) for mult in BIG4_MULTS for size in range(len(BIG4_SIZES) + 1)}
    want = want4("big", k)
    assert (want["rows"] > 0).all() and (want["unique"] > 0).all()
    for g, n in enumerate(BIG4_SIZES):
        assert all(want["within_hist"][g, c] > 0 for c in edge_counts(n))


def test_exp4_bins_case():
    k = 7
    for npiv, nbins in ((2, MAX_BINS), (3, MAX_BINS + 1)):
        seqs, group_of, pivots, plants = exp4_bins(npiv)
        sizes = group_sizes(group_of)
        assert len(sizes) == BINS4_GROUPS and max(sizes) == MAX_COUNT and len(pivots) == npiv
        assert bins4(sizes, npiv) == nbins and nbins in (4096, 4097)
        holds_exactly(k, seqs, plants, lambda pl: pl[1])
        holds_exactly(k, pivots, plants, lambda pl: pl[2])
        every_edge_count(sizes, group_of, plants)
        assert (want4("bins", npiv)["rows"] > 0).any(axis=1).all()
