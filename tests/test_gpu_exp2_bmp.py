"""kh_exp2_run (fused experiment type 2) against oracle/kmer_oracle.py: for every pivot the `intersect -ocsum`
histograms and `kmers_subtract` counts against its own group and against the other groups, and the distinct counts,
bit-exact; and from the statistics which form did the work: k_bmp_build + k_bmp_pivot (kh_bmp.hip) for k <= 12, the
set operations inside the library otherwise.

The planted inputs (word, wave, range and bitmap edges; every count of every pivot) are proven on the CPU by the
unmarked tests at the end: every planted code is canonical, lies where the case says it lies and occurs in exactly the
texts it was meant for, and every bin of the expected answer is non-zero."""
import functools
import os
import random
import shutil

import numpy as np
import pytest

from khoice_amd import synth
from oracle import kmer_oracle as O
from tests.util import revcomp_np

TILE, SPLIT = 64, 192            # KHOICE_BMP_TILE_POS / KHOICE_BMP_SPLIT_POS of the planted cases: several tiles and splits per text
PLANT_K = (5, 8, 11, 12)
RANGE_BITS = 20                  # codes of a build range: k = 11 has 4 ranges, k = 12 has 16
FIELDS = ("within_hist", "across_hist", "within_only", "across_only", "distinct_per_seq", "distinct_per_pivot")
KERNELS = ("bmp_build", "bmp_pivot", "bmp_readout", "union_tagged", "skm_union", "setop")


@pytest.fixture(scope="module")
def eng():
    from khoice_amd import build as kbuild
    from khoice_amd import engine as E
    kbuild.build_library()
    e = E.Engine(0)
    yield e
    e.close()


# ---------------------------------------------------------------- the oracle's answer
@functools.lru_cache(maxsize=None)
def plain_set(text, k):
    """`kmc -ci1` + `set_counts 1` of a cleaned text (records separated by a line feed)."""
    fasta = b"".join(b">r\n" + rec + b"\n" for rec in text.split(b"\n"))
    return O.set_counts(O.build(fasta, k), 1)


def oracle(seqs, group_of, pivots, pivot_group, k, cs=5000, hist_len=5001):
    ng, cmax = max(group_of) + 1, hist_len - 1
    sets = [plain_set(bytes(t), k) for t in seqs]
    psets = [plain_set(bytes(t), k) for t in pivots]
    unions = [O.union_sum([s for s, g in zip(sets, group_of) if g == h], cs) for h in range(ng)]
    group_sets = [O.set_counts(u, 1) for u in unions]
    others = {g: O.union_sum([group_sets[h] for h in range(ng) if h != g], cs) for g in set(pivot_group)}
    want = {"within_hist": np.zeros((len(pivots), hist_len), dtype=np.uint64),
            "across_hist": np.zeros((len(pivots), hist_len), dtype=np.uint64),
            "within_only": np.zeros(len(pivots), dtype=np.uint64), "across_only": np.zeros(len(pivots), dtype=np.uint64),
            "distinct_per_seq": np.array([len(s) for s in sets], dtype=np.uint64),
            "distinct_per_pivot": np.array([len(s) for s in psets], dtype=np.uint64)}
    for p, g in enumerate(pivot_group):
        for scope, other in (("within", unions[g]), ("across", others[g])):
            hist = O.histogram(O.intersect(psets[p], other, "sum", cs), cmax)
            assert hist[0] == 0
            want[scope + "_hist"][p] = hist
            want[scope + "_only"][p] = O.histogram(O.kmers_subtract(psets[p], other), cmax)[1]
    return want


def deltas(st0, st1):
    d = {n: st1["kernels"][n]["launches"] - st0["kernels"][n]["launches"] for n in KERNELS}
    for n in ("retries", "builds", "bases", "kmers", "distinct", "setops", "setop_in", "setop_out"):
        d[n] = st1[n] - st0[n]
    return d


def run(eng, seqs, group_of, pivots, pivot_group, k, cs=5000, hist_len=5001, want=None):
    eng.profile(True)
    st0 = eng.stats()
    got = eng.exp2_run(seqs, group_of, pivots, pivot_group, k, cs=cs, hist_len=hist_len)
    st1 = eng.stats()
    eng.profile(False)
    if want is None:
        want = oracle(seqs, group_of, pivots, pivot_group, k, cs, hist_len)
    for f in FIELDS:
        assert got[f].shape == want[f].shape, (f, k, cs, hist_len)
        assert (got[f] == want[f]).all(), (f, k, cs, hist_len, np.argwhere(got[f] != want[f])[:8].tolist())
    return got, deltas(st0, st1)


def check(eng, seqs, group_of, pivots, pivot_group, k, cs=5000, hist_len=5001, want=None):
    """The oracle's answers, and the bitmap form alone did the work."""
    got, d = run(eng, seqs, group_of, pivots, pivot_group, k, cs, hist_len, want)
    assert d["bmp_build"] >= 1 and d["bmp_pivot"] == 1 and d["bmp_readout"] == 0, d
    assert d["union_tagged"] == 0 and d["skm_union"] == 0 and d["setop"] == 0 and d["retries"] == 0, d
    assert d["builds"] == len(seqs) + len(pivots), d
    return got, d


def same(a, b):
    return all(a[f].shape == b[f].shape and (a[f] == b[f]).all() for f in FIELDS)


@functools.lru_cache(maxsize=None)
def species(n=20_000):
    """3 groups x 3 genomes, and per group a fourth genome of the same ancestor as its pivot."""
    items = synth.species_set(3, 3, n)
    pivots = [synth.clean_text(synth.genome_records(s, 3, n, synth.ancestor(s, n))) for s in (1, 2, 3)]
    return [t for _, _, t in items], [s - 1 for s, _, _ in items], pivots, [0, 1, 2]


# ---------------------------------------------------------------- 1. every k
@pytest.mark.gpu
@pytest.mark.parametrize("k", range(1, 13))
def test_exp2_every_k(eng, k):
    seqs, group_of, pivots, pivot_group = species()
    want = oracle(seqs, group_of, pivots, pivot_group, k)
    got1, d1 = check(eng, seqs, group_of, pivots, pivot_group, k, want=want)
    got2, d2 = check(eng, seqs, group_of, pivots, pivot_group, k, want=want)
    assert same(got1, got2) and d1 == d2, (d1, d2)
    assert d1["bases"] == sum(len(s) for s in seqs + pivots)
    assert d1["distinct"] == int(want["distinct_per_seq"].sum() + want["distinct_per_pivot"].sum())


# ---------------------------------------------------------------- 2. planted codes at every edge
PLANT_SIZES = (3, 1, 2)          # genomes per group; one pivot per group
PLANT_ROUNDS = 12                # codes per category at least: texts of several splits


def kmer_text(code, k):
    return "".join("ACGT"[(code >> (2 * (k - 1 - i))) & 3] for i in range(k))


def revcomp_code(code, k):
    r = 0
    for _ in range(k):
        r = (r << 2) | (3 - (code & 3))
        code >>= 2
    return r


def is_canonical(code, k):
    return code <= revcomp_code(code, k)


def first_canonical(codes, k):
    """The first canonical code of a range (numpy; the CPU tests below check the result in plain Python), or None."""
    a = np.array(codes, dtype=np.uint64).reshape(-1, 1)
    hit = np.flatnonzero(a[:, 0] <= revcomp_np(k, a)[:, 0])
    return int(a[hit[0], 0]) if hit.size else None


@functools.lru_cache(maxsize=None)
def edge_codes(k):
    """{what: canonical code} at the edges of the read-out's walk and of the build's ranges.  Where the very first or
    last code of a region is no canonical code (it never occurs in a bitmap) the nearest canonical one inside stands
    in; test_planted_codes_lie_on_the_edges proves that nothing canonical lies beyond it."""
    ncodes = 4 ** k
    nwords = max(1, ncodes // 64)
    rbits = min(RANGE_BITS, 2 * k)
    out = {}
    for r in range(ncodes >> rbits):
        lo, hi = r << rbits, (r + 1) << rbits
        out[f"range{r}_first"] = first_canonical(range(lo, hi), k)
        out[f"range{r}_last"] = first_canonical(range(hi - 1, lo - 1, -1), k)
    out["bit0"] = first_canonical(range(64, ncodes, 64), k)                # bit 0 of a word (code 0 is range0_first)
    out["bit63"] = first_canonical(range(63, ncodes, 64), k)               # bit 63 of a word
    if nwords > 64:                                                        # last word of a wave's 64, first of the next 64
        out["wave_last_word"] = first_canonical(range(63 * 64, 64 * 64), k)
        out["wave_first_word"] = first_canonical(range(64 * 64, 65 * 64), k)
        last_wave = (out[f"range{(ncodes >> rbits) - 1}_last"] // 64) // 64   # the last 64 words that hold anything
        out["last_wave_first_word"] = first_canonical(range(last_wave * 64 * 64, (last_wave * 64 + 1) * 64), k)
    by_code = {}
    for what, c in out.items():
        if c is not None:                                                  # (k = 5: no canonical code at bit 63 of any word)
            by_code.setdefault(c, what)                                    # a code on two edges at once: named once
    return {what: c for c, what in by_code.items()}


@functools.lru_cache(maxsize=None)
def planted_case(k):
    """Texts made of chosen canonical codes, every code a record of its own.  Per pivot p of group g (size n) the
    categories: ("within", v) pivot + exactly v genomes of g, v = 1..n; ("across", v) pivot + one genome in each of
    v other groups, v = 0..ngroups-1 (v = 0: the pivot alone); ("group",) a genome of g but not the pivot; ("rc",) the
    pivot holds the k-mer, a genome of g its reverse complement.  The edge codes go to the categories in turn, the
    rest is filled from a seeded pool: every category of every pivot holds PLANT_ROUNDS codes or more.
    Returns seqs, group_of, pivots, pivot_group, plants = [(code, category, pivot, genomes, what)]."""
    ng = len(PLANT_SIZES)
    group_of = [g for g, n in enumerate(PLANT_SIZES) for _ in range(n)]
    first = [group_of.index(g) for g in range(ng)]
    cats = []
    for p, n in enumerate(PLANT_SIZES):
        cats += [(("within", v), p) for v in range(1, n + 1)] + [(("across", v), p) for v in range(ng)]
        cats += [(("group",), p), (("rc",), p)]
    edges = edge_codes(k)
    rng = random.Random(900 + k)
    used = set(edges.values())
    assert len(used) == len(edges)

    def fresh():
        while True:
            c = rng.randrange(4 ** k)
            if is_canonical(c, k) and c != revcomp_code(c, k) and c not in used:
                used.add(c)
                return c

    rng.shuffle(cats)
    todo = [(what, c) for what, c in sorted(edges.items())]
    plants = []
    i = 0
    while todo or i < PLANT_ROUNDS * len(cats):
        (cat, p) = cats[i % len(cats)]
        i += 1
        what, code = todo.pop() if todo else ("fill", fresh())
        if cat[0] == "rc" and code == revcomp_code(code, k):                 # its own reverse complement: no second spelling
            todo.append((what, code))
            what, code = "fill", fresh()
        n = PLANT_SIZES[p]
        if cat[0] == "within":
            genomes = [first[p] + (i + j) % n for j in range(cat[1])]
        elif cat[0] == "across":
            genomes = [first[(p + 1 + j) % ng] + i % PLANT_SIZES[(p + 1 + j) % ng] for j in range(cat[1])]
        else:
            genomes = [first[p] + i % n]
        plants.append((code, cat, p, tuple(sorted(genomes)), what))
    texts = [[] for _ in group_of]
    ptexts = [[] for _ in PLANT_SIZES]
    for code, cat, p, genomes, _ in plants:
        if cat[0] != "group":
            ptexts[p].append(kmer_text(code, k))
        for gi in genomes:
            texts[gi].append(kmer_text(revcomp_code(code, k) if cat[0] == "rc" else code, k))
    join = lambda t: "N".join(t).encode()
    return [join(t) for t in texts], group_of, [join(t) for t in ptexts], list(range(ng)), plants


def planted_answer(k, cs=5000, hist_len=5001):
    """The expected outputs worked out from the plants alone."""
    seqs, group_of, pivots, pivot_group, plants = planted_case(k)
    ng = len(PLANT_SIZES)
    occ_w = [[0] * (n + 1) for n in PLANT_SIZES]
    occ_a = [[0] * ng for _ in PLANT_SIZES]
    dseq, dpiv = [0] * len(seqs), [0] * len(pivots)
    for code, cat, p, genomes, _ in plants:
        for gi in genomes:
            dseq[gi] += 1
        if cat[0] == "group":
            continue
        dpiv[p] += 1
        occ_w[p][sum(group_of[gi] == p for gi in genomes)] += 1
        occ_a[p][len({group_of[gi] for gi in genomes} - {p})] += 1
    want = {"within_hist": np.zeros((ng, hist_len), dtype=np.uint64), "across_hist": np.zeros((ng, hist_len), dtype=np.uint64),
            "within_only": np.array([o[0] for o in occ_w], dtype=np.uint64),
            "across_only": np.array([o[0] for o in occ_a], dtype=np.uint64),
            "distinct_per_seq": np.array(dseq, dtype=np.uint64), "distinct_per_pivot": np.array(dpiv, dtype=np.uint64)}
    for p in range(ng):
        for occ, f in ((occ_w[p], "within_hist"), (occ_a[p], "across_hist")):
            for v in range(1, len(occ)):
                want[f][p, min(1 + min(v, cs), cs, hist_len - 1)] += occ[v]
    return want, occ_w, occ_a


@pytest.fixture
def small_tiles(monkeypatch):
    monkeypatch.setenv("KHOICE_BMP_TILE_POS", str(TILE))
    monkeypatch.setenv("KHOICE_BMP_SPLIT_POS", str(SPLIT))


@pytest.mark.gpu
@pytest.mark.parametrize("k", PLANT_K)
def test_exp2_planted_edges(eng, small_tiles, k):
    seqs, group_of, pivots, pivot_group, _ = planted_case(k)
    want, _, _ = planted_answer(k)
    check(eng, seqs, group_of, pivots, pivot_group, k, want=want)


# ---------------------------------------------------------------- 3. shapes
def related(rng, n, length, rate=0.03):
    """n texts: copies of one random ancestor with substitutions."""
    anc = rng.integers(0, 4, length)
    out = []
    for _ in range(n):
        g = anc.copy()
        hit = rng.random(length) < rate
        g[hit] = rng.integers(0, 4, int(hit.sum()))
        out.append(np.frombuffer(b"ACGT", dtype=np.uint8)[g].tobytes())
    return out


@functools.lru_cache(maxsize=None)
def shape_case(name, length=5_000):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "counter_widths":          # groups of 1, 2, 17 and 70: counters of 1, 2, 5 and 7 slices; every kind of pivot
        sizes = (1, 2, 17, 70)
        fam = [related(rng, n + 2, length) for n in sizes]
        seqs = [t for f, n in zip(fam, sizes) for t in f[:n]]
        group_of = [g for g, n in enumerate(sizes) for _ in range(n)]
        n_run = fam[2][18][:2_000] + b"N" * 40 + fam[2][18][2_000:]
        pivots = [fam[0][1], fam[1][0], fam[2][17], n_run, fam[3][70], b"ACGT"]
        return seqs, group_of, pivots, [0, 1, 2, 2, 3, 3]     # fam[1][0]: identical to a genome of its group; ACGT: shorter than k
    if name == "two_and_none":            # two pivots in one group, none in another
        fam = [related(rng, 4, length) for _ in range(3)]
        return [t for f in fam for t in f[:2]], [0, 0, 1, 1, 2, 2], [fam[0][2], fam[2][2], fam[2][3]], [0, 2, 2]
    if name == "one_group":
        fam = related(rng, 4, length)
        return fam[:3], [0, 0, 0], [fam[3]], [0]
    if name == "groups65":                # 65 groups of one genome of one ancestor: a 7-slice across counter, > 64 bins per pivot
        fam = related(rng, 68, length)
        return fam[:65], list(range(65)), fam[65:], [0, 31, 64]
    if name == "many_pivots":             # more pivots than the 16 (k <= 10) or 4 (k = 11) operands of a round
        fam = [related(rng, 8, length) for _ in range(3)]
        return ([t for f in fam for t in f[:2]], [0, 0, 1, 1, 2, 2],
                [t for f in fam for t in f[2:]], [g for g in range(3) for _ in range(6)])
    raise KeyError(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name,k", [("counter_widths", 9), ("two_and_none", 9), ("one_group", 9), ("groups65", 9),
                                    ("many_pivots", 9), ("many_pivots", 11), ("two_and_none", 11)])
def test_exp2_shapes(eng, name, k):
    seqs, group_of, pivots, pivot_group = shape_case(name)
    got, _ = check(eng, seqs, group_of, pivots, pivot_group, k)
    if name == "counter_widths":
        assert (got["within_hist"][5] == 0).all() and got["within_only"][5] == 0 and got["distinct_per_pivot"][5] == 0
        assert got["within_only"][1] == 0                                   # the pivot that is a genome of its group
        assert got["within_hist"][4][60:72].sum() > 0                       # counts that need the seventh slice
    if name == "one_group":
        assert (got["across_hist"] == 0).all() and (got["across_only"] == got["distinct_per_pivot"]).all()
    if name == "groups65":
        assert got["across_hist"][:, 40:66].sum() > 0


# ---------------------------------------------------------------- 4. clamps
@pytest.mark.gpu
@pytest.mark.parametrize("cs", (1, 3, 5000))
@pytest.mark.parametrize("hist_len", (2, 4, 5001))
def test_exp2_clamps(eng, cs, hist_len):
    seqs, group_of, pivots, pivot_group = species()
    check(eng, seqs, group_of, pivots, pivot_group, 10, cs=cs, hist_len=hist_len)


# ---------------------------------------------------------------- 5. the other form, declining, arguments
def by_sets(eng, seqs, group_of, pivots, pivot_group, k, **kw):
    got, d = run(eng, seqs, group_of, pivots, pivot_group, k, **kw)
    assert d["bmp_build"] == 0 and d["bmp_pivot"] == 0 and d["setop"] > 0, d
    return got, d


@pytest.mark.gpu
@pytest.mark.parametrize("k", (13, 21, 41))
def test_exp2_set_form_above_the_bitmaps(eng, k):
    by_sets(eng, *species(8_000), k)


@pytest.mark.gpu
def test_exp2_switches_and_declines(eng, monkeypatch):
    k = 9
    case = species(8_000)
    want = oracle(*case, k)
    got, _ = check(eng, *case, k, want=want)
    for name in ("KHOICE_NO_BMP", "KHOICE_NO_SKM"):
        monkeypatch.setenv(name, "1")
        other, _ = by_sets(eng, *case, k, want=want)
        monkeypatch.delenv(name)
        assert same(got, other)
    monkeypatch.setenv("KHOICE_BMP_MAX_BYTES", "1")                     # the bitmaps do not fit: declined, not retried
    _, d = by_sets(eng, *case, k, want=want)
    assert d["retries"] == 0, d
    monkeypatch.delenv("KHOICE_BMP_MAX_BYTES")
    check(eng, *case, k, want=want)
    for shape in ("one_group", "two_and_none", "counter_widths"):       # the set form's own corners: no other group, a group
                                                                        # without pivot, a pivot without k-mers
        monkeypatch.setenv("KHOICE_NO_BMP", "1")
        by_sets(eng, *shape_case(shape), k)
        monkeypatch.delenv("KHOICE_NO_BMP")


@pytest.mark.gpu
def test_exp2_bad_arguments(eng):
    from khoice_amd import engine as E
    seqs, group_of, pivots, pivot_group = species(8_000)
    bad = [dict(pivot_group=[0, 1, 3]),                                 # a pivot's group outside [0, ngroups)
           dict(pivot_group=[0, 1, -1]),
           dict(group_of=[0, 0, 0, 0, 0, 0, 2, 2, 2], pivot_group=[0, 1, 2]),   # a pivot whose group has no genome
           dict(hist_len=1), dict(k=0), dict(k=65)]
    for change in bad:
        args = dict(seqs=seqs, group_of=group_of, pivots=pivots, pivot_group=pivot_group, k=9, hist_len=5001)
        args.update(change)
        with pytest.raises(E.KhoiceError) as ei:
            eng.exp2_run(**args)
        assert ei.value.code == -1, change                              # KH_E_ARG
        assert len(str(ei.value)) > len("khoice_hip error -1: "), change   # with a message from kh_last_error
    check(eng, seqs, group_of, pivots, pivot_group, 9)                  # and the context still works


# ---------------------------------------------------------------- 6. workflow
def tree_files(root):
    out = {}
    for scope in ("within", "across"):
        top = os.path.join(root, f"{scope}_dataset_results_type_2")
        for d, _, names in os.walk(top):
            for n in names:
                if n.endswith(".hist.txt"):
                    out[os.path.relpath(os.path.join(d, n), root)] = open(os.path.join(d, n)).read()
    return out


@pytest.mark.gpu
def test_exp2_run_fused_matches_oracle_and_run_batched(tmp_path):
    from khoice_amd.workflow import exp_type_2 as W2
    from tests.test_workflow_cpu import expected_type2_outputs
    ks = [9, 12, 21]
    root = str(tmp_path / "fused")
    os.makedirs(root)
    synth.write_type2_tree(root, 3, 2, 30_000)
    root2 = str(tmp_path / "batched")
    shutil.copytree(root, root2)
    out = W2.run_fused(root, ks, 3)
    files, within, across = expected_type2_outputs(root, ks, 3, str(tmp_path / "expected"))
    assert len(files) == 4 * 3 * len(ks) and tree_files(root) == files          # within / across x intersect / subtract
    assert all(text.count("\n") == 65535 for text in files.values())
    assert out["within"] == within and out["across"] == across and out["processes"] == 0
    out2 = W2.run_batched(root2, ks, 3)
    assert tree_files(root2) == tree_files(root) and out2 == out
    for name in ("within", "across"):
        rel = f"{name}_dataset_analysis_type_2/{name}_dataset_analysis.csv"
        assert open(os.path.join(root, rel)).read() == open(os.path.join(root2, rel)).read() == out[name]


@pytest.mark.gpu
def test_exp2_run_fused_one_dataset(tmp_path):
    """One dataset: no other group, so neither runner writes across files — and the shared summary stage, which
    reads them, stops both runners the same way.  The within files are the oracle's."""
    from khoice_amd.workflow import exp_type_2 as W2
    from tests.test_workflow_cpu import expected_type2_outputs
    ks = [9, 21]
    root = str(tmp_path / "fused")
    os.makedirs(root)
    synth.write_type2_tree(root, 1, 2, 30_000)
    root2 = str(tmp_path / "batched")
    shutil.copytree(root, root2)
    for runner, r in ((W2.run_fused, root), (W2.run_batched, root2)):
        with pytest.raises(FileNotFoundError):
            runner(r, ks, 1)
    files, _, _ = expected_type2_outputs_within(root, ks, tmp_path)
    assert tree_files(root) == files == tree_files(root2) and len(files) == 2 * len(ks)


def expected_type2_outputs_within(root, ks, tmp_path):
    """tests.test_workflow_cpu.expected_type2_outputs needs two datasets for its CSVs: the within files of one dataset
    from the same oracle calls."""
    from khoice_amd.workflow import exp_type_2 as W2
    files = {}
    for k in ks:
        sets = [O.set_counts(O.build(O.read_fasta_bytes(os.path.join(root, f"input_type_2/rest_of_set/dataset_1/{g}.fna.gz")), k), 1)
                for g in W2.rest_of_set(root, 1)]
        union = O.union_sum(sets, 5000)
        pivot = O.set_counts(O.build(O.read_fasta_bytes(os.path.join(root, "input_type_2/pivot/dataset_1/pivot_1.fna.gz")), k), 1)
        for op, db in (("intersect", O.intersect(pivot, union, "sum", 5000)), ("subtract", O.kmers_subtract(pivot, union))):
            files[f"within_dataset_results_type_2/k_{k}/dataset_1/{op}/dataset_1_pivot_{op}_group.hist.txt"] = O.histogram_text(db, 65535)
    return files, None, None


# ---------------------------------------------------------------- 7. preconditions, without a GPU
@pytest.mark.parametrize("k", PLANT_K)
def test_planted_codes_lie_on_the_edges(k):
    edges = edge_codes(k)
    ncodes, rbits = 4 ** k, min(RANGE_BITS, 2 * k)
    nranges = ncodes >> rbits
    assert nranges == {5: 1, 8: 1, 11: 4, 12: 16}[k]
    assert all(is_canonical(c, k) for c in edges.values()) and len(set(edges.values())) == len(edges)
    for r in range(nranges):
        lo, hi = r << rbits, ((r + 1) << rbits) - 1
        first, last = edges[f"range{r}_first"], edges[f"range{r}_last"]
        assert lo <= first < last <= hi
        assert not any(is_canonical(c, k) for c in range(lo, first))           # nothing canonical in front of it
        assert not any(is_canonical(c, k) for c in range(last + 1, hi + 1))    # nor behind it
    assert edges["range0_first"] == 0                                       # bit 0 of word 0, the first word of the first wave
    top = edges[f"range{nranges - 1}_last"]                                 # the last word of the bitmap that holds anything
    assert top == max(c for c in range(ncodes - (1 << rbits), ncodes) if is_canonical(c, k))
    assert edges["bit0"] % 64 == 0 and edges["bit0"] > 0
    if k >= 6:
        assert edges["bit63"] % 64 == 63
        assert edges["wave_last_word"] // 64 == 63 and edges["wave_first_word"] // 64 == 64
        lwf = edges.get("last_wave_first_word", top)
        assert (lwf // 64) % 64 == 0 and lwf // 4096 == top // 4096
    else:                                                                   # k = 5: one wave of 16 words, the last holds the top code
        assert ncodes // 64 == 16 and top // 64 == 15
        assert not any(is_canonical(c, k) for c in range(63, ncodes, 64))   # ..TTT is never the smaller strand of a 5-mer


@pytest.mark.parametrize("k", PLANT_K)
def test_planted_case_holds_every_count_of_every_pivot(k):
    seqs, group_of, pivots, pivot_group, plants = planted_case(k)
    codes = [c for c, *_ in plants]
    assert len(set(codes)) == len(codes) and all(is_canonical(c, k) for c in codes)
    assert set(edge_codes(k).values()) <= set(codes)
    assert max(len(t) for t in seqs + pivots) > 2 * SPLIT                   # several splits of several tiles
    for gi, text in enumerate(seqs):                                        # every code in exactly the texts it was meant for
        assert set(plain_set(text, k)) == {c for c, _, _, genomes, _ in plants if gi in genomes}
    for p, text in enumerate(pivots):
        assert set(plain_set(text, k)) == {c for c, cat, q, _, _ in plants if q == p and cat[0] != "group"}
    for code, cat, p, genomes, _ in plants:
        mine = [gi for gi in genomes if group_of[gi] == p]
        if cat[0] == "within":
            assert len(mine) == len(genomes) == cat[1]
        elif cat[0] == "across":
            assert not mine and len({group_of[gi] for gi in genomes}) == len(genomes) == cat[1]
        else:
            assert len(mine) == len(genomes) == 1
        if cat[0] == "rc":                                                  # the genome spells the other strand
            assert kmer_text(code, k) in pivots[p].decode().split("N")
            assert kmer_text(code, k) not in seqs[genomes[0]].decode().split("N")
            assert kmer_text(revcomp_code(code, k), k) in seqs[genomes[0]].decode().split("N")
    cats = {(cat, p) for _, cat, p, _, _ in plants}
    for p, n in enumerate(PLANT_SIZES):
        assert {(("within", v), p) for v in range(1, n + 1)} | {(("across", v), p) for v in range(len(PLANT_SIZES))} \
            | {(("group",), p), (("rc",), p)} <= cats
    want, occ_w, occ_a = planted_answer(k)
    theirs = oracle(seqs, group_of, pivots, pivot_group, k)
    for f in FIELDS:
        assert (want[f] == theirs[f]).all(), f
    assert all(v > 0 for occ in occ_w + occ_a for v in occ)                 # every within and across bin of every pivot
    for p, n in enumerate(PLANT_SIZES):
        assert all(theirs["within_hist"][p, v + 1] > 0 for v in range(1, n + 1)) and theirs["within_only"][p] > 0
        assert all(theirs["across_hist"][p, v + 1] > 0 for v in range(1, len(PLANT_SIZES))) and theirs["across_only"][p] > 0


def test_shape_cases_are_what_they_claim():
    k = 9
    seqs, group_of, pivots, pivot_group = shape_case("counter_widths")
    assert [group_of.count(g) for g in range(4)] == [1, 2, 17, 70]
    assert [(n).bit_length() for n in (1, 2, 17, 70)] == [1, 2, 5, 7]
    assert pivots[1] in [s for s, g in zip(seqs, group_of) if g == 1] and len(pivots[5]) < k and b"N" * 40 in pivots[3]
    assert len(seqs) + len(pivots) > 16
    seqs, group_of, pivots, pivot_group = shape_case("two_and_none")
    assert pivot_group.count(2) == 2 and pivot_group.count(1) == 0 and len(seqs) + len(pivots) > 4
    seqs, group_of, pivots, pivot_group = shape_case("groups65")
    ng = max(group_of) + 1
    assert ng == 65 and ng.bit_length() == 7 and all(1 + 1 + ng > 64 for _ in pivots)
    seqs, group_of, pivots, pivot_group = shape_case("many_pivots")
    assert len(pivots) > 16
