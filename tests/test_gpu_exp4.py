"""kh_exp4_run (fused experiment type 4) against the oracles as they stand: the confusion-matrix rows and unique counts
of oracle/merge_oracle.py for every pivot against the `set_counts 1` union of every group, compared with == on float64
(the order of the sum is part of the contract), the histograms of the -cs unions and the distinct counts; and from the
statistics which form did the work: k_bmp_build + k_bmp_count + k_bmp_present + k_bmp_member (kh_bmp.hip) for k <= 12
and at most 64 groups, builds, unions and the membership search inside the library otherwise.

The unmarked tests at the end prove on the CPU what the GPU cases rely on: the planted codes lie on the edges their
names say, every planted multiplicity and membership size occurs, every expected cell is non-zero, a sum in another
order gives another row, and merge_lists.confusion_from_rows writes the reference's files."""
import functools
import json
import os
import random
import shutil

import numpy as np
import pytest

from khoice_amd import synth
from oracle import kmer_oracle as O
from oracle import merge_oracle as MO
from tests.test_gpu_exp2_bmp import (RANGE_BITS, SPLIT, TILE, edge_codes, is_canonical, kmer_text, related,
                                     revcomp_code)

PLANT_K = (5, 8, 11, 12)
FIELDS = ("rows", "unique", "within_hist", "distinct_per_seq", "distinct_per_pivot")
KERNELS = ("bmp_build", "bmp_count", "bmp_present", "bmp_member", "bmp_readout", "bmp_pivot", "union_tagged", "skm_union",
           "setop")
KMC_CS = 255


@pytest.fixture(scope="module")
def eng():
    from khoice_amd import build as kbuild
    from khoice_amd import engine as E
    kbuild.build_library()
    e = E.Engine(0)
    yield e
    e.close()


# ---------------------------------------------------------------- the oracles' answer
def fasta_of(text):
    return b"".join(b">r\n" + rec + b"\n" for rec in bytes(text).split(b"\n"))


@functools.lru_cache(maxsize=None)
def plain_set(text, k):
    """`kmc -ci1` + `set_counts 1` of a cleaned text (records separated by a line feed)."""
    return O.set_counts(O.build(fasta_of(text), k), 1)


@functools.lru_cache(maxsize=None)
def counted(text, k, pivot_cs):
    """`kmc -ci1` of a pivot, counters saturating at pivot_cs."""
    return O.build(fasta_of(text), k, cs=pivot_cs)


def oracle(seqs, group_of, pivots, k, cs=5000, hist_len=5001, pivot_cs=KMC_CS):
    ng = max(group_of) + 1
    sets = [plain_set(bytes(t), k) for t in seqs]
    unions = [O.union_sum([s for s, g in zip(sets, group_of) if g == h], cs) for h in range(ng)]
    group_sets = [O.set_counts(u, 1) for u in unions]
    want = {"rows": np.zeros((len(pivots), ng), dtype=np.float64), "unique": np.zeros(len(pivots), dtype=np.uint64),
            "within_hist": np.array([O.histogram(u, hist_len - 1) for u in unions], dtype=np.uint64),
            "distinct_per_seq": np.array([len(s) for s in sets], dtype=np.uint64),
            "distinct_per_pivot": np.zeros(len(pivots), dtype=np.uint64)}
    for p, t in enumerate(pivots):
        db = counted(bytes(t), k, pivot_cs)
        row, unique = MO.confusion_row(db, group_sets)
        want["rows"][p] = row
        want["unique"][p] = unique
        want["distinct_per_pivot"][p] = len(db)
    return want


def deltas(st0, st1):
    d = {n: st1["kernels"][n]["launches"] - st0["kernels"][n]["launches"] for n in KERNELS}
    for n in ("retries", "builds", "bases", "kmers", "distinct", "setops", "setop_in", "setop_out", "text_packed"):
        d[n] = st1[n] - st0[n]
    return d


def same(a, b):
    return all(a[f].shape == b[f].shape and (a[f] == b[f]).all() for f in FIELDS)


def run(eng, seqs, group_of, pivots, k, cs=5000, hist_len=5001, pivot_cs=KMC_CS, want=None, texts=None):
    """texts: (seqs, pivots) to hand to the library in place of the host bytes (device-resident ones)."""
    eng.profile(True)
    st0 = eng.stats()
    a, b = texts if texts else (seqs, pivots)
    got = eng.exp4_run(a, group_of, b, k, cs=cs, hist_len=hist_len, pivot_cs=pivot_cs)
    st1 = eng.stats()
    eng.profile(False)
    if want is None:
        want = oracle(seqs, group_of, pivots, k, cs, hist_len, pivot_cs)
    for f in FIELDS:
        assert got[f].shape == want[f].shape and got[f].dtype == want[f].dtype, (f, k, got[f].shape, want[f].shape)
        assert (got[f] == want[f]).all(), (f, k, cs, hist_len, pivot_cs, np.argwhere(got[f] != want[f])[:8].tolist())
    return got, deltas(st0, st1)


def check(eng, seqs, group_of, pivots, k, **kw):
    """The oracles' answers, and the bitmap form alone did the work."""
    got, d = run(eng, seqs, group_of, pivots, k, **kw)
    n = 1 if len(pivots) else 0
    assert d["bmp_build"] >= 1 and d["bmp_present"] == 1 and d["bmp_count"] == n and d["bmp_member"] == n, d
    assert d["bmp_readout"] == 0 and d["bmp_pivot"] == 0 and d["union_tagged"] == 0 and d["skm_union"] == 0, d
    assert d["setop"] == 0 and d["retries"] == 0, d
    assert d["builds"] == len(seqs) + len(pivots), d
    return got, d


def by_sets(eng, seqs, group_of, pivots, k, **kw):
    got, d = run(eng, seqs, group_of, pivots, k, **kw)
    assert all(d[n] == 0 for n in KERNELS if n.startswith("bmp_")) and d["setop"] > 0, d
    return got, d


@functools.lru_cache(maxsize=None)
def species(n=20_000):
    """3 groups x 3 genomes, and per group a pivot: a fourth genome of the same ancestor."""
    items = synth.species_set(3, 3, n)
    pivots = [synth.clean_text(synth.genome_records(s, 3, n, synth.ancestor(s, n))) for s in (1, 2, 3)]
    return [t for _, _, t in items], [s - 1 for s, _, _ in items], pivots


# ---------------------------------------------------------------- 1. every k
@pytest.mark.gpu
@pytest.mark.parametrize("k", range(1, 13))
def test_exp4_every_k(eng, k):
    seqs, group_of, pivots = species()
    want = oracle(seqs, group_of, pivots, k)
    got1, d1 = check(eng, seqs, group_of, pivots, k, want=want)
    got2, d2 = check(eng, seqs, group_of, pivots, k, want=want)
    assert same(got1, got2) and d1 == d2, (d1, d2)
    assert d1["bases"] == sum(len(s) for s in seqs + pivots)
    assert d1["distinct"] == int(want["distinct_per_seq"].sum() + want["distinct_per_pivot"].sum())


# ---------------------------------------------------------------- 2. planted codes at every edge
PLANT_SIZES = (2, 1, 2)          # genomes per group
PLANT_PIVOTS = 2
MULTS = (1, 2, 254, 255, 256, 300)
PLANT_CS = (255, 1, 3)           # pivot_cs of the planted runs


def palindromes(k, n, rng):
    """n codes that are their own reverse complement (even k)."""
    out = set()
    while len(out) < n:
        half = rng.randrange(4 ** (k // 2))
        code = (half << k) | revcomp_code(half, k // 2)
        assert code == revcomp_code(code, k)
        out.add(code)
    return sorted(out)


@functools.lru_cache(maxsize=None)
def planted_case(k):
    """Pivot texts made of chosen canonical codes, every occurrence a record of its own.  plants = [(code, what, pivot,
    multiplicity, groups holding it, both strands?)]: the edge codes of the read-out's walk and of the build's ranges
    (tests.test_gpu_exp2_bmp.edge_codes: word 0, the last word that holds anything, bit 0 and bit 63 of a word, words
    63 and 64, the first and last code of every build range), palindromes for even k, and seeded filling, so that
    every multiplicity meets every number of groups (0 .. all) in both pivots.  A k-mer of multiplicity >= 2 marked
    `both` is spelled on both strands in the pivot; a group holds a k-mer in one of its genomes, every other time as
    the reverse complement."""
    ng = len(PLANT_SIZES)
    group_of = [g for g, n in enumerate(PLANT_SIZES) for _ in range(n)]
    first = [group_of.index(g) for g in range(ng)]
    rng = random.Random(4000 + k)
    edges = dict(edge_codes(k))
    if k % 2 == 0:
        for i, c in enumerate(c for c in palindromes(k, 4, rng) if c not in edges.values()):
            edges[f"palindrome{i}"] = c
    used = set(edges.values())
    assert len(used) == len(edges)

    def fresh():
        while True:
            c = rng.randrange(4 ** k)
            if is_canonical(c, k) and c != revcomp_code(c, k) and c not in used:
                used.add(c)
                return c

    combos = [(m, size) for m in MULTS for size in range(ng + 1)]
    todo = sorted(edges.items())
    plants = []
    i = 0
    while todo or i < 2 * PLANT_PIVOTS * len(combos):
        mult, size = combos[(i // PLANT_PIVOTS) % len(combos)]
        p = i % PLANT_PIVOTS
        what, code = todo.pop() if todo else ("fill", fresh())
        if mult > 2 and i >= PLANT_PIVOTS * len(combos):
            mult = 1 + i % 2                                   # (the large multiplicities once per pivot and size)
        groups = tuple(sorted((i + j) % ng for j in range(size)))
        both = mult >= 2 and code != revcomp_code(code, k) and i % 3 != 0
        plants.append((code, what, p, mult, groups, both))
        i += 1
    texts = [[] for _ in group_of]
    ptexts = [[] for _ in range(PLANT_PIVOTS)]
    for j, (code, _, p, mult, groups, both) in enumerate(plants):
        rc = revcomp_code(code, k)
        for m in range(mult):
            ptexts[p].append(kmer_text(rc if both and m % 2 else code, k))
        for g in groups:
            texts[first[g] + j % PLANT_SIZES[g]].append(kmer_text(rc if (j + g) % 2 else code, k))
    for t in ptexts:
        rng.shuffle(t)                                          # the occurrences of a code lie in several tiles and splits
    join = lambda t: "N".join(t).encode()
    return [join(t) for t in texts], group_of, [join(t) for t in ptexts], plants


@pytest.fixture
def small_tiles(monkeypatch):
    monkeypatch.setenv("KHOICE_BMP_TILE_POS", str(TILE))
    monkeypatch.setenv("KHOICE_BMP_SPLIT_POS", str(SPLIT))


@pytest.mark.gpu
@pytest.mark.parametrize("pivot_cs", PLANT_CS)
@pytest.mark.parametrize("k", PLANT_K)
def test_exp4_planted_edges(eng, small_tiles, k, pivot_cs):
    seqs, group_of, pivots, _ = planted_case(k)
    check(eng, seqs, group_of, pivots, k, pivot_cs=pivot_cs)


# ---------------------------------------------------------------- 3. the order of the sum
ORDER_K, ORDER_SIZES = 9, (3, 5, 6, 7)


@functools.lru_cache(maxsize=None)
def order_case():
    """7 groups of one genome and one pivot of about 5 kbp in four pieces: piece j lies in ORDER_SIZES[j] groups, so its
    k-mers add 1/3, 1/5, 1/6 and 1/7 of their counts: sums whose roundings depend on the order."""
    rng = np.random.default_rng(77)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    pieces = [letters[rng.integers(0, 4, 1250)].tobytes() for _ in ORDER_SIZES]
    held = [sorted(rng.permutation(7)[:n].tolist()) for n in ORDER_SIZES]
    seqs = [b"N".join(pc for pc, h in zip(pieces, held) if g in h) for g in range(7)]
    return seqs, list(range(7)), [b"N".join(pieces)]


def order_addends(k=ORDER_K):
    """[(code, groups holding it, addend)] of the order case's pivot, as the reference forms them."""
    seqs, group_of, pivots = order_case()
    db = counted(pivots[0], k, KMC_CS)
    sets = [plain_set(t, k) for t in seqs]
    out = []
    for code in sorted(db):
        m = [g for g, s in enumerate(sets) if code in s]
        if m:
            out.append((code, m, 1 / len(m) * db[code]))
    return out


@pytest.mark.gpu
def test_exp4_sums_in_code_order(eng):
    seqs, group_of, pivots = order_case()
    check(eng, seqs, group_of, pivots, ORDER_K)


# ---------------------------------------------------------------- 4. shapes
@functools.lru_cache(maxsize=None)
def shape_case(name, length=3_000):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "one_group":
        fam = related(rng, 4, length)
        return fam[:3], [0, 0, 0], [fam[3]]
    if name == "one_pivot":
        fam = [related(rng, 3, length) for _ in range(3)]
        return [t for f in fam for t in f[:2]], [0, 0, 1, 1, 2, 2], [fam[1][2]]
    if name == "five_pivots":             # shorter than k, nothing but N, a genome of a group, two ordinary ones
        fam = [related(rng, 4, length) for _ in range(3)]
        return ([t for f in fam for t in f[:2]], [0, 0, 1, 1, 2, 2],
                [b"ACGT", b"N" * 50, fam[1][0], fam[0][2], fam[2][3]])
    if name == "no_pivot":
        fam = [related(rng, 2, length) for _ in range(3)]
        return [t for f in fam for t in f], [0, 0, 1, 1, 2, 2], []
    if name == "counter_widths":          # groups of 1, 2, 17 and 70: counters of 1, 2, 5 and 7 slices
        sizes = (1, 2, 17, 70)
        fam = [related(rng, n + 1, length) for n in sizes]
        return ([t for f, n in zip(fam, sizes) for t in f[:n]], [g for g, n in enumerate(sizes) for _ in range(n)],
                [fam[2][17], fam[3][70]])
    if name in ("groups64", "groups65"):  # one genome per group, one ancestor: k-mers in up to all groups; mask bit 63
        ng = int(name[-2:])
        fam = related(rng, ng + 2, length)
        return fam[:ng], list(range(ng)), fam[ng:]
    if name in ("pivots20", "pivots6"):   # more pivots than the 16 (k <= 10) or 4 (k = 11) operands of a read-out round
        n = int(name[6:])
        fam = [related(rng, 2 + (n + 2) // 3, length) for _ in range(3)]
        return [t for f in fam for t in f[:2]], [0, 0, 1, 1, 2, 2], [t for f in fam for t in f[2:]][:n]
    raise KeyError(name)


SHAPES = [(n, k) for k in (9, 11) for n in ("one_group", "one_pivot", "five_pivots", "no_pivot", "counter_widths", "groups64")]
SHAPES += [("pivots20", 9), ("pivots6", 11)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,k", SHAPES)
def test_exp4_shapes(eng, name, k):
    seqs, group_of, pivots = shape_case(name)
    got, _ = check(eng, seqs, group_of, pivots, k)
    if name == "five_pivots":
        for p in (0, 1):
            assert (got["rows"][p] == 0).all() and got["unique"][p] == 0 and got["distinct_per_pivot"][p] == 0
        assert got["unique"][2] == 0 and got["rows"][2, 1] > 0             # the pivot that is a genome of group 1
    if name == "no_pivot":
        assert got["rows"].shape == (0, 3) and got["unique"].shape == (0,)
    if name == "counter_widths":
        assert got["within_hist"][3][60:71].sum() > 0                      # counts that need the seventh slice
    if name == "groups64":
        assert (got["rows"][:, 63] > 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("k", (9, 11))
def test_exp4_65_groups_go_through_sets(eng, k):
    seqs, group_of, pivots = shape_case("groups65")
    got, d = by_sets(eng, seqs, group_of, pivots, k)
    assert d["retries"] == 0 and (got["rows"][:, 64] > 0).all(), d


# ---------------------------------------------------------------- 5. clamps
@pytest.mark.gpu
@pytest.mark.parametrize("cs", (1, 3, 5000))
@pytest.mark.parametrize("hist_len", (2, 4, 5001))
def test_exp4_clamps(eng, cs, hist_len):
    seqs, group_of, pivots = species()
    check(eng, seqs, group_of, pivots, 10, cs=cs, hist_len=hist_len)


# ---------------------------------------------------------------- 6. the set form, declining
@pytest.mark.gpu
@pytest.mark.parametrize("k", (13, 16, 21, 41))
def test_exp4_set_form_above_the_bitmaps(eng, k):
    by_sets(eng, *species(8_000), k)


@pytest.mark.gpu
def test_exp4_switches_and_declines(eng, monkeypatch):
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


# ---------------------------------------------------------------- 7. device-resident texts
@pytest.mark.gpu
def test_exp4_device_texts(eng, tmp_path):
    k = 9
    seqs, group_of, pivots = species()
    paths = []
    for i, t in enumerate(seqs + pivots):
        paths.append(str(tmp_path / f"t{i}.fa"))
        with open(paths[-1], "wb") as fh:
            fh.write(fasta_of(t))
    want = oracle(seqs, group_of, pivots, k)
    host, hd = check(eng, seqs, group_of, pivots, k, want=want)
    texts = eng.ingest_fasta(paths)
    try:
        assert all(ptr % 16 == 0 and n == len(t) for (ptr, n), t in zip(texts.seqs, seqs + pivots))
        dev, dd = check(eng, seqs, group_of, pivots, k, want=want, texts=(texts.seqs[:len(seqs)], texts.seqs[len(seqs):]))
    finally:
        texts.free()
    assert same(host, dev)
    assert hd["text_packed"] == sum(len(t) for t in seqs + pivots) and dd["text_packed"] == 0, (hd, dd)
    with pytest.raises(ValueError):
        eng.exp4_run(seqs, group_of, [(0, 0)], k)


# ---------------------------------------------------------------- 8. arguments
@pytest.mark.gpu
def test_exp4_bad_arguments(eng):
    from khoice_amd import engine as E
    seqs, group_of, pivots = species(8_000)
    bad = [dict(group_of=[0, 0, 0, 1, 1, 1, 2, 2, -1]),                 # a group outside [0, ngroups)
           dict(group_of=[0, 0, 0, 0, 0, 0, 2, 2, 2]),                  # a group without a genome
           dict(hist_len=1), dict(k=0), dict(k=65), dict(pivot_cs=0)]
    for change in bad:
        args = dict(seqs=seqs, group_of=group_of, pivots=pivots, k=9, hist_len=5001)
        args.update(change)
        with pytest.raises(E.KhoiceError) as ei:
            eng.exp4_run(**args)
        assert ei.value.code == -1, change                              # KH_E_ARG
        assert len(str(ei.value)) > len("khoice_hip error -1: "), change   # with a message from kh_last_error
    check(eng, seqs, group_of, pivots, 9)                               # and the context still works


# ---------------------------------------------------------------- 9. workflow
def tree_files(root, top):
    out = {}
    for d, _, names in os.walk(os.path.join(root, top)):
        for n in names:
            out[os.path.relpath(os.path.join(d, n), os.path.join(root, top))] = open(os.path.join(d, n)).read()
    return out


@pytest.mark.gpu
def test_exp4_run_fused_matches_oracle_and_run_batched(tmp_path):
    from khoice_amd.workflow import exp_type_4 as W4
    from tests.test_workflow_cpu import expected_type4_outputs
    ks = [9, 12, 21]
    root = str(tmp_path / "fused")
    os.makedirs(root)
    synth.write_type4_tree(root, 3, 2, 30_000)
    root2 = str(tmp_path / "batched")
    shutil.copytree(root, root2)
    out = W4.run_fused(root, ks, 3)
    want, cat = {}, ""
    for k in ks:
        want.update(expected_type4_outputs(root, k, 3))
    for k in sorted(ks, key=str):                                          # `cat values/*.csv`: the shell's order
        cat += want[f"values/k_{k}_accuracy_values.csv"]
    want["accuracy_values.csv"] = cat
    assert tree_files(root, "accuracies_type_4") == want and len(want) == 3 * len(ks) + 1
    assert out == {"accuracy_values": os.path.join(root, "accuracies_type_4/accuracy_values.csv"), "processes": 0}
    hists = tree_files(root, "unions_type_4")
    assert sorted(hists) == sorted(f"rest_of_set/k_{k}/dataset_{n}/dataset_{n}.hist.txt" for k in ks for n in (1, 2, 3))
    for k in ks:
        for n in (1, 2, 3):
            sets = [O.set_counts(O.build(O.read_fasta_bytes(os.path.join(root, f"input_type4/rest_of_set/dataset_{n}/{g}.fna.gz")), k), 1)
                    for g in W4.rest_of_set(root, n)]
            assert hists[f"rest_of_set/k_{k}/dataset_{n}/dataset_{n}.hist.txt"] == O.histogram_text(O.union_sum(sets, 5000), 65535)
    out2 = W4.run_batched(root2, ks, 3)
    assert tree_files(root2, "accuracies_type_4") == want and tree_files(root2, "unions_type_4") == hists
    assert out2 == {"accuracy_values": os.path.join(root2, "accuracies_type_4/accuracy_values.csv"), "processes": 0}


# ---------------------------------------------------------------- 10. preconditions, without a GPU
@pytest.mark.parametrize("k", PLANT_K)
def test_planted_codes_lie_on_the_edges_their_names_say(k):
    _, _, pivots, plants = planted_case(k)
    ncodes, rbits = 4 ** k, min(RANGE_BITS, 2 * k)
    nranges = ncodes >> rbits
    assert nranges == {5: 1, 8: 1, 11: 4, 12: 16}[k]
    named = {what: code for code, what, *_ in plants if what != "fill"}
    codes = [code for code, *_ in plants]
    assert len(set(codes)) == len(codes) and all(is_canonical(c, k) for c in codes)
    canon = [c for c in range(ncodes) if is_canonical(c, k)] if k <= 8 else None
    for r in range(nranges):
        lo, hi = r << rbits, ((r + 1) << rbits) - 1
        first, last = named[f"range{r}_first"], named[f"range{r}_last"]
        assert lo <= first < last <= hi
        assert not any(is_canonical(c, k) for c in range(lo, first))        # nothing canonical in front of it
        assert not any(is_canonical(c, k) for c in range(last + 1, hi + 1))  # nor behind it
    assert named["range0_first"] == 0                                       # bit 0 of word 0, block 0
    top = named[f"range{nranges - 1}_last"]                                 # the last word of the code space that holds anything
    if canon:
        assert top == canon[-1]
    assert named["bit0"] % 64 == 0 and named["bit0"] > 0
    if k >= 6:
        assert named["bit63"] % 64 == 63
        assert named["wave_last_word"] // 64 == 63 and named["wave_first_word"] // 64 == 64   # the block edge of the ranks
        lwf = named.get("last_wave_first_word", top)
        assert (lwf // 64) % 64 == 0 and lwf // 4096 == top // 4096
    else:
        assert ncodes // 64 == 16 and top // 64 == 15                       # k = 5: one block of 16 words
    pal = [c for w, c in named.items() if w.startswith("palindrome")]
    assert (len(pal) >= 3 and all(c == revcomp_code(c, k) for c in pal)) if k % 2 == 0 else not pal


@pytest.mark.parametrize("k", PLANT_K)
def test_planted_case_holds_every_multiplicity_and_membership(k):
    seqs, group_of, pivots, plants = planted_case(k)
    ng = len(PLANT_SIZES)
    assert min(len(t) for t in pivots) > 2 * SPLIT                           # several splits of several tiles
    group_sets = [set().union(*[set(plain_set(t, k)) for t, g in zip(seqs, group_of) if g == h]) for h in range(ng)]
    for p in range(PLANT_PIVOTS):
        raw = counted(pivots[p], k, 1 << 30)
        mine = [pl for pl in plants if pl[2] == p]
        assert {code: mult for code, _, _, mult, _, _ in mine} == raw           # exactly the planted codes and multiplicities
        for code, _, _, _, groups, _ in mine:
            assert tuple(g for g in range(ng) if code in group_sets[g]) == groups
        assert {(mult, len(groups)) for _, _, _, mult, groups, _ in mine} >= {(m, s) for m in MULTS for s in range(ng + 1)}
        both = [pl for pl in mine if pl[5]]
        assert both and all(kmer_text(revcomp_code(c, k), k) in pivots[p].decode().split("N") and
                            kmer_text(c, k) in pivots[p].decode().split("N") for c, *_ in both)
        for cs in PLANT_CS:                                                  # every cell of the expected answer is non-zero
            want = oracle(seqs, group_of, pivots, k, pivot_cs=cs)
            assert (want["rows"] > 0).all() and (want["unique"] > 0).all(), cs
            assert set(counted(pivots[p], k, cs).values()) == {min(m, cs) for m in MULTS}
    assert sum(1 for t in seqs for w in t.decode().split("N") if not is_canonical(O.encode(w), k)) > 0   # genomes spell the other strand too


def summed(adds):
    row = [0.0] * 7
    for _, m, a in adds:
        for g in m:
            row[g] += a
    return row


@pytest.mark.parametrize("k", (ORDER_K, 21, 41))
def test_order_case_sums_differently_in_another_order(k):
    adds = order_addends(k)
    seqs, group_of, pivots = order_case()
    want = oracle(seqs, group_of, pivots, k)["rows"][0]
    sizes = {len(m) for _, m, _ in adds}
    assert sizes >= set(ORDER_SIZES) and 4_000 < len(pivots[0]) < 6_000
    assert min(sum(1 for _, m, _ in adds if g in m) for g in range(7)) >= 200
    assert [code for code, _, _ in adds] == sorted(code for code, _, _ in adds)
    fwd, rev = summed(adds), summed(reversed(adds))
    by_numpy = [float(np.sum(np.array([a for _, m, a in adds if g in m]))) for g in range(7)]
    assert fwd == want.tolist()
    assert any(r != w for r, w in zip(rev, want.tolist()))
    assert any(r != w for r, w in zip(by_numpy, want.tolist()))
    if k > 32:   # two-word keys: an order that compared the low 64-bit word first is another order, and another row
        low_first = sorted(adds, key=lambda t: (t[0] & (2 ** 64 - 1), t[0] >> 64))
        low_only = sorted(adds, key=lambda t: t[0] & (2 ** 64 - 1))
        assert [c for c, _, _ in low_first] != [c for c, _, _ in adds] and {c >> 64 for c, _, _ in adds} != {0}
        assert any(r != w for r, w in zip(summed(low_first), want.tolist()))
        assert any(r != w for r, w in zip(summed(low_only), want.tolist()))


def test_shape_cases_are_what_they_claim():
    seqs, group_of, pivots = shape_case("five_pivots")
    assert len(pivots[0]) < 9 and set(pivots[1]) == {ord("N")} and pivots[2] in [s for s, g in zip(seqs, group_of) if g == 1]
    assert len(pivots) == 5 and max(group_of) + 1 == 3 and len(shape_case("one_pivot")[2]) == 1
    assert shape_case("no_pivot")[2] == [] and max(shape_case("one_group")[1]) == 0
    seqs, group_of, pivots = shape_case("counter_widths")
    assert [group_of.count(g) for g in range(4)] == [1, 2, 17, 70] and [n.bit_length() for n in (1, 2, 17, 70)] == [1, 2, 5, 7]
    for name, ng in (("groups64", 64), ("groups65", 65)):
        seqs, group_of, pivots = shape_case(name)
        assert max(group_of) + 1 == ng and len(pivots) == 2
        assert (oracle(seqs, group_of, pivots, 9)["rows"][:, ng - 1] > 0).all()
    assert len(shape_case("pivots20")[2]) == 20 > 16 and len(shape_case("pivots6")[2]) == 6 > 4


GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "merge_lists.json")))["cases"]


@pytest.mark.parametrize("case", GOLD, ids=lambda c: f"k{c['k']}_n{c['num_datasets']}")
def test_confusion_from_rows_reproduces_the_reference_outputs(case):
    from khoice_amd import merge_lists as ML
    n, k = case["num_datasets"], case["k"]
    unions = [O.set_counts(O.union_sum([O.set_counts(O.count_records([g], k), 1) for g in gs], 5000), 1)
              for gs in case["rest_of_set"]]
    rows, uniques = zip(*[MO.confusion_row(O.count_records([p], k), unions) for p in case["pivots"]])
    assert ML.confusion_from_rows(rows, uniques, n, str(k)) == case["outputs"]
    assert ML.confusion_from_rows(np.array(rows), np.array(uniques, dtype=np.uint64), n, str(k)) == case["outputs"]
