"""kh_exp3_run (fused experiment type 3) against oracle/kmer_oracle.py: for every pivot (a read set) and every group
the `intersect -ocsum` histogram against the group's -cs union, and the distinct counts, bit-exact; and from the
statistics which form did the work: k_bmp_build + one k_bmp_cross per batch of pivots (kh_bmp.hip) for k <= 12, the set
operations inside the library otherwise.

The planted inputs (word, wave, range and bitmap edges; every count of every group for every pivot) and the walk cases
are proven on the CPU by tests/test_exp3_cpu.py."""
import functools
import os
import random
import shutil

import numpy as np
import pytest

from khoice_amd import synth
from oracle import kmer_oracle as O
from tests import test_gpu_exp2_bmp as X2      # edge_codes, kmer_text, revcomp_code, is_canonical, plain_set, related

TILE, SPLIT = X2.TILE, X2.SPLIT  # KHOICE_BMP_TILE_POS / KHOICE_BMP_SPLIT_POS: several tiles and splits per text, reads straddle both
PLANT_K = X2.PLANT_K
FIELDS = ("inter_hist", "distinct_per_seq", "distinct_per_pivot")
KERNELS = ("bmp_build", "bmp_cross", "bmp_pivot", "bmp_readout", "union_tagged", "skm_union", "setop")


@pytest.fixture(scope="module")
def eng():
    from khoice_amd import build as kbuild
    from khoice_amd import engine as E
    kbuild.build_library()
    e = E.Engine(0)
    yield e
    e.close()


# ---------------------------------------------------------------- the oracle's answer
def oracle(seqs, group_of, pivots, k, cs=5000, hist_len=5001):
    ng = max(group_of) + 1
    sets = [X2.plain_set(bytes(t), k) for t in seqs]                      # set_counts(build)
    psets = [X2.plain_set(bytes(t), k) for t in pivots]
    unions = [O.union_sum([s for s, g in zip(sets, group_of) if g == h], cs) for h in range(ng)]
    want = {"inter_hist": np.zeros((len(pivots), ng, hist_len), dtype=np.uint64),
            "distinct_per_seq": np.array([len(s) for s in sets], dtype=np.uint64),
            "distinct_per_pivot": np.array([len(s) for s in psets], dtype=np.uint64)}
    for p, ps in enumerate(psets):
        for g in range(ng):
            want["inter_hist"][p, g] = O.histogram(O.intersect(ps, unions[g], "sum", cs), hist_len - 1)
    return want


def deltas(st0, st1):
    d = {n: st1["kernels"][n]["launches"] - st0["kernels"][n]["launches"] for n in KERNELS}
    for n in ("retries", "builds", "bases", "kmers", "distinct", "setops", "setop_in", "setop_out", "text_packed"):
        d[n] = st1[n] - st0[n]
    return d


def run(eng, seqs, group_of, pivots, k, cs=5000, hist_len=5001, want=None, texts=None):
    eng.profile(True)
    st0 = eng.stats()
    a, b = texts if texts else (seqs, pivots)
    got = eng.exp3_run(a, group_of, b, k, cs=cs, hist_len=hist_len)
    st1 = eng.stats()
    eng.profile(False)
    if want is None:
        want = oracle(seqs, group_of, pivots, k, cs, hist_len)
    for f in FIELDS:
        assert got[f].shape == want[f].shape, (f, k, cs, hist_len)
        assert (got[f] == want[f]).all(), (f, k, cs, hist_len, np.argwhere(got[f] != want[f])[:8].tolist())
    return got, deltas(st0, st1)


def check(eng, seqs, group_of, pivots, k, cs=5000, hist_len=5001, want=None, batches=1, texts=None):
    """The oracle's answers, and the bitmap form alone did the work, in `batches` launches."""
    got, d = run(eng, seqs, group_of, pivots, k, cs, hist_len, want, texts)
    assert d["bmp_build"] >= 1 and d["bmp_cross"] == batches, d
    assert d["bmp_pivot"] == 0 and d["bmp_readout"] == 0 and d["setop"] == 0, d
    assert d["union_tagged"] == 0 and d["skm_union"] == 0 and d["retries"] == 0, d
    assert d["builds"] == len(seqs) + len(pivots), d
    return got, d


def by_sets(eng, seqs, group_of, pivots, k, **kw):
    got, d = run(eng, seqs, group_of, pivots, k, **kw)
    assert d["bmp_build"] == 0 and d["bmp_cross"] == 0 and d["bmp_pivot"] == 0 and d["bmp_readout"] == 0, d
    assert d["setop"] > 0, d
    return got, d


def same(a, b):
    return all(a[f].shape == b[f].shape and (a[f] == b[f]).all() for f in FIELDS)


def read_text(codes, n_reads, read_len, error_rate, seed, min_len=None):
    return b"\n".join(synth.simulated_reads(codes, n_reads, read_len, error_rate, seed, min_len))


@functools.lru_cache(maxsize=None)
def species(n=20_000):
    """3 groups x 3 genomes; 6 pivots: per group a short-read set and a long-read set of a fourth genome of it."""
    items = synth.species_set(3, 3, n)
    pivots = []
    for s in (1, 2, 3):
        codes = synth.genome_codes(s, 3, n, synth.ancestor(s, n))
        pivots.append(read_text(codes, 40, 150, 0.002, 10 * s))
        pivots.append(read_text(codes, 12, 3000, 0.05, 10 * s + 1, min_len=200))
    return [t for _, _, t in items], [s - 1 for s, _, _ in items], pivots


# ---------------------------------------------------------------- 1. every k
@pytest.mark.gpu
@pytest.mark.parametrize("k", range(1, 13))
def test_exp3_every_k(eng, k):
    seqs, group_of, pivots = species()
    want = oracle(seqs, group_of, pivots, k)
    got1, d1 = check(eng, seqs, group_of, pivots, k, want=want)
    got2, d2 = check(eng, seqs, group_of, pivots, k, want=want)
    assert same(got1, got2) and d1 == d2, (d1, d2)
    assert d1["bases"] == sum(len(s) for s in seqs + pivots)
    assert d1["distinct"] == int(want["distinct_per_seq"].sum() + want["distinct_per_pivot"].sum())


# ---------------------------------------------------------------- 2. read-shaped pivots
@pytest.fixture
def small_tiles(monkeypatch):
    monkeypatch.setenv("KHOICE_BMP_TILE_POS", str(TILE))
    monkeypatch.setenv("KHOICE_BMP_SPLIT_POS", str(SPLIT))


@functools.lru_cache(maxsize=None)
def read_shaped_case(k, n=2_000):
    """Genomes of 3 groups x 2 and the pivots the issue names; returns seqs, group_of, pivots, names."""
    rng = np.random.default_rng(300 + k)
    fam = [X2.related(rng, 3, n) for _ in range(3)]
    seqs = [t for f in fam for t in f[:2]]
    group_of = [0, 0, 1, 1, 2, 2]
    src = fam[0][2]
    recs = [src[100:100 + k - 1], src[200:200 + k], src[300:300 + k + 1], b"", b"N" * (k + 3),
            src[400:400 + 3 * k].lower(), src[500:500 + 150]]
    codes = np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), np.frombuffer(fam[1][2], dtype=np.uint8)).astype(np.uint8)
    reads = read_text(codes, 30, 150, 0.01, 7)
    pivots = {"edge_records": b"\n".join(recs), "empty": b"", "shorter_than_k": src[:k - 1] if k > 1 else b"N",
              "a_genome": seqs[2], "reads": reads}
    return seqs, group_of, list(pivots.values()), list(pivots)


@pytest.mark.gpu
@pytest.mark.parametrize("k", (4, 9, 12))
def test_exp3_read_shaped_pivots(eng, small_tiles, k):
    seqs, group_of, pivots, names = read_shaped_case(k)
    got, _ = check(eng, seqs, group_of, pivots, k)
    assert got["distinct_per_pivot"][names.index("empty")] == 0 and got["distinct_per_pivot"][names.index("shorter_than_k")] == 0
    assert (got["inter_hist"][names.index("empty")] == 0).all()
    p = names.index("a_genome")                                           # identical to a genome of group 1: every k-mer of it is met there
    assert got["inter_hist"][p, 1].sum() == got["distinct_per_pivot"][p] == got["distinct_per_seq"][2] > 0
    none, d = check(eng, seqs, group_of, [], k)                           # no pivots: one launch for the genomes' counters
    assert none["inter_hist"].shape == (0, 3, 5001) and (none["distinct_per_seq"] == got["distinct_per_seq"]).all()


# ---------------------------------------------------------------- 3. planted codes at every edge
PLANT_SIZES = (3, 1, 2)          # genomes per group
PLANT_PIVOT_SETS = ((0, 1, 2, 3), (0,), (1,), (2,), (3,), (0, 2), (1, 3), ())   # (): held by groups and no pivot
PLANT_VECTORS = ((0, 0, 0), (1, 1, 1), (2, 0, 2), (3, 1, 0), (0, 1, 2), (1, 0, 1))   # genomes of every group that hold the code
PLANT_ROUNDS = 4                 # codes per kind at least: texts of several splits


@functools.lru_cache(maxsize=None)
def planted_case(k):
    """Texts made of chosen canonical codes, every code a record of its own.  A plant is (code, pivots, vector, genomes,
    rc, what): the code is held by the pivots of the set and by vector[g] genomes of group g; rc: the genomes spell the
    reverse complement.  (0, 0, 0) with pivots: held by pivots and no group; () with a vector: by groups and no pivot.
    The edge codes (tests/test_gpu_exp2_bmp.py: edge_codes) go to the kinds in turn, the rest is filled from a seeded
    pool.  The first pivot set holds every vector, so every (pivot, group, v) is planted: v = 0 .. size.
    Returns seqs, group_of, pivots, plants."""
    ng = len(PLANT_SIZES)
    group_of = [g for g, n in enumerate(PLANT_SIZES) for _ in range(n)]
    first = [group_of.index(g) for g in range(ng)]
    kinds = [(ps, vec) for ps in PLANT_PIVOT_SETS for vec in PLANT_VECTORS if ps or any(vec)]
    edges = X2.edge_codes(k)
    rng = random.Random(1300 + k)
    used = set(edges.values())

    def fresh():
        while True:
            c = rng.randrange(4 ** k)
            if X2.is_canonical(c, k) and c != X2.revcomp_code(c, k) and c not in used:
                used.add(c)
                return c

    rng.shuffle(kinds)
    todo = sorted(edges.items())
    plants = []
    i = 0
    while todo or i < PLANT_ROUNDS * len(kinds):
        ps, vec = kinds[i % len(kinds)]
        i += 1
        what, code = todo.pop() if todo else ("fill", fresh())
        rc = i % 3 == 0 and code != X2.revcomp_code(code, k)
        genomes = tuple(first[g] + (i + j) % PLANT_SIZES[g] for g in range(ng) for j in range(vec[g]))
        plants.append((code, ps, vec, genomes, rc, what))
    texts = [[] for _ in group_of]
    ptexts = [[] for _ in range(4)]
    for code, ps, vec, genomes, rc, _ in plants:
        for p in ps:
            ptexts[p].append(X2.kmer_text(code, k))
        for gi in genomes:
            texts[gi].append(X2.kmer_text(X2.revcomp_code(code, k) if rc else code, k))
    return ["N".join(t).encode() for t in texts], group_of, ["\n".join(t).encode() for t in ptexts], plants


def planted_answer(k, cs=5000, hist_len=5001):
    """The expected outputs worked out from the plants alone; occ[p][g][v], v = 0 .. size."""
    seqs, group_of, pivots, plants = planted_case(k)
    ng = len(PLANT_SIZES)
    occ = [[[0] * (n + 1) for n in PLANT_SIZES] for _ in pivots]
    dseq, dpiv = [0] * len(seqs), [0] * len(pivots)
    for code, ps, vec, genomes, rc, _ in plants:
        for gi in genomes:
            dseq[gi] += 1
        for p in ps:
            dpiv[p] += 1
            for g in range(ng):
                occ[p][g][vec[g]] += 1
    want = {"inter_hist": np.zeros((len(pivots), ng, hist_len), dtype=np.uint64),
            "distinct_per_seq": np.array(dseq, dtype=np.uint64), "distinct_per_pivot": np.array(dpiv, dtype=np.uint64)}
    for p in range(len(pivots)):
        for g in range(ng):
            for v in range(1, PLANT_SIZES[g] + 1):
                want["inter_hist"][p, g, min(1 + min(v, cs), cs, hist_len - 1)] += occ[p][g][v]
    return want, occ


@pytest.mark.gpu
@pytest.mark.parametrize("k", PLANT_K)
def test_exp3_planted_edges(eng, small_tiles, k):
    seqs, group_of, pivots, _ = planted_case(k)
    want, _ = planted_answer(k)
    check(eng, seqs, group_of, pivots, k, want=want)


# ---------------------------------------------------------------- 4. walk edges
WALK_SIZES = (1, 3, 4, 17, 33)   # counters of 1, 2, 3, 5 and 6 slices; 58 genomes


@functools.lru_cache(maxsize=None)
def walk_case(npiv, length=1_500):
    """Groups of 1, 3, 4, 17 and 33 related genomes and npiv pivots (reads of a further genome of the groups in turn):
    the operands of the launch are the pivots, then the 58 genomes, taken 16 (k <= 10) or 4 (k = 11) to a round."""
    rng = np.random.default_rng(40 + npiv)
    fam = [X2.related(rng, n + 1, length) for n in WALK_SIZES]
    seqs = [t for f, n in zip(fam, WALK_SIZES) for t in f[:n]]
    group_of = [g for g, n in enumerate(WALK_SIZES) for _ in range(n)]
    pivots = []
    for p in range(npiv):
        t = fam[p % len(fam)][-1]
        at = [int(x) for x in rng.integers(0, length - 150, 6)]
        pivots.append(b"\n".join(t[a:a + 150] for a in at))
    return seqs, group_of, pivots


@pytest.mark.gpu
@pytest.mark.parametrize("npiv,k", [(6, 9), (7, 9), (15, 9), (6, 11), (5, 11)])
def test_exp3_walk_edges(eng, npiv, k):
    """58 + 6 = 64 operands: a multiple of 16 and of 4; 58 + 7, 58 + 15 and 58 + 5 are not.  With 6 or 7 pivots the first
    round of 16 holds pivots and the genomes of groups 0, 1 and 2 together; 15 pivots: the single genome of group 0 closes
    the first round; the groups of 17 and 33 span rounds."""
    seqs, group_of, pivots = walk_case(npiv)
    got, _ = check(eng, seqs, group_of, pivots, k)
    assert got["inter_hist"][:, 3, 2:19].sum() > 0 and got["inter_hist"][:, 4, 18:35].sum() > 0   # counts that need 5 and 6 slices


# ---------------------------------------------------------------- 5. pivot batches
@pytest.mark.gpu
def test_exp3_pivot_batches(eng, monkeypatch):
    k = 9
    seqs, group_of, pivots = species(8_000)
    pivots = pivots + [pivots[0] + b"\n" + pivots[3]]                     # 7 pivots, 9 genomes
    want = oracle(seqs, group_of, pivots, k)
    one, _ = check(eng, seqs, group_of, pivots, k, want=want)
    monkeypatch.setenv("KHOICE_BMP_MAX_BINS", "40")                       # (40 - 9) // (9 + 1) = 3 pivots a launch: 3 + 3 + 1
    three, d = check(eng, seqs, group_of, pivots, k, want=want, batches=3)
    assert same(one, three)
    monkeypatch.setenv("KHOICE_BMP_MAX_BINS", "18")                       # one pivot: 9 bins + 1 + 9 counters = 19
    sets, d = by_sets(eng, seqs, group_of, pivots, k, want=want)
    assert d["retries"] == 0 and same(one, sets), d
    monkeypatch.setenv("KHOICE_BMP_MAX_BINS", "19")
    check(eng, seqs, group_of, pivots, k, want=want, batches=7)


# ---------------------------------------------------------------- 6. clamps
@pytest.mark.gpu
@pytest.mark.parametrize("cs", (1, 2, 5000))
@pytest.mark.parametrize("hist_len", (2, 3, 5001))
def test_exp3_clamps(eng, cs, hist_len):
    seqs, group_of, pivots = species()
    check(eng, seqs, group_of, pivots, 10, cs=cs, hist_len=hist_len)


# ---------------------------------------------------------------- 7. the forms agree, declining, arguments
@pytest.mark.gpu
def test_exp3_forms_agree(eng, monkeypatch):
    k = 8
    case = species(8_000)
    want = oracle(*case, k)
    got, _ = check(eng, *case, k, want=want)
    monkeypatch.setenv("KHOICE_NO_BMP", "1")
    other, _ = by_sets(eng, *case, k, want=want)
    monkeypatch.delenv("KHOICE_NO_BMP")
    assert same(got, other)
    monkeypatch.setenv("KHOICE_BMP_MAX_BYTES", "1")                       # the bitmaps do not fit: declined, not retried
    _, d = by_sets(eng, *case, k, want=want)
    assert d["retries"] == 0, d
    monkeypatch.delenv("KHOICE_BMP_MAX_BYTES")
    check(eng, *case, k, want=want)
    monkeypatch.setenv("KHOICE_NO_BMP", "1")                              # the set form's own corners: texts without k-mers, no pivot
    seqs, group_of, pivots, _ = read_shaped_case(9)
    by_sets(eng, seqs, group_of, pivots, 9)
    none, d = run(eng, seqs, group_of, [], 9)
    assert d["bmp_build"] == 0 and d["builds"] == len(seqs) and none["inter_hist"].shape == (0, 3, 5001), d


@pytest.mark.gpu
@pytest.mark.parametrize("k", (13, 21))
def test_exp3_set_form_above_the_bitmaps(eng, k):
    by_sets(eng, *species(8_000), k)


@pytest.mark.gpu
def test_exp3_bad_arguments(eng):
    from khoice_amd import engine as E
    seqs, group_of, pivots = species(8_000)
    bad = [dict(group_of=[0, 0, 0, 1, 1, 1, 2, 2, -1]),                   # a group outside [0, ngroups)
           dict(group_of=[0, 0, 0, 0, 0, 0, 2, 2, 2]),                    # a group without a genome
           dict(hist_len=1), dict(k=0), dict(k=65), dict(cs=0)]
    for change in bad:
        args = dict(seqs=seqs, group_of=group_of, pivots=pivots, k=9, hist_len=5001)
        args.update(change)
        with pytest.raises(E.KhoiceError) as ei:
            eng.exp3_run(**args)
        assert ei.value.code == -1, change                                # KH_E_ARG
        assert len(str(ei.value)) > len("khoice_hip error -1: "), change  # with a message from kh_last_error
    check(eng, seqs, group_of, pivots, 9)                                 # and the context still works


# ---------------------------------------------------------------- 8. device-resident texts
@pytest.mark.gpu
def test_exp3_device_texts(eng, tmp_path):
    from khoice_amd.workflow import exp_type_3 as W3
    k, n = 9, 3
    root = str(tmp_path)
    synth.write_type3_tree(root, n, 2, 3000, 40)
    paths, group_of = [], []
    for num in range(1, n + 1):
        for g in W3.rest_of_set(root, num):
            paths.append(os.path.join(root, f"input_type3/rest_of_set/dataset_{num}/{g}.fna.gz"))
            group_of.append(num - 1)
    ppaths = [os.path.join(root, W3.reads_path(rt, num)) for rt in W3.READ_TYPES for num in range(1, n + 1)]
    host = [eng.read_fasta(p) for p in paths + ppaths]
    seqs, pivots = host[:len(paths)], host[len(paths):]
    want = oracle(seqs, group_of, pivots, k)
    got, hd = check(eng, seqs, group_of, pivots, k, want=want)
    texts = eng.ingest_fasta(paths + ppaths)
    try:
        assert all(ptr % 16 == 0 and ln == len(t) for (ptr, ln), t in zip(texts.seqs, host))
        dev, dd = check(eng, seqs, group_of, pivots, k, want=want, texts=(texts.seqs[:len(paths)], texts.seqs[len(paths):]))
    finally:
        texts.free()
    assert same(got, dev)
    assert hd["text_packed"] == sum(len(t) for t in host) and dd["text_packed"] == 0, (hd, dd)
    with pytest.raises(ValueError):
        eng.exp3_run(seqs, group_of, [(0, 0)], k)


# ---------------------------------------------------------------- 9. workflow
def tree_files(root):
    out = {}
    for top in ("genome_sets_type3/pivot", "within_dataset_results_type3", "final_analysis_type3"):
        for d, _, names in os.walk(os.path.join(root, top)):
            for name in names:
                if name.endswith((".hist.txt", ".csv")):
                    out[os.path.relpath(os.path.join(d, name), root)] = open(os.path.join(d, name)).read()
    return out


@pytest.mark.gpu
def test_exp3_workflow_three_runners(tmp_path, monkeypatch):
    """The rule runner goes through bin/kmc and bin/kmc_tools as clients of one resident bin/khoice_server: 138 rule
    processes, none of which pays a HIP initialisation of its own."""
    import subprocess
    from khoice_amd import build as kbuild
    from khoice_amd.workflow import exp_type_3 as W3
    from tests.test_exp3_cpu import expected_type3_outputs
    kbuild.build_clis()
    ks, n = [9, 21], 3
    roots = [str(tmp_path / name) for name in ("rules", "batched", "fused")]
    os.makedirs(roots[0])
    synth.write_type3_tree(roots[0], n, 2, 3000, 40)
    for r in roots[1:]:
        shutil.copytree(roots[0], r)
    server = os.path.join(W3.REPO_BIN, "khoice_server")
    sock = str(tmp_path / "khoice.sock")
    srv = subprocess.Popen([server, sock], stderr=subprocess.PIPE, text=True)
    try:
        assert "ready on" in srv.stderr.readline()                          # printed behind listen()
        monkeypatch.setenv("KHOICE_SERVER", sock)
        by_rules = W3.run(roots[0], ks, n)
    finally:
        subprocess.run([server, "--stop", sock], timeout=30)
        srv.wait(timeout=30)
    monkeypatch.delenv("KHOICE_SERVER")
    assert f"served {by_rules['processes'] + 1} requests" in srv.stderr.read()   # every rule, and the shutdown
    outs = [by_rules, W3.run_batched(roots[1], ks, n), W3.run_fused(roots[2], ks, n)]
    files, csv = expected_type3_outputs(roots[0], ks, n)
    files["final_analysis_type3/final_analysis_type3.csv"] = csv
    assert len(files) == 2 * n * len(ks) * (1 + n) + 1
    for r, out in zip(roots, outs):
        assert tree_files(r) == files, r
        assert out["csv"] == csv
    assert outs[0]["processes"] == len(ks) * (n * (2 * 2 + 1) + 2 * n * (3 + 2 * n)) and outs[1]["processes"] == outs[2]["processes"] == 0
