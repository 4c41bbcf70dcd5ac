"""The presence-bitmap form of kh_exp1_run (k_bmp_build + k_bmp_readout, khoice_amd/csrc/kh_bmp.hip; taken for
k <= 12 when no set is requested) against the C restatement: within-group and across-group histograms and the distinct
counts, bit-exact, and from the statistics the proof that this form — and no other — did the work.

The planted inputs (range edges, slice edges, tile and split boundaries) are proven on the CPU by the unmarked tests
at the end: every planted code is canonical, lies where the case says it lies and occurs in exactly the genomes it
was meant for, so a green GPU run cannot be green by missing its target."""
import functools
import random

import numpy as np
import pytest

from khoice_amd import synth
from oracle import c_oracle as CO
from tests.util import random_dna, revcomp_np

TILE, SPLIT = 64, 192            # KHOICE_BMP_TILE_POS / KHOICE_BMP_SPLIT_POS of the text-edge cases: three tiles per split
EDGE_K = (5, 8, 12)
FIELDS = ("within_hist", "across_hist", "distinct_per_seq")


@pytest.fixture(scope="module")
def eng():
    from khoice_amd import build as kbuild
    from khoice_amd import engine as E
    kbuild.build_library()
    e = E.Engine(0)
    yield e
    e.close()


# ---------------------------------------------------------------- helpers
def kmer_text(code, k):
    return "".join("ACGT"[(code >> (2 * (k - 1 - i))) & 3] for i in range(k))


def revcomp_code(code, k):
    r = 0
    for _ in range(k):
        r = (r << 2) | (3 - (code & 3))
        code >>= 2
    return r


def canonical_codes(text, k):
    """The set of canonical k-mer codes of a text, in plain Python (any byte outside ACGTacgt breaks a run)."""
    val = {ord(c): i for i, c in enumerate("ACGT")}
    val.update({ord(c): i for i, c in enumerate("acgt")})
    out, fw, run, mask = set(), 0, 0, (1 << (2 * k)) - 1
    for b in text:
        if b not in val:
            run = 0
            continue
        fw = ((fw << 2) | val[b]) & mask
        run += 1
        if run >= k:
            out.add(min(fw, revcomp_code(fw, k)))
    return out


def deltas(st0, st1):
    d = {n: st1["kernels"][n]["launches"] - st0["kernels"][n]["launches"]
         for n in ("bmp_build", "bmp_readout", "union_tagged", "skm_union")}
    for n in ("retries", "builds", "bases", "kmers", "distinct", "setops", "setop_in", "setop_out"):
        d[n] = st1[n] - st0[n]
    return d


def run(eng, seqs, group_of, k, cs=5000, hist_len=5001, want=None, **kw):
    eng.profile(True)
    st0 = eng.stats()
    got = eng.exp1_run(seqs, group_of, k, cs=cs, hist_len=hist_len, **kw)
    st1 = eng.stats()
    eng.profile(False)
    if want is None:
        want = CO.exp1(seqs, group_of, k, cs=cs, hist_len=hist_len)
    for f in FIELDS:
        assert got[f].shape == want[f].shape and (got[f] == want[f]).all(), (f, k, cs, hist_len)
    return got, deltas(st0, st1)


def check(eng, seqs, group_of, k, cs=5000, hist_len=5001, want=None):
    """The oracle's answers, and the bitmap form alone did the work."""
    got, d = run(eng, seqs, group_of, k, cs, hist_len, want)
    assert d["bmp_build"] >= 1 and d["bmp_readout"] == 1, d
    assert d["union_tagged"] == 0 and d["skm_union"] == 0 and d["retries"] == 0, d
    assert d["builds"] == len(seqs), d
    return got, d


def species(n=20_000):
    items = synth.species_set(3, 3, n)
    return [t for _, _, t in items], [s - 1 for s, _, _ in items]


# ---------------------------------------------------------------- 1. every k
@pytest.mark.gpu
@pytest.mark.parametrize("k", range(1, 13))
def test_bmp_every_k(eng, k):
    seqs, group_of = species()
    want = CO.exp1(seqs, group_of, k)
    got1, d1 = check(eng, seqs, group_of, k, want=want)
    got2, d2 = check(eng, seqs, group_of, k, want=want)
    assert d1 == d2, (d1, d2)                                           # identical statistics, run after run
    assert d1["distinct"] == int(want["distinct_per_seq"].sum()) and d1["bases"] == sum(len(s) for s in seqs)
    assert d1["kmers"] == sum(valid_positions(s, k) for s in seqs)


def valid_positions(text, k):
    """k-mer positions of a text whose k bases are all ACGTacgt (numpy: a window sum over the break flags)."""
    a = np.frombuffer(text, dtype=np.uint8)
    if a.size < k:
        return 0
    ok = np.isin(a, np.frombuffer(b"ACGTacgt", dtype=np.uint8)).astype(np.int64)
    c = np.concatenate([[0], np.cumsum(ok)])
    return int(((c[k:] - c[:-k]) == k).sum())


# ---------------------------------------------------------------- 2. text edges
@functools.lru_cache(maxsize=None)
def edge_case(k):
    """The inputs of test_fused_edge_inputs at a few thousand bases, and genomes built around the tile and split
    boundaries of TILE / SPLIT.  meta: what the CPU test below proves about them."""
    rng = random.Random(70 + k)
    anc = random_dna(rng, 3_000)
    seqs = [
        anc.encode(),
        (anc[:1_500].lower() + "N" * 40 + anc[1_500:]).encode(),       # lower case, an N run
        b"ACGT",                                                        # shorter than k
        b"",                                                            # empty
        ("A" * 2_000 + "\n" + anc[:500]).encode(),                      # poly-A plus a second record
        (">x\n" + anc[::-1]).encode(),                                  # header bytes break runs
        random_dna(rng, 200).encode(),                                  # a 200-base genome
        b"N" * 500,                                                     # all N
        random_dna(rng, k).encode(),                                    # exactly k bases: one k-mer
        random_dna(rng, k - 1).encode(),                                # k - 1 bases: none
    ]
    meta = {"straddle": [], "breaks": []}
    km = [random_dna(rng, k) for _ in range(2)]
    # one k-mer, everything else N: it starts two positions before the tile boundary / its last base alone lies
    # behind the split boundary
    for kmer, start, boundary in ((km[0], TILE - 2, TILE), (km[1], SPLIT - (k - 1), SPLIT)):
        meta["straddle"].append((len(seqs), start, boundary, kmer))
        seqs.append(("N" * start + kmer + "N" * 10).encode())
    # a break byte at base index TILE / SPLIT exactly, bases on both sides of it
    for boundary in (TILE, SPLIT):
        meta["breaks"].append((len(seqs), boundary))
        seqs.append((random_dna(rng, boundary) + "N" + random_dna(rng, 50)).encode())
    meta["three_tiles_plus_one"] = (len(seqs), len(seqs) + 1)
    seqs.append(random_dna(rng, 3 * TILE + 1).encode())                 # three tiles plus one base
    seqs.append(random_dna(rng, 3 * TILE + k).encode())                 # three tiles plus one k-mer position
    group_of = [0, 0, 0, 1, 1, 2, 2, 3, 3, 3, 4, 4, 5, 5, 6, 6]
    assert len(group_of) == len(seqs)
    return seqs, group_of, meta


@pytest.fixture
def small_tiles(monkeypatch):
    monkeypatch.setenv("KHOICE_BMP_TILE_POS", str(TILE))
    monkeypatch.setenv("KHOICE_BMP_SPLIT_POS", str(SPLIT))


@pytest.mark.gpu
@pytest.mark.parametrize("k", EDGE_K)
def test_bmp_text_edges(eng, small_tiles, k):
    seqs, group_of, _ = edge_case(k)
    _, d = check(eng, seqs, group_of, k, cs=5000, hist_len=64)
    assert d["kmers"] == sum(valid_positions(s, k) for s in seqs)
    check(eng, seqs, group_of, k, cs=2, hist_len=64)                    # saturation of both counters
    check(eng, seqs, group_of, k, cs=5000, hist_len=3)                  # counters beyond the last bin
    check(eng, seqs, group_of, k, cs=2, hist_len=3)
    check(eng, [seqs[0]], [0], k)                                       # one genome in one group
    check(eng, [seqs[2][:min(4, k - 1)], seqs[3]], [0, 1], k)           # nothing to count at all


@pytest.mark.gpu
@pytest.mark.parametrize("k", EDGE_K)
def test_bmp_text_edges_default_tiles(eng, k):
    """The same inputs with the tile and split sizes the library chooses."""
    seqs, group_of, _ = edge_case(k)
    check(eng, seqs, group_of, k, cs=5000, hist_len=64)


# ---------------------------------------------------------------- 3. range edges
BLOCK_BITS = 16


@functools.lru_cache(maxsize=None)
def block_edge_codes(k):
    """First and last canonical code of every 2^16-code block of the 4^k code space: whatever power-of-two range
    of at least 2^16 codes a build workgroup owns, both ends of every range are among them."""
    out = []
    for b in range(4 ** k >> BLOCK_BITS):
        codes = np.arange(b << BLOCK_BITS, (b + 1) << BLOCK_BITS, dtype=np.uint64).reshape(-1, 1)
        canon = np.flatnonzero(codes[:, 0] <= revcomp_np(k, codes)[:, 0])
        out += [int(codes[canon[0], 0]), int(codes[canon[-1], 0])]
    return out


@functools.lru_cache(maxsize=None)
def range_case(k):
    """Every block-edge code as a record of its own (N between records) in a chosen subset of four genomes."""
    codes = block_edge_codes(k)
    subsets = [(i % 15) + 1 for i in range(len(codes))]                 # a non-empty 4-bit mask of genomes
    texts = [[] for _ in range(4)]
    for code, m in zip(codes, subsets):
        for g in range(4):
            if (m >> g) & 1:
                texts[g].append(kmer_text(code, k))
    seqs = ["N".join(t).encode() for t in texts]
    return seqs, [0, 0, 1, 1], codes, subsets


def planted_histograms(group_of, plants, cs, hist_len):
    """Expected answers when the k-mers of the input are exactly `plants` = [(code, set of genomes)], all distinct."""
    ng = max(group_of) + 1
    within = np.zeros((ng, hist_len), dtype=np.uint64)
    across = np.zeros(hist_len, dtype=np.uint64)
    distinct = np.zeros(len(group_of), dtype=np.uint64)
    for _, genomes in plants:
        per_group = {}
        for i in genomes:
            distinct[i] += 1
            per_group[group_of[i]] = per_group.get(group_of[i], 0) + 1
        for g, c in per_group.items():
            within[g, min(c, cs, hist_len - 1)] += 1
        across[min(len(per_group), cs, hist_len - 1)] += 1
    return {"within_hist": within, "across_hist": across, "distinct_per_seq": distinct}


@pytest.mark.gpu
@pytest.mark.parametrize("k", (11, 12))
def test_bmp_range_edges(eng, k):
    seqs, group_of, codes, subsets = range_case(k)
    got, _ = check(eng, seqs, group_of, k, hist_len=8)
    assert int(got["distinct_per_seq"].sum()) == sum(bin(m).count("1") for m in subsets)


# ---------------------------------------------------------------- 4. slice edges
SLICE_K = 7
GROUP_SIZES = (1, 2, 3, 4, 7, 8, 63, 64, 65)
GROUP_COUNTS = (1, 2, 64, 65, 130)
SATURATIONS = [(cs, hl) for cs in (1, 2, 3, 5000) for hl in (2, 3, 5001)]


@functools.lru_cache(maxsize=None)
def slice_codes():
    """Distinct canonical 7-mers in a seeded order."""
    codes = [c for c in range(4 ** SLICE_K) if c <= revcomp_code(c, SLICE_K)]
    random.Random(4).shuffle(codes)
    return codes


def edge_counts(n):
    """1, every 2^j - 1 and 2^j up to n, and n itself."""
    return sorted({1, n} | {v for j in range(1, 11) for v in ((1 << j) - 1, 1 << j) if v <= n})


def texts_of(plants, n):
    texts = [[] for _ in range(n)]
    for code, genomes in plants:
        for i in sorted(genomes):
            texts[i].append(kmer_text(code, SLICE_K))
    return ["N".join(t).encode() for t in texts]


@functools.lru_cache(maxsize=None)
def slice_case_genomes():
    """Groups of GROUP_SIZES genomes; per group one k-mer present in exactly c of its genomes for every edge count c."""
    pool = iter(slice_codes())
    group_of, plants = [], []
    for g, n in enumerate(GROUP_SIZES):
        first = len(group_of)
        group_of += [g] * n
        for j, c in enumerate(edge_counts(n)):
            plants.append((next(pool), frozenset(first + (3 * j + i) % n for i in range(c))))
    return texts_of(plants, len(group_of)), group_of, plants


@functools.lru_cache(maxsize=None)
def slice_case_groups(ngroups):
    """ngroups groups of one genome sharing k-mers present in exactly 1, 63, 64, 65 and all groups."""
    pool = iter(slice_codes())
    plants = []
    for j, c in enumerate(sorted({c for c in (1, 63, 64, 65, ngroups) if c <= ngroups})):
        plants.append((next(pool), frozenset((5 * j + i) % ngroups for i in range(c))))
    return texts_of(plants, ngroups), list(range(ngroups)), plants


@pytest.mark.gpu
@pytest.mark.parametrize("cs,hist_len", SATURATIONS)
def test_bmp_slice_edges_genomes(eng, cs, hist_len):
    seqs, group_of, _ = slice_case_genomes()
    check(eng, seqs, group_of, SLICE_K, cs=cs, hist_len=hist_len)


@pytest.mark.gpu
@pytest.mark.parametrize("cs,hist_len", SATURATIONS)
def test_bmp_slice_edges_groups(eng, cs, hist_len):
    for ngroups in GROUP_COUNTS:
        seqs, group_of, _ = slice_case_groups(ngroups)
        check(eng, seqs, group_of, SLICE_K, cs=cs, hist_len=hist_len)


# ---------------------------------------------------------------- 5. switches and declines
def not_taken(eng, seqs, group_of, k, want, key_arrays, **kw):
    got, d = run(eng, seqs, group_of, k, want=want, **kw)
    assert d["bmp_build"] == 0 and d["bmp_readout"] == 0, d
    if key_arrays:
        assert d["union_tagged"] > 0, d
    return got, d


@pytest.mark.gpu
def test_bmp_switches_and_declines(eng, monkeypatch):
    k = 9
    seqs, group_of = species()
    want = CO.exp1(seqs, group_of, k)
    check(eng, seqs, group_of, k, want=want)
    for name in ("KHOICE_NO_BMP", "KHOICE_NO_SKM"):
        monkeypatch.setenv(name, "1")
        not_taken(eng, seqs, group_of, k, want, True)
        monkeypatch.delenv(name)
    not_taken(eng, seqs, group_of, k, want, False, want_sets=True)      # emitted sets: the other forms
    not_taken(eng, seqs, group_of, k, want, False, want_across_set=True)
    monkeypatch.setenv("KHOICE_BMP_MAX_BYTES", "1")                     # the partial bitmaps do not fit: declined, not retried
    _, d = not_taken(eng, seqs, group_of, k, want, True)
    assert d["retries"] == 0, d
    monkeypatch.delenv("KHOICE_BMP_MAX_BYTES")
    check(eng, seqs, group_of, k, want=want)


@pytest.mark.gpu
def test_bmp_not_taken_above_its_range(eng):
    seqs, group_of = species()
    not_taken(eng, seqs, group_of, 13, None, True)


# ---------------------------------------------------------------- 6. preconditions, without a GPU
@pytest.mark.parametrize("k", EDGE_K)
def test_edge_case_lies_on_the_boundaries(k):
    seqs, group_of, meta = edge_case(k)
    assert TILE % 16 == 0 and SPLIT % TILE == 0 and SPLIT > TILE
    want = CO.exp1(seqs, group_of, k, hist_len=64)
    for i, start, boundary, kmer in meta["straddle"]:
        text = seqs[i].decode()
        assert text[start:start + k] == kmer and set(text[:start]) | set(text[start + k:]) == {"N"}
        assert start < boundary <= start + k - 1                        # it starts in front of the boundary and ends behind it
        assert start // boundary == 0 and (start + k - 1) // boundary == 1
        assert int(want["distinct_per_seq"][i]) == 1                    # the genome's only k-mer: missed -> a wrong count
    for i, boundary in meta["breaks"]:
        text = seqs[i].decode()
        assert text[boundary] == "N" and "N" not in text[:boundary] + text[boundary + 1:]
        assert boundary >= k and len(text) - boundary - 1 >= k          # k-mers on both sides of the break
        assert int(want["distinct_per_seq"][i]) == len(canonical_codes(seqs[i], k))
    a, b = meta["three_tiles_plus_one"]
    assert len(seqs[a]) == 3 * TILE + 1 and len(seqs[b]) - k + 1 == 3 * TILE + 1
    assert len(seqs[8]) == k and int(want["distinct_per_seq"][8]) == 1
    assert len(seqs[9]) == k - 1 and int(want["distinct_per_seq"][9]) == 0
    assert int(want["distinct_per_seq"][7]) == 0 and set(seqs[7]) == {ord("N")}


@pytest.mark.parametrize("k", (11, 12))
def test_range_case_holds_every_block_edge(k):
    seqs, group_of, codes, subsets = range_case(k)
    nblocks = 4 ** k >> BLOCK_BITS
    assert len(codes) == 2 * nblocks <= 512 and len(set(codes)) == len(codes)
    for b in range(nblocks):
        first, last = codes[2 * b], codes[2 * b + 1]
        lo, hi = b << BLOCK_BITS, ((b + 1) << BLOCK_BITS) - 1
        assert lo <= first < last <= hi
        for c in (first, last):
            assert c <= revcomp_code(c, k)                              # canonical
        # nothing canonical between the block's end and the code: scanned inward in plain Python
        assert all(c > revcomp_code(c, k) for c in range(lo, first))
        assert all(c > revcomp_code(c, k) for c in range(last + 1, hi + 1))
    assert codes[0] == 0 and kmer_text(codes[0], k) == "A" * k
    assert codes[-1] == max(c for c in range(4 ** k - (1 << BLOCK_BITS), 4 ** k) if c <= revcomp_code(c, k))
    for g in range(4):                                                  # every code in exactly the intended genomes
        assert canonical_codes(seqs[g], k) == {c for c, m in zip(codes, subsets) if (m >> g) & 1}
    plants = [(c, {g for g in range(4) if (m >> g) & 1}) for c, m in zip(codes, subsets)]
    want = CO.exp1(seqs, group_of, k, hist_len=8)
    mine = planted_histograms(group_of, plants, 5000, 8)
    for f in FIELDS:
        assert (want[f] == mine[f]).all(), f


def test_slice_cases_hold_every_count():
    k = SLICE_K
    seqs, group_of, plants = slice_case_genomes()
    assert [group_of.count(g) for g in range(len(GROUP_SIZES))] == list(GROUP_SIZES)
    assert len({c for c, _ in plants}) == len(plants) and all(c <= revcomp_code(c, k) for c, _ in plants)
    for g, n in enumerate(GROUP_SIZES):                                 # per group: exactly the edge counts, each once
        counts = sorted(len(gen) for _, gen in plants if group_of[min(gen)] == g)
        assert counts == edge_counts(n) and all({group_of[i] for i in gen} == {g} for _, gen in plants if group_of[min(gen)] == g)
    assert edge_counts(65) == [1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64, 65]
    for i in range(len(seqs)):
        assert canonical_codes(seqs[i], k) == {c for c, gen in plants if i in gen}
    for cs, hl in SATURATIONS:
        want = CO.exp1(seqs, group_of, k, cs=cs, hist_len=hl)
        mine = planted_histograms(group_of, plants, cs, hl)
        for f in FIELDS:
            assert (want[f] == mine[f]).all(), (f, cs, hl)
    for ngroups in GROUP_COUNTS:
        seqs, group_of, plants = slice_case_groups(ngroups)
        assert sorted(len(gen) for _, gen in plants) == sorted({c for c in (1, 63, 64, 65, ngroups) if c <= ngroups})
        assert all(c <= revcomp_code(c, k) for c, _ in plants)
        for i in range(ngroups):
            assert canonical_codes(seqs[i], k) == {c for c, gen in plants if i in gen}
        for cs, hl in SATURATIONS:
            want = CO.exp1(seqs, group_of, k, cs=cs, hist_len=hl)
            mine = planted_histograms(group_of, plants, cs, hl)
            for f in FIELDS:
                assert (want[f] == mine[f]).all(), (f, ngroups, cs, hl)
