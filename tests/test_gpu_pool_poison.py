"""Every form of the library on poisoned pool memory (KHOICE_DEBUG_POISON, kh_ctx::buf_alloc / pin_alloc in
khoice_amd/csrc/kh_engine.cpp): whatever a block of the caching allocator held before, fresh or recycled, device or
pinned, the answers are the oracle's, bit for bit, and the kernels that ran are the ones that run on clean memory.

Every entry of the battery is run once without the knob and once per pattern with it, on one module-scoped engine:
  - every output equals the oracle's (oracle/c_oracle.py, oracle/kmer_oracle.py, oracle/merge_oracle.py) and the output
    of the run without the knob;
  - `poisoned_bytes` grew under the knob and stayed where it was without it;
  - the kernel launches, `retries`, `big_slots` and `order_fallbacks` are those of the run without the knob, and the
    form the entry is named after is the one that ran (`expect`).
Patterns: 0x00 (the state the rest of the suite runs in), 0x41 'A' and 0x63 'c' (valid bases: a text reader that looks
behind `len` counts k-mers that are not there), 0xFF (the hash sets' EMPTY key, the largest cursor, an invalid base).

The witnesses.  Every text input ends with TAILS, in a group (and as pivots) of their own, so they are the last texts
of every packed copy: T x 69 and G x 85 (len % 16 != 0: the bytes up to the next text's 16-byte boundary are the
block's), and last G x 80 (len % 16 == 0: the 256 bytes behind it are).  Each is one run of valid bases, and the
oracle's distinct count of `text + p * 32` differs from that of `text` for p = 'A' and p = 'c' at every k >= 2.  At
k = 1 a text holds A/T or C/G, so no text can show both letters: T x 69 shows 'c', the two G texts show 'A'.  The
unmarked tests at the end prove this on the oracle alone, for every entry and every k it uses.

Beside the battery: the knob is read at every allocation and ignores what is no byte value; the fill is really in
the block, and in front of the block's first writer (the bytes behind a resident text); and one engine without the
knob runs a super-k-mer, a bitmap and a key-array call in turn and in reverse, each on blocks the other forms left."""
import atexit
import functools
import gzip
import os
import shutil
import tempfile

import numpy as np
import pytest

from khoice_amd import synth
from oracle import c_oracle as CO
from oracle import kmer_oracle as O
from oracle import merge_oracle as MO
from tests import test_gpu_bmp as X1
from tests import test_gpu_exp2_bmp as X2
from tests import test_gpu_exp3 as X3
from tests import test_gpu_exp4 as X4
from tests import test_gpu_exp_set_forms as XF
from tests import test_gpu_skm_scatter as XS
from tests import test_gpu_views_tables as XV
from tests.util import db_to_arrays, set_to_db, unmix_np, words

PATTERNS = (0x00, 0x41, 0x63, 0xFF)
LETTERS = (0x41, 0x63)
TAILS = (b"T" * 69, b"G" * 85, b"G" * 80)
COUNTERS = ("retries", "big_slots", "order_fallbacks")
BMP_EDGES = {"KHOICE_BMP_TILE_POS": "64", "KHOICE_BMP_SPLIT_POS": "192"}
NO_SKM = {"KHOICE_NO_SKM": "1"}


@pytest.fixture(scope="module")
def eng():
    import torch
    from khoice_amd import build as kbuild
    from khoice_amd import engine as E
    kbuild.build_library()
    torch.cuda.init()
    e = E.Engine(0)
    yield e
    e.close()


# ---------------------------------------------------------------- inputs
def tailed(seqs, group_of):
    """The case with TAILS behind it, in a group of their own."""
    return list(seqs) + list(TAILS), list(group_of) + [max(group_of) + 1] * len(TAILS)


@functools.lru_cache(maxsize=None)
def species(ns, ng, n):
    items = synth.species_set(ns, ng, n)
    return tailed([t for _, _, t in items], [s - 1 for s, _, _ in items])


@functools.lru_cache(maxsize=None)
def stress():
    return tailed(*XS.stress_set())


@functools.lru_cache(maxsize=None)
def big_group():
    return tailed(*XF.two_pass_case())


@functools.lru_cache(maxsize=None)
def pivot_case(kind, n):
    """species(n) of the module of experiment type `kind`, TAILS behind the genomes and behind the pivots."""
    case = {2: X2, 3: X3, 4: X4}[kind].species(n)
    seqs, group_of = tailed(case[0], case[1])
    pivots = list(case[2]) + list(TAILS)
    if kind == 2:
        return seqs, group_of, pivots, list(case[3]) + [group_of[-1]] * len(TAILS)
    return seqs, group_of, pivots


# ---------------------------------------------------------------- the battery
class Entry:
    """call(eng) -> {name: array, dict or bytes}; want() -> the oracle's values of (a subset of) them; texts: every
    text the call hands to the library, in packing order; ks: every k it runs at; expect(d): what the launch counts
    of the form look like."""

    def __init__(self, call, want, texts, ks, env=None, expect=None):
        self.call, self.want, self.texts, self.ks, self.env, self.expect = call, want, texts, ks, env or {}, expect


BATTERY = {}


def sets_of(kset):
    keys, counts = kset.download_sorted()
    return {"keys": keys, "counts": counts}


def group_union(seqs, k, cs):
    return CO.union_sum([CO.count(s, k).set_counts(1) for s in seqs], cs)


def add_exp1(name, case, k, env=None, expect=None, want_sets=False, want_across_set=False):
    def call(eng):
        seqs, group_of = case()
        r = eng.exp1_run(seqs, group_of, k, want_sets=want_sets, want_across_set=want_across_set)
        out = {f: r[f] for f in X1.FIELDS}
        for g, s in enumerate(r.get("group_sets", [])):
            out[f"group_set{g}"] = sets_of(s)
        if "across_set" in r:
            out["across_set"] = sets_of(r["across_set"])
        return out

    def want():
        seqs, group_of = case()
        w = CO.exp1(seqs, group_of, k)
        out = {f: w[f] for f in X1.FIELDS}
        ng = max(group_of) + 1
        unions = [group_union([s for s, h in zip(seqs, group_of) if h == g], k, 5000) for g in range(ng)]
        if want_sets:
            for g, u in enumerate(unions):
                out[f"group_set{g}"] = dict(zip(("keys", "counts"), u.arrays()))
        if want_sets or want_across_set:
            out["across_set"] = dict(zip(("keys", "counts"), CO.union_sum([u.set_counts(1) for u in unions], 5000).arrays()))
        return out

    BATTERY[name] = Entry(call, want, lambda: case()[0], (k,), env, expect)


def skm_only(d):
    assert d["skm_union"] == 1 and d["union_tagged"] == 0 and d["retries"] == 0 and d["bmp_build"] == 0, d


def skm_big(d):
    assert d["skm_union"] >= 1 and d["skm_big"] >= 1 and d["big_slots"] > 0 and d["retries"] == 0, d


def skm_any(d):
    assert d["skm_scatter"] >= 1 and d["union_tagged"] == 0 and d["retries"] == 0 and d["bmp_build"] == 0, d


def key_arrays(d):
    assert d["union_tagged"] >= 1 and d["skm_union"] == 0 and d["bmp_build"] == 0 and d["retries"] == 0, d


def bitmaps(d):
    assert d["bmp_build"] >= 1 and d["skm_union"] == 0 and d["union_tagged"] == 0 and d["setop"] == 0 and d["retries"] == 0, d


def set_form(d):
    assert d["bmp_build"] == 0 and d["setop"] > 0 and d["retries"] == 0, d


# ---- key arrays
def add_build(k):
    case = functools.partial(species, 2, 2, 5_000)

    def call(eng):
        return {f"set{i}": sets_of(s) for i, s in enumerate(eng.build_batch(case()[0], k))}

    def want():
        return {f"set{i}": dict(zip(("keys", "counts"), CO.count(s, k).arrays())) for i, s in enumerate(case()[0])}

    BATTERY[f"build_counts_k{k}"] = Entry(call, want, lambda: case()[0], (k,), None,
                                          lambda d: d["bucket_sort_rle"] >= 1 and d["retries"] == 0 or pytest.fail(str(d)))


for _k in (13, 16, 32, 33, 64):
    add_build(_k)
for _k in (15, 64):
    add_exp1(f"exp1_want_sets_k{_k}", functools.partial(species, 3, 2, 4_000), _k, want_sets=True)
    add_exp1(f"exp1_want_across_set_k{_k}", functools.partial(species, 3, 2, 4_000), _k, want_across_set=True)
add_exp1("tagged_union_k31", functools.partial(species, 3, 3, 8_000), 31, NO_SKM, key_arrays)
add_exp1("tagged_union_k31_fine_bins", functools.partial(species, 3, 3, 8_000), 31, dict(NO_SKM, KHOICE_NO_UNION_HASH="1"),
         key_arrays)

SETS_K = 21
SMALL = functools.partial(species, 1, 3, 3_000)       # three related genomes, then TAILS


def small_dbs(k, cs=255):
    return [O.build(X4.fasta_of(t), k, cs=cs) for t in SMALL()[0]]


def setops_call(eng):
    s = eng.build_batch(SMALL()[0], SETS_K)
    u, hist = eng.union_sum(s[:3], 5000, hist_len=64)
    return {"union": set_to_db(u), "union_hist": hist, "histogram": eng.union_histogram(s[:3] + s[5:], 300, 64),
            "intersect": set_to_db(eng.intersect(s[0], s[1], "sum", cs=5000)),
            "subtract": set_to_db(eng.kmers_subtract(s[0], s[2])), "subtract_tail": set_to_db(eng.kmers_subtract(s[4], s[5]))}


def setops_want():
    d = small_dbs(SETS_K)
    u = O.union_sum(d[:3], 5000)
    return {"union": u, "union_hist": np.array(O.histogram(u, 63), dtype=np.uint64),
            "histogram": np.array(O.histogram(O.union_sum(d[:3] + d[5:], 300), 63), dtype=np.uint64),
            "intersect": O.intersect(d[0], d[1], "sum", 5000), "subtract": O.kmers_subtract(d[0], d[2]),
            "subtract_tail": O.kmers_subtract(d[4], d[5])}


BATTERY["set_operations"] = Entry(setops_call, setops_want, lambda: SMALL()[0], (SETS_K,), None,
                                  lambda d: d["setop"] >= 5 and d["retries"] == 0 or pytest.fail(str(d)))


def member_call(eng):
    texts = SMALL()[0]
    pivot = eng.build(texts[0], SETS_K)
    sets = [s.set_counts(1) for s in eng.build_batch(texts[1:], SETS_K, with_counts=False)]
    keys, counts, masks = eng.membership(pivot, sets)
    row, uniq = eng.confusion_row(pivot, sets)
    return {"keys": keys, "counts": counts, "masks": masks, "row": row, "unique": uniq}


def member_want():
    d = small_dbs(SETS_K)
    keys, counts = db_to_arrays(d[0], SETS_K)
    masks = np.array([[sum(1 << j for j, s in enumerate(d[1:]) if c in s)] for c in sorted(d[0])], dtype=np.uint64)
    row, uniq = MO.confusion_row(d[0], d[1:])
    return {"keys": keys, "counts": counts, "masks": masks, "row": np.array(row, dtype=np.float64), "unique": uniq}


BATTERY["membership_confusion_row"] = Entry(member_call, member_want, lambda: SMALL()[0], (SETS_K,))

TABLE_K = 8


def table_call(eng):
    import torch
    table = torch.zeros(4 ** TABLE_K, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    for s in eng.build_batch(SMALL()[0], TABLE_K):
        eng.table_add_set(s, table.data_ptr(), 4)
    hist = eng.table_histogram(table.data_ptr(), 4, 0, 4 ** TABLE_K, 5000, 64)
    part = eng.table_histogram(table.data_ptr(), 4, 16 * 37, 4 ** TABLE_K - 5, 2, 3)
    eng.sync()
    return {"hist": hist, "part": part, "cells": table.cpu().numpy().astype(np.int64)}


def table_want():
    cells = np.zeros(4 ** TABLE_K, dtype=np.int64)
    for d in small_dbs(TABLE_K):
        cells[sorted(d)] += 1
    return {"hist": XV.ref_table_hist(cells, 5000, 64), "part": XV.ref_table_hist(cells[16 * 37:4 ** TABLE_K - 5], 2, 3),
            "cells": cells}


BATTERY["occurrence_table"] = Entry(table_call, table_want, lambda: SMALL()[0], (TABLE_K,))

VIEW_K, VIEW_PARTS = 33, 7


def views_call(eng):
    import torch
    s = eng.build_batch(SMALL()[0], VIEW_K)
    out = {"bounds": eng.partition_bounds(s, VIEW_PARTS), "bounds0": s[0].partition_bounds(VIEW_PARTS)}
    n, w = len(s[0]), words(VIEW_K)
    lo, hi = 5, n - 3
    kbuf = torch.full(((hi - lo) * w,), -1, dtype=torch.int64, device="cuda:0")
    cbuf = torch.full((hi - lo,), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    s[0].export_range(lo, hi, kbuf.data_ptr(), cbuf.data_ptr())
    eng.sync()
    wrap = eng.wrap_device(VIEW_K, hi - lo, kbuf.data_ptr(), cbuf.data_ptr())
    out["wrapped"] = set_to_db(wrap)
    out["wrapped_union"] = set_to_db(eng.union_sum([wrap, s[1]], 5000))
    return out


def views_want():
    d = small_dbs(VIEW_K)
    stored = []
    for db in d:
        keys, counts = db_to_arrays(db, VIEW_K)
        stored.append(XV.stored(VIEW_K, keys, counts))
    bounds = np.array([XV.ref_bounds(VIEW_K, m, VIEW_PARTS) for m, _ in stored])
    mixed, counts = stored[0]
    raw = unmix_np(VIEW_K, mixed[5:mixed.shape[0] - 3])
    wrapped = {int(lo) | (int(hi) << 64): int(c) for (lo, hi), c in zip(raw, counts[5:mixed.shape[0] - 3])}
    return {"bounds": bounds, "bounds0": bounds[0], "wrapped": wrapped, "wrapped_union": O.union_sum([wrapped, d[1]], 5000)}


BATTERY["views_bounds_export_wrap"] = Entry(views_call, views_want, lambda: SMALL()[0], (VIEW_K,))

# ---- super-k-mers
for _k in (17, 24, 31, 32, 33, 41, 63):
    add_exp1(f"skm_species_k{_k}", functools.partial(species, 3, 3, 20_000), _k, None, skm_only)
for _k in (17, 31):
    add_exp1(f"skm_stress_k{_k}", stress, _k, None, skm_any)
add_exp1("skm_large_slots_k31", functools.partial(species, 3, 3, 20_000), 31,
         {"KHOICE_SKM_MEAN": "6000", "KHOICE_SKM_SLACK": "1.1"}, skm_only)
add_exp1("skm_large_slots_k41", functools.partial(species, 3, 3, 20_000), 41,
         {"KHOICE_SKM_MEAN": "3000", "KHOICE_SKM_SLACK": "1.1"}, skm_only)


# (regions of 1.1 x the mean hold every slot of the species set: the side list and k_skm_big are reached by the inputs
# their own modules build for them)
@functools.lru_cache(maxsize=None)
def overfull_one_word():
    from tests.test_gpu_skm_hashsets import deep_case
    return tailed(*deep_case(31))


@functools.lru_cache(maxsize=None)
def overfull_two_words():
    from tests.test_gpu_skm2 import insertion_sequence_set
    return tailed(*insertion_sequence_set())


add_exp1("skm_overfull_k31", overfull_one_word, 31, {"KHOICE_SKM_SLACK": "0.3"}, skm_big)
add_exp1("skm_overfull_k47", overfull_two_words, 47, None, skm_big)
add_exp1("skm_two_passes_70_genomes_k31", functools.partial(species, 7, 10, 3_000), 31, None, skm_any)
add_exp1("skm_group_of_70_k31", big_group, 31, None, skm_any)


# ---- record exchange
@functools.lru_cache(maxsize=None)
def exchange_ranks(R):
    from tests import test_gpu_skm_exchange as XE
    ranks = []
    for r in range(R):
        seqs, tags = XE.species_rank(1 + 3 * r, 2, 2, 6_000)
        ranks.append(tailed(seqs, tags))
    return ranks


def add_exchange(R, k=31):
    def call(eng):
        from tests import test_gpu_skm_exchange as XE
        job = XE.Job(eng, exchange_ranks(R), k)
        owners = [job.owner_hist(j) for j in range(R)]
        return {"hist": sum(owners), "part_n": np.array(job.part_n)} | {f"owner{j}": h for j, h in enumerate(owners)}

    def want():
        seqs, groups, first = [], [], 0
        for s, t in exchange_ranks(R):
            seqs += s
            groups += [first + g for g in t]
            first += max(t) + 1
        return {"hist": CO.exp1(seqs, groups, k)["across_hist"]}

    BATTERY[f"exchange_{R}_ranks"] = Entry(call, want, lambda: [t for s, _ in exchange_ranks(R) for t in s], (k,), None,
                                           lambda d: d["skm_pack"] == R and d["skm_phased"] == R or pytest.fail(str(d)))


for _R in (2, 3):
    add_exchange(_R)

# ---- bitmaps
for _k in (1, 2, 3, 5, 8, 11, 12):
    add_exp1(f"bmp_exp1_k{_k}", functools.partial(species, 3, 3, 4_000), _k, BMP_EDGES, bitmaps)
add_exp1("bmp_exp1_k13", functools.partial(species, 3, 3, 4_000), 13, dict(BMP_EDGES, KHOICE_BMP_MAX_K="13"), bitmaps)
add_exp1("sets_exp1_k21", functools.partial(species, 3, 3, 4_000), 21, None,
         lambda d: d["setop"] > 0 and d["bmp_build"] == 0 or pytest.fail(str(d)), want_sets=True)


def add_pivots(kind, k, env, expect, n=3_000):
    X = {2: X2, 3: X3, 4: X4}[kind]
    case = functools.partial(pivot_case, kind, n)

    def call(eng):
        r = getattr(eng, f"exp{kind}_run")(*case(), k)
        return {f: r[f] for f in X.FIELDS}

    BATTERY[f"{'bmp' if k <= 12 else 'sets'}_exp{kind}_k{k}"] = Entry(
        call, lambda: X.oracle(*case(), k), lambda: case()[0] + case()[2], (k,), env, expect)


def cross_batches(d):
    bitmaps(d)
    assert d["bmp_cross"] == 3, d


for _k in (5, 9, 12):
    add_pivots(2, _k, BMP_EDGES, bitmaps)
    add_pivots(3, _k, dict(BMP_EDGES, KHOICE_BMP_MAX_BINS="51"), cross_batches)   # 12 genomes: 12 + 3 x 13 bins, 9 pivots
    add_pivots(4, _k, BMP_EDGES, bitmaps)
for _kind in (2, 3, 4):
    add_pivots(_kind, 21, None, set_form)


# ---- ingest
@functools.lru_cache(maxsize=None)
def fasta_files():
    """Three gz files whose cleaned texts end with TAILS: no newline at the end, CRLF, and a plain one last."""
    root = tempfile.mkdtemp(prefix="khoice_poison_")
    atexit.register(shutil.rmtree, root, ignore_errors=True)
    items = synth.species_set(1, 3, 3_000)
    paths = []
    for i, ((_, _, text), tail) in enumerate(zip(items, TAILS)):
        recs = text[(len(text) + 1) % 16:].split(b"\n") + [tail]         # the cleaned text is as long as its tail, mod 16
        nl = b"\r\n" if i == 1 else b"\n"
        body = b"".join(b">r%d" % j + nl + nl.join(r[p:p + 70] for p in range(0, len(r), 70)) + nl for j, r in enumerate(recs))
        if i == 0:
            body = body[:-1]
        paths.append(os.path.join(root, f"g{i}.fna.gz"))
        with gzip.open(paths[-1], "wb") as fh:
            fh.write(body)
    return paths


def cleaned_texts():
    return [b"\n".join(r.encode("latin-1") for r in O.fasta_records(O.read_fasta_bytes(p))) for p in fasta_files()]


INGEST_K = (9, 31)


def ingest_call(eng):
    texts = eng.ingest_fasta(fasta_files(), threads=2)
    out = {f"text{i}": texts.download(i) for i in range(len(texts.seqs))}
    out["read_fasta"] = [eng.read_fasta(p) == out[f"text{i}"] for i, p in enumerate(fasta_files())]
    for k in INGEST_K:
        r = eng.exp1_run(texts.seqs, [0, 0, 1], k)
        out.update({f"{f}_k{k}": r[f] for f in X1.FIELDS})
    texts.free()
    return out


def ingest_want():
    clean = cleaned_texts()
    out = {f"text{i}": t for i, t in enumerate(clean)}
    out["read_fasta"] = [True] * len(clean)
    for k in INGEST_K:
        w = CO.exp1(clean, [0, 0, 1], k)
        out.update({f"{f}_k{k}": w[f] for f in X1.FIELDS})
    return out


BATTERY["ingest_then_exp1_in_place"] = Entry(ingest_call, ingest_want, cleaned_texts, INGEST_K, None,
                                             lambda d: d["bmp_build"] >= 1 and d["skm_union"] == 1 or pytest.fail(str(d)))


# ---------------------------------------------------------------- running an entry
def same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.asarray(a), np.asarray(b)
        return a.shape == b.shape and bool((a == b).all())
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[n], b[n]) for n in a)
    return a == b


def measured(eng, call):
    """(outputs, {kernel class: launches, counter: growth}) of one call."""
    eng.profile(True)
    st0 = eng.stats()
    out = call(eng)
    st1 = eng.stats()
    eng.profile(False)
    d = {n: st1["kernels"][n]["launches"] - st0["kernels"][n]["launches"] for n in st1["kernels"]}
    for n in COUNTERS + ("poisoned_bytes",):
        d[n] = st1[n] - st0[n]
    return out, d


@functools.lru_cache(maxsize=None)
def wanted(name):
    return BATTERY[name].want()


CLEAN = {}


def clean_run(eng, name):
    """The entry without the knob (its own switches set by the caller): run once, kept for every pattern."""
    if name not in CLEAN:
        CLEAN[name] = measured(eng, BATTERY[name].call)
    return CLEAN[name]


def differing(got, ref):
    return [n for n in ref if n not in got or not same(got[n], ref[n])]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BATTERY))
@pytest.mark.parametrize("pattern", PATTERNS, ids=lambda p: f"p{p:02X}")
def test_poisoned_pool(eng, monkeypatch, pattern, name):
    entry = BATTERY[name]
    monkeypatch.delenv("KHOICE_DEBUG_POISON", raising=False)
    for var, value in entry.env.items():
        monkeypatch.setenv(var, value)
    clean, d0 = clean_run(eng, name)
    assert d0["poisoned_bytes"] == 0, d0
    monkeypatch.setenv("KHOICE_DEBUG_POISON", str(pattern))
    got, d1 = measured(eng, entry.call)
    monkeypatch.delenv("KHOICE_DEBUG_POISON")
    print(name, f"0x{pattern:02X}", d1["poisoned_bytes"], {n: v for n, v in d1.items() if v and n != "poisoned_bytes"})
    want = wanted(name)
    assert not differing(clean, want), ("without the knob", differing(clean, want))
    assert not differing(got, want), (f"0x{pattern:02X}", differing(got, want))
    assert not differing(got, clean) and got.keys() == clean.keys(), (f"0x{pattern:02X}", differing(got, clean))
    assert d1["poisoned_bytes"] > 0, d1
    assert {n: v for n, v in d1.items() if n != "poisoned_bytes"} == {n: v for n, v in d0.items() if n != "poisoned_bytes"}, (d0, d1)
    if entry.expect:
        entry.expect(d1)


@pytest.mark.gpu
def test_knob_is_read_at_every_allocation_and_ignores_what_is_no_byte(eng, monkeypatch):
    seqs, group_of = species(2, 2, 5_000)
    for value, active in (("", False), ("256", False), ("-1", False), ("x", False), ("0x41", True), ("255", True), ("0", True)):
        monkeypatch.setenv("KHOICE_DEBUG_POISON", value)
        _, d = measured(eng, lambda e: e.exp1_run(seqs, group_of, 31))
        assert (d["poisoned_bytes"] > 0) == active, (value, d["poisoned_bytes"])
    monkeypatch.delenv("KHOICE_DEBUG_POISON")
    _, d = measured(eng, lambda e: e.exp1_run(seqs, group_of, 31))
    assert d["poisoned_bytes"] == 0


def bytes_behind(texts, i, n):
    """n bytes of device memory right behind resident text i."""
    import ctypes
    ptr, length = texts.seqs[i]
    buf = (ctypes.c_ubyte * n)()
    rc = ctypes.CDLL("libamdhip64.so").hipMemcpy(buf, ctypes.c_void_p(ptr + length), ctypes.c_size_t(n), 2)   # device to host
    assert rc == 0, rc
    return bytes(buf)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", (0x41, 0xFF), ids=lambda p: f"p{p:02X}")
def test_the_fill_is_in_the_block_and_in_front_of_its_first_writer(eng, monkeypatch, pattern):
    """A resident text's block has 256 bytes more than the raw file: what the cleaning kernels did not write is the
    pattern, what they wrote is the text — the fill ran, on the whole block, before the block's first user."""
    monkeypatch.setenv("KHOICE_DEBUG_POISON", str(pattern))
    texts = eng.ingest_fasta(fasta_files(), threads=2)
    monkeypatch.delenv("KHOICE_DEBUG_POISON")
    for i, want in enumerate(cleaned_texts()):
        assert texts.download(i) == want
        assert bytes_behind(texts, i, 256) == bytes([pattern]) * 256, i
    texts.free()


# ---------------------------------------------------------------- recycled blocks that carry another form's live-looking data
@pytest.mark.gpu
def test_different_structure_in_a_row(eng, monkeypatch):
    """One engine, no knob: a super-k-mer call, a bitmap call and a key-array call, then the three in reverse order on
    other inputs, so that each form gets blocks another one has just filled with its own records, cursors and tables."""
    monkeypatch.delenv("KHOICE_DEBUG_POISON", raising=False)

    def skm(case):
        _, d = X1.run(eng, *case, 31)
        assert d["skm_union"] == 1 and d["retries"] == 0, d

    def bmp(case):
        X1.check(eng, *case, 9)

    def arrays(case):
        for s, text in zip(eng.build_batch(case[0], 33), case[0]):
            keys, counts = s.download_sorted()
            okeys, ocounts = CO.count(text, 33).arrays()
            assert same(keys, okeys) and same(counts, ocounts)
        monkeypatch.setenv("KHOICE_NO_SKM", "1")
        _, d = X1.run(eng, *case, 31)
        monkeypatch.delenv("KHOICE_NO_SKM")
        assert d["union_tagged"] >= 1 and d["skm_union"] == 0 and d["retries"] == 0, d

    a, b = species(3, 3, 20_000), species(4, 2, 13_000)
    eng.trim()                                                            # from an empty pool: the blocks below are these calls'
    for step, case in ((skm, a), (bmp, a), (arrays, a), (arrays, b), (bmp, b), (skm, b), (bmp, a), (skm, a)):
        step(case)


# ---------------------------------------------------------------- preconditions, without a GPU
def distinct(text, k):
    return len(CO.count(text, k))


def shows(text, k, p):
    """A reader that runs past len into 32 bytes of p changes the oracle's distinct count of the text."""
    return distinct(text + bytes([p]) * 32, k) != distinct(text, k)


def test_patterns_and_tails():
    assert PATTERNS == (0x00, 0x41, 0x63, 0xFF) and bytes(LETTERS) == b"Ac"
    assert [len(t) % 16 for t in TAILS] == [5, 5, 0] and all(len(t) >= 64 and set(t) <= set(b"ACGT") for t in TAILS)
    assert len({k for e in BATTERY.values() for k in e.ks}) >= 20


@pytest.mark.parametrize("name", list(BATTERY))
def test_every_entry_has_texts_that_show_a_reader_past_len(name):
    entry = BATTERY[name]
    texts = entry.texts()
    for k in entry.ks:
        assert k <= 64
        last = texts[-1]
        assert len(last) % 16 == 0 and last.endswith(TAILS[2])            # the 256 bytes behind the packed copy follow it
        odd = [t for t in texts[-3:] if len(t) % 16 != 0]
        assert odd and all(t.endswith(TAILS[0]) or t.endswith(TAILS[1]) for t in odd)
        for t in odd + [last]:                                            # each ends inside a run of at least k valid bases
            assert len(t) >= k and set(t[-k:]) <= set(b"ACGTacgt")
        for p in LETTERS:
            assert any(shows(t, k, p) for t in odd), (name, k, p)
            if k >= 2:
                assert all(shows(t, k, p) for t in odd) and shows(last, k, p), (name, k, p)
        if k == 1:                                                        # one letter each: no text of valid bases lacks both
            assert shows(last, 1, 0x41) and not shows(last, 1, 0x63)
        assert not any(shows(t, k, 0xFF) or shows(t, k, 0x00) for t in odd + [last])   # no base: only a stale read of state shows


def test_ingest_files_are_what_they_claim():
    raw = [O.read_fasta_bytes(p) for p in fasta_files()]
    assert not raw[0].endswith(b"\n") and b"\r\n" in raw[1] and b"\r" not in raw[0] + raw[2] and raw[2].endswith(b"\n")
    clean = cleaned_texts()
    assert [t.endswith(tail) for t, tail in zip(clean, TAILS)] == [True] * 3
    assert all(b"\r" not in t and b">" not in t for t in clean)
    for k in INGEST_K:
        assert all(distinct(t, k) > 1000 for t in clean)
