"""Seeded random sweep of kh_exp2_run, kh_exp3_run, kh_exp4_run and kh_exp6_run over every form of each: presence
bitmaps (k <= 12, and k = 13 behind KHOICE_BMP_MAX_K), the set operations, and for types 2 and 3 the super-k-mer form of
k = 17 .. 63 (KHOICE_EXP2_SKM=1 / KHOICE_EXP3_SKM=1).  The shapes are drawn, not constructed: k across the form
boundaries, groups interleaved in the caller's order, empty genomes and genomes of k - 1 bases beside ordinary ones, N
runs, lower case, several records and low-complexity tails in one call, pivots that copy a genome, share a group or hold
a stretch a few hundred times, and cs / hist_len / pivot_cs drawn with them.  Every form of a case is compared with ==
against the restatements the constructed tests use (imported, not restated; computed once per case and shared), and the
launch counts must show that the form asked for answered, alone and without a retry.  The texts are small — the tile,
slot and table edges are the constructed tests' business — so that a case costs a fraction of a second of oracle.

The unmarked tests prove from draw_case and the oracles alone that the 24 seeds of every kind hold what the GPU tests
rely on."""
import functools
import random
import re
import types

import numpy as np
import pytest

from oracle import kmer_oracle as O
from tests import read_level_oracle as RL
from tests import test_gpu_exp2_bmp as X2
from tests import test_gpu_exp2_skm as S2
from tests import test_gpu_exp3 as X3
from tests import test_gpu_exp3_skm as S3
from tests import test_gpu_exp4 as X4
from tests import test_gpu_exp6_bmp as X6
from tests.util import random_dna

KINDS = (2, 3, 4, 6)
NSEEDS = 24
KS = [1, 3, 5, 8, 11, 12, 13, 15, 16, 17, 21, 27, 31, 32, 33, 41, 47, 55, 63, 64]
RATES = (0.0, 0.001, 0.01, 0.05)
CS, HIST_LEN, PIVOT_CS = (1, 2, 3, 255, 5000), (2, 3, 64, 300, 5001), (1, 2, 255, 2**32 - 1)
MAX_BASES = 150_000
SEED_BASE = 0x5EED02
FIXED_K = (8, 21, 41)            # of the deterministic extras
FIELDS = {2: X2.FIELDS, 3: X3.FIELDS, 4: X4.FIELDS, 6: ("within_hist", "distinct_per_seq", "tie_masks", "unmatched")}
SWITCHES = ("KHOICE_NO_BMP", "KHOICE_NO_SKM", "KHOICE_NO_SKM2", "KHOICE_BMP_MAX_K", "KHOICE_BMP_MAX_BYTES", "KHOICE_BMP_MAX_BINS",
            "KHOICE_EXP2_SKM", "KHOICE_EXP3_SKM", "KHOICE_SKM_MIN_K", "KHOICE_SKM_MEAN", "KHOICE_READS_MAX_POS")
KH_E_ARG = -1


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


# ---------------------------------------------------------------- the draw
def has_kmer(text, k):
    return re.search("[ACGTacgt]{%d}" % k, text) is not None


def mutated(rng, anc):
    t = list(anc)
    for _ in range(int(len(t) * rng.choice(RATES))):
        t[rng.randrange(len(t))] = rng.choice("ACGT")
    return t


def decorated(rng, t, k, shared, p_shared=0.5):
    """The decorations of the type-1 draw: N runs, the shared block behind an N, a poly-A record, a lower-cased half."""
    for _ in range(rng.randrange(0, 4)):
        at = rng.randrange(len(t))
        n = min(rng.randrange(1, 40), len(t) - at)
        t[at:at + n] = "N" * n
    s = "".join(t)
    if rng.random() < p_shared:
        s += "N" + shared
    if rng.random() < 0.3:
        s += "\n" + "A" * rng.randrange(k, k + 300)
    if rng.random() < 0.3:
        s = s[:len(s) // 2].lower() + s[len(s) // 2:]
    return s


def draw_reads(rng, k, genomes, group_of, shared):
    """1 - 3 read sets of 5 - 60 reads of upper-case ACGT: cuts of the genomes' clean stretches (0 .. 400 bases; k - 1, k
    and k + 1 lead the first set), cuts of the shared block, random sequence, and reads pieced together from two groups."""
    runs = {}
    for text, g in zip(genomes, group_of):
        runs.setdefault(g, []).extend(r for r in re.findall("[ACGT]+", text.upper().replace("\n", "N")) if len(r) >= 8)
    groups = sorted(g for g, r in runs.items() if r)

    def cut(n, g=None):
        if not groups:
            return random_dna(rng, n)
        pool = runs[groups[rng.randrange(len(groups))] if g is None else g]
        fit = [r for r in pool if len(r) >= n] or [max(pool, key=len)]
        r = fit[rng.randrange(len(fit))]
        at = rng.randrange(0, max(1, len(r) - n + 1))
        return r[at:at + n]

    out = []
    for s in range(rng.randrange(1, 4)):
        reads = []
        for i in range(rng.randrange(5, 61)):
            u = rng.random()
            if s == 0 and i < 3:
                read = cut(k - 1 + i)
                read += random_dna(rng, k - 1 + i - len(read))          # (no clean stretch that long: filled up)
            elif u < 0.12:
                read = random_dna(rng, rng.randrange(0, 401))
            elif u < 0.24 and groups:
                a = groups[rng.randrange(len(groups))]
                b = groups[rng.randrange(len(groups))]
                read = cut(rng.randrange(0, 200), a) + cut(rng.randrange(0, 200), b)
            elif u < 0.36:
                at = rng.randrange(len(shared))
                read = shared[at:at + rng.randrange(0, 401)]
            else:
                read = cut(rng.randrange(0, 401))
            reads.append(read)
        out.append(tuple(reads))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def draw_case(kind, seed, k=None):
    """A pure function of (kind, seed): the first twenty seeds of a kind take every k of KS once, in an order of the
    kind's own; `k` overrides the drawn one (the deterministic extras).  -> k, seqs, group_of, pivots, pivot_group
    (type 2), reads (type 6: read sets of str), cs, hist_len, pivot_cs."""
    assert kind in KINDS
    rng = random.Random(SEED_BASE + 1000 * kind + seed)
    drawn = rng.choice(KS)
    if k is None:
        k = random.Random(SEED_BASE + kind).sample(KS, len(KS))[seed] if seed < len(KS) else drawn
    ngroups = rng.choice((1, 2, 2, 3, 3, 4))
    barren = None                                     # one case in about eight: a group none of whose genomes holds a k-mer
    if rng.random() < 0.125:
        ngroups = max(ngroups, 2)
        barren = rng.randrange(ngroups)
    shared = random_dna(rng, rng.randrange(100, 1200))
    ancestors, genomes = [], []
    for g in range(ngroups):
        anc = random_dna(rng, int(10 ** rng.uniform(2.5, 3.5)))
        ancestors.append(anc)
        members = []
        for _ in range(rng.randrange(1, 5)):
            s = decorated(rng, mutated(rng, anc), k, shared)
            u = rng.random()
            if g == barren:
                s = rng.choice(("", anc[:k - 1], "N" * rng.randrange(1, 2 * k + 2), anc[:k // 2].lower()))
            elif u < 0.08:
                s = ""
            elif u < 0.16:
                s = anc[:k - 1]
            members.append(s)
        if g != barren and not any(has_kmer(s, k) for s in members):
            members[0] = anc
        genomes += [(s, g) for s in members]
    if rng.random() < 0.65:
        rng.shuffle(genomes)
    seqs, group_of = [s for s, _ in genomes], [g for _, g in genomes]
    case = types.SimpleNamespace(kind=kind, seed=seed, k=k, seqs=tuple(s.encode() for s in seqs), group_of=tuple(group_of), pivots=(),
                                 pivot_group=(), reads=(), cs=rng.choice(CS), hist_len=rng.choice(HIST_LEN), pivot_cs=rng.choice(PIVOT_CS))
    if kind == 6:
        case.reads = draw_reads(rng, k, seqs, group_of, shared)
        return case
    pivots, pivot_group, repeated = [], [], False
    with_kmers = [i for i, s in enumerate(seqs) if has_kmer(s, k)]
    for _ in range(rng.choice((0, 1, 1, 2, 2, 3, 3, 4))):
        g, u = rng.randrange(ngroups), rng.random()
        if 0.45 <= u < 0.60 and with_kmers:           # an exact copy of one genome
            i = with_kmers[rng.randrange(len(with_kmers))]
            text, g = seqs[i], group_of[i]
        elif 0.60 <= u < 0.72:                        # unrelated sequence
            text = random_dna(rng, rng.randrange(k, 2000))
        elif 0.72 <= u < 0.85:                        # empty or shorter than k
            text = rng.choice(("", ancestors[g][:k - 1]))
        elif u >= 0.85 and not repeated:              # a stretch repeated 2 .. 300 times (one pivot of a case at most: the size)
            repeated = True
            stretch = random_dna(rng, rng.randrange(k, k + 30))
            times = rng.choice((rng.randrange(2, 301), rng.randrange(257, 301)))
            at = rng.randrange(len(ancestors[g]))
            text = ancestors[g][:at][-300:] + stretch * times + ancestors[g][at:at + 300]
        else:                                         # a further mutated copy of the group's ancestor
            text = decorated(rng, mutated(rng, ancestors[g]), k, shared, 0.85)
        pivots.append(text.encode())
        pivot_group.append(g if rng.random() < 0.5 else rng.randrange(ngroups))
    case.pivots = tuple(pivots)
    if kind == 2:
        case.pivot_group = tuple(pivot_group)
    return case


def total_bases(case):
    return sum(len(t) for t in case.seqs + case.pivots) + sum(len(r) for reads in case.reads for r in reads)


def interleaved(case):
    return list(case.group_of) != sorted(case.group_of)


def sorted_by_group(case):
    """The same case with the genomes sorted by group (a stable sort), and the order: new position -> old index."""
    order = sorted(range(len(case.seqs)), key=case.group_of.__getitem__)
    new = types.SimpleNamespace(**vars(case))
    new.seqs = tuple(case.seqs[i] for i in order)
    new.group_of = tuple(case.group_of[i] for i in order)
    return new, order


def interleaved_case(kind, k):
    """The first drawn case of (kind, k) from seed 100 on whose group_of is interleaved and, for types 2 - 4, that has a pivot."""
    for seed in range(100, 200):
        case = draw_case(kind, seed, k)
        if interleaved(case) and (kind == 6 or case.pivots):
            return case
    raise AssertionError((kind, k))


@functools.lru_cache(maxsize=None)
def error_case(k):
    """Type 6: a drawn case of this k whose read set holds two reads of at least k bases with a bad byte, an N in one
    and a lower-case base in the other (which of the two comes first changes with k).  -> case, set, lower read"""
    for seed in range(200, 300):
        case = draw_case(6, seed, k)
        for p, reads in enumerate(case.reads):
            long = [i for i, r in enumerate(reads) if len(r) >= k + 2]
            if len(long) >= 4:
                lo, hi = long[1], long[-1]
                spoil = [lambda r: r[:-1] + "N", lambda r: r[:2] + r[2].lower() + r[3:]]
                if k % 2:
                    spoil.reverse()
                reads = list(reads)
                reads[lo], reads[hi] = spoil[0](reads[lo]), spoil[1](reads[hi])
                new = types.SimpleNamespace(**vars(case))
                new.reads = case.reads[:p] + (tuple(reads),) + case.reads[p + 1:]
                return new, p, lo
    raise AssertionError(k)


# ---------------------------------------------------------------- the oracles (imported), once per case
def group_kmer_strings(case):
    """The groups' k-mer sets as the read-level restatement wants them, from the databases of oracle/kmer_oracle.py."""
    sets = [set() for _ in range(max(case.group_of) + 1)]
    for text, g in zip(case.seqs, case.group_of):
        sets[g] |= {O.decode(c, case.k) for c in X2.plain_set(text, case.k)}
    return sets


def oracle_of(case):
    seqs, group_of, k = list(case.seqs), list(case.group_of), case.k
    if case.kind == 2:
        return X2.oracle(seqs, group_of, list(case.pivots), list(case.pivot_group), k, case.cs, case.hist_len)
    if case.kind == 3:
        return X3.oracle(seqs, group_of, list(case.pivots), k, case.cs, case.hist_len)
    if case.kind == 4:
        return X4.oracle(seqs, group_of, list(case.pivots), k, case.cs, case.hist_len, case.pivot_cs)
    x4 = X4.oracle(seqs, group_of, [], k, case.cs, case.hist_len)
    sets = group_kmer_strings(case)
    votes = [RL.reads_votes(reads, k, sets) for reads in case.reads]
    return {"within_hist": x4["within_hist"], "distinct_per_seq": x4["distinct_per_seq"], "votes": votes,
            "tie_masks": [RL.tie_masks(v, len(sets)) for v in votes],
            "unmatched": [np.array([w[2] for w in v], dtype=np.uint32) for v in votes]}


@functools.lru_cache(maxsize=None)
def wanted(kind, seed, k=None):
    """Computed once per case, shared by its forms and by the unmarked tests; nobody writes to it."""
    return oracle_of(draw_case(kind, seed, k))


# ---------------------------------------------------------------- the forms
def forms_of(kind, k, npivots):
    """[(form, switches)] of the issue's table."""
    if k <= 12:
        return [("bitmaps", {}), ("sets", {"KHOICE_NO_BMP": "1"})]
    if k == 13:
        return [("sets", {}), ("bitmaps", {"KHOICE_BMP_MAX_K": "13"})]
    out = [("sets", {})]
    if 17 <= k <= 63 and kind in (2, 3) and npivots:
        out.append(("skm", {f"KHOICE_EXP{kind}_SKM": "1"}))
    return out


def set_switches(monkeypatch, switches):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in switches.items():
        monkeypatch.setenv(name, value)


class DeviceTexts:
    """Every text of a case in one torch.uint8 tensor, back to back: most texts at an address that is no multiple of
    16, the bytes behind a text its neighbour's."""

    def __init__(self, case):
        import torch
        texts = list(case.seqs) + list(case.pivots) + [X6.layout(r)[0] for r in case.reads]
        blob = b"".join(texts) + b"A" * 64
        self.dev = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to("cuda:0")
        torch.cuda.synchronize()
        at, out = self.dev.data_ptr(), []
        for t in texts:
            out.append((at, len(t)))
            at += len(t)
        n, m = len(case.seqs), len(case.seqs) + len(case.pivots)
        self.seqs, self.pivots, self.reads = out[:n], out[n:m], out[m:]


def same(kind, a, b):
    for f in FIELDS[kind]:
        if isinstance(a[f], list):
            assert len(a[f]) == len(b[f]), f
            for x, y in zip(a[f], b[f]):
                assert x.shape == y.shape and (x == y).all(), f
        else:
            assert a[f].shape == b[f].shape and a[f].dtype == b[f].dtype and (a[f] == b[f]).all(), f


def skm_alone(d, nseq, npivots):
    """`check` of tests/test_gpu_exp2_skm.py and tests/test_gpu_exp3_skm.py on the deltas of one pass: one launch of
    the slot walk, and a second one exactly when slots were listed (a drawn shape may crowd one minimizer)."""
    assert d["skm_cross"] == 1 + (d["big_slots"] > 0), d
    assert d["skm_scatter"] >= 1 and d["skm_regroup"] >= 1, d
    assert d["skm_union"] == 0 and d["skm_big"] == 0 and d["setop"] == 0 and d["union_tagged"] == 0 and d["retries"] == 0, d
    assert all(v == 0 for n, v in d.items() if n.startswith("bmp_")), d
    assert d["builds"] == nseq + npivots, d


def sets_alone(d):
    """Where no genome holds a k-mer no set operation has anything to launch: `by_sets` without its `setop > 0`."""
    assert all(v == 0 for n, v in d.items() if n.startswith("bmp_")) and d.get("skm_cross", 0) == 0 and d["retries"] == 0, d


def run_form(eng, case, want, form, dev=None):
    """One call in the form the switches ask for: every field against the oracle, and the form from the statistics."""
    kind, k, group_of = case.kind, case.k, list(case.group_of)
    seqs, pivots = (dev.seqs, dev.pivots) if dev else (list(case.seqs), list(case.pivots))
    nseq, npiv = len(seqs), len(pivots)
    launches = bool(want["distinct_per_seq"].sum()) and (kind != 3 or npiv > 0)     # the set form has a set operation to launch
    if kind == 6:
        reads = [(dev.reads[p] if dev else X6.layout(r)[0], X6.layout(r)[1]) for p, r in enumerate(case.reads)]
        r0 = eng.stats()["retries"]
        got, d = X6.measured(eng, lambda: eng.exp6_run(seqs, group_of, reads, k, cs=case.cs, hist_len=case.hist_len))
        assert eng.stats()["retries"] == r0
        same(6, got, want)
        (X6.bitmap_form if form == "bitmaps" else X6.set_form)(d, len(reads))
        assert all(d[n] == 0 for n in d if n.startswith("skm_")), d
        return got
    mod = {2: X2, 3: X3, 4: X4}[kind]
    args = (eng, seqs, group_of, pivots) + ((list(case.pivot_group),) if kind == 2 else ()) + (k,)
    kw = dict(cs=case.cs, hist_len=case.hist_len, want=want)
    if kind == 4:
        kw["pivot_cs"] = case.pivot_cs
    if form == "bitmaps":
        got, d = mod.check(*args, **kw)
    elif form == "skm":
        got, d = {2: S2, 3: S3}[kind].run(*args, **kw)
        skm_alone(d, nseq, npiv)
    elif launches:
        got, d = mod.by_sets(*args, **kw)
        assert d["retries"] == 0, d
    else:
        got, d = mod.run(*args, **kw)
        sets_alone(d)
    same(kind, got, want)                               # (the modules' `run` has compared them already: shapes, types and lists again)
    return got


# ---------------------------------------------------------------- the sweep
@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(NSEEDS))
@pytest.mark.parametrize("kind", KINDS)
def test_every_form_on_random_shapes(eng, monkeypatch, kind, seed):
    case, want = draw_case(kind, seed), wanted(kind, seed)
    dev = DeviceTexts(case) if seed % 3 == 0 else None     # every third seed: the texts device-resident as well
    for form, switches in forms_of(kind, case.k, len(case.pivots)):
        set_switches(monkeypatch, switches)
        got = run_form(eng, case, want, form)
        if dev:
            same(kind, run_form(eng, case, want, form, dev), got)
        if seed % 6 == 0:                                  # four seeds of a kind: the second call equals the first
            same(kind, run_form(eng, case, want, form), got)


@pytest.mark.gpu
@pytest.mark.parametrize("k", FIXED_K)
@pytest.mark.parametrize("kind", KINDS)
def test_interleaved_groups_give_what_sorted_groups_give(eng, monkeypatch, kind, k):
    case = interleaved_case(kind, k)
    other, order = sorted_by_group(case)
    want, want_sorted = wanted(kind, case.seed, k), oracle_of(other)
    for form, switches in forms_of(kind, k, len(case.pivots)):
        set_switches(monkeypatch, switches)
        a, b = run_form(eng, case, want, form), run_form(eng, other, want_sorted, form)
        back = dict(b)
        back["distinct_per_seq"] = np.zeros_like(b["distinct_per_seq"])
        back["distinct_per_seq"][order] = b["distinct_per_seq"]      # the permutation undone
        same(kind, a, back)


@pytest.mark.gpu
@pytest.mark.parametrize("k", FIXED_K)
def test_exp6_bad_bytes_in_two_reads(eng, monkeypatch, k):
    from khoice_amd import engine as E
    case, p, lo = error_case(k)
    reads = [X6.layout(r) for r in case.reads]
    texts = []
    for form, switches in forms_of(6, k, 0):
        set_switches(monkeypatch, switches)
        with pytest.raises(E.KhoiceError) as ei:
            eng.exp6_run(list(case.seqs), list(case.group_of), reads, k, cs=case.cs, hist_len=case.hist_len)
        assert ei.value.code == KH_E_ARG and f"read {lo} " in str(ei.value), (form, str(ei.value))
        texts.append(str(ei.value))
    assert len(texts) == (2 if k <= 12 else 1) and len(set(texts)) == 1, texts
    set_switches(monkeypatch, {})
    clean = draw_case(6, case.seed, k)                      # and the context still works
    run_form(eng, clean, wanted(6, case.seed, k), forms_of(6, k, 0)[0][0])


# ---------------------------------------------------------------- what the GPU tests rely on, without a GPU
def k_classes(ks):
    return {"k<=12": any(k <= 12 for k in ks), "k=13": 13 in ks, "14..16": any(14 <= k <= 16 for k in ks),
            "17..32": any(17 <= k <= 32 for k in ks), "33..63": any(33 <= k <= 63 for k in ks), "k=64": 64 in ks}


def holds(case, want):
    """What one case holds of the issue's list."""
    k, seqs = case.k, case.seqs
    ng = max(case.group_of) + 1
    per_group = [sum(int(d) for d, g in zip(want["distinct_per_seq"], case.group_of) if g == h) for h in range(ng)]
    out = {"interleaved": interleaved(case), "empty genome": any(len(s) == 0 for s in seqs),
           "genome of k - 1 bases": k >= 2 and any(len(s) == k - 1 for s in seqs), "group without k-mers": 0 in per_group,
           "lower case": any(re.search(b"[acgt]", s) for s in seqs), "N run": any(re.search(b"NN", s) for s in seqs),
           "records": any(b"\n" in s for s in seqs)}
    if case.kind != 6:
        dpp = want["distinct_per_pivot"]
        out.update({"no pivot": not case.pivots, "pivot equal to a genome": any(t in seqs and dpp[p] > 0 for p, t in enumerate(case.pivots)),
                    "pivot without k-mers": any(d == 0 for d in dpp),
                    "multiplicity above 255": any(max(X4.counted(t, k, 2**32 - 1).values(), default=0) > 255 for t in case.pivots)})
    if case.kind == 2:
        out["two pivots of one group"] = len(set(case.pivot_group)) < len(case.pivot_group)
        out["group without a pivot"] = bool(case.pivots) and len(set(case.pivot_group)) < ng
    if case.kind == 6:
        flat = [(r, v) for reads, votes in zip(case.reads, want["votes"]) for r, v in zip(reads, votes)]
        windows = lambda r: max(0, len(r) - k + 1)
        out.update({"read shorter than k": any(len(r) < k for r, _ in flat),
                    "read with nothing held": any(windows(r) >= 1 and v[2] == windows(r) and len(v[1]) == ng for r, v in flat),
                    "tie of two": ng > 2 and any(len(v[1]) == 2 and v[2] < windows(r) for r, v in flat),
                    "single winner": ng >= 2 and any(len(v[1]) == 1 for _, v in flat)})
    return out


def says_something(field):
    return any(x.any() for x in field) if isinstance(field, list) else bool(field.any())


@pytest.mark.parametrize("kind", KINDS)
def test_the_seeds_hold_what_the_sweep_is_for(kind):
    cases = [draw_case(kind, s) for s in range(NSEEDS)]
    assert all(k_classes([c.k for c in cases]).values()), k_classes([c.k for c in cases])
    assert {c.k for c in cases} == set(KS)
    seen = [holds(c, wanted(kind, c.seed)) for c in cases]
    count = {what: sum(h[what] for h in seen) for what in seen[0]}
    assert count["interleaved"] >= 8, count
    assert all(n >= 1 for n in count.values()), count
    for c in cases:
        assert total_bases(c) <= MAX_BASES and 1 <= len(c.seqs) <= 16 and max(c.group_of) + 1 <= 4, (c.seed, total_bases(c))
        assert set(c.group_of) == set(range(max(c.group_of) + 1))
        assert c.cs in CS and c.hist_len in HIST_LEN and c.pivot_cs in PIVOT_CS
        assert all(1 <= [g for g in c.group_of].count(h) <= 4 for h in set(c.group_of))
        if kind == 6:
            assert 1 <= len(c.reads) <= 3 and all(5 <= len(r) <= 60 for r in c.reads)
            assert all(set(r) <= set("ACGT") and len(r) <= 400 for reads in c.reads for r in reads)
            assert [len(r) for r in c.reads[0][:3]] == [c.k - 1, c.k, c.k + 1]
        else:
            assert len(c.pivots) <= 4 and (kind != 2 or all(0 <= g <= max(c.group_of) for g in c.pivot_group))
    if kind in (2, 3):                                     # the super-k-mer form is really swept
        assert sum(1 for c in cases if 17 <= c.k <= 63 and c.pivots) >= 6
    for f in FIELDS[kind]:                                 # every field says something in half the cases or more
        alive = sum(1 for c in cases if says_something(wanted(kind, c.seed)[f]))
        assert alive >= NSEEDS // 2, (f, alive)


def test_the_draw_is_a_pure_function():
    for kind in KINDS:
        a = draw_case(kind, 5)
        draw_case.cache_clear()
        b = draw_case(kind, 5)
        assert a is not b and vars(a) == vars(b)
        assert draw_case(kind, 5, 21).k == 21 and draw_case(kind, 6).seqs != a.seqs


PAIRS = {2: 40, 3: 41, 4: 32, 6: 33}   # (case, form) pairs of the sweep per kind


def test_the_forms_of_the_table():
    assert [f for f, _ in forms_of(2, 12, 1)] == ["bitmaps", "sets"] and forms_of(4, 12, 0)[1][1] == {"KHOICE_NO_BMP": "1"}
    assert forms_of(6, 13, 0) == [("sets", {}), ("bitmaps", {"KHOICE_BMP_MAX_K": "13"})]
    assert [f for f, _ in forms_of(3, 16, 2)] == [f for f, _ in forms_of(3, 64, 2)] == [f for f, _ in forms_of(4, 21, 2)] == ["sets"]
    assert forms_of(2, 17, 1)[1] == ("skm", {"KHOICE_EXP2_SKM": "1"}) and forms_of(3, 63, 1)[1] == ("skm", {"KHOICE_EXP3_SKM": "1"})
    assert [f for f, _ in forms_of(2, 21, 0)] == ["sets"]
    pairs = {kind: sum(len(forms_of(kind, c.k, len(c.pivots))) for c in (draw_case(kind, s) for s in range(NSEEDS))) for kind in KINDS}
    assert pairs == PAIRS, pairs


def test_the_extras_are_what_they_claim():
    for k in FIXED_K:
        case, p, lo = error_case(k)
        clean = draw_case(6, case.seed, k).reads[p]
        bad = [i for i, (a, b) in enumerate(zip(case.reads[p], clean)) if a != b]
        assert len(bad) == 2 and bad[0] == lo and all(len(clean[i]) >= k for i in bad)
        spoiled = "".join(case.reads[p][i] for i in bad)
        assert "N" in spoiled and re.search("[acgt]", spoiled) and set(spoiled.upper()) <= set("ACGTN")
        assert ("N" in case.reads[p][lo]) == (k % 2 == 0)
        for kind in KINDS:
            c = interleaved_case(kind, k)
            other, order = sorted_by_group(c)
            assert c.k == k and interleaved(c) and not interleaved(other) and sorted(order) == list(range(len(c.seqs)))
            assert [c.seqs[i] for i in order] == list(other.seqs) and total_bases(c) <= MAX_BASES
            assert kind == 6 or c.pivots
