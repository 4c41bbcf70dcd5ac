"""GPU: the sorted-set operations (k_range_bounds, k_setop with its distribution sort, run-length
emit and fused histogram, k_histogram, and the host planner / re-plan loop of kh_engine.cpp) on
CONSTRUCTED sets: keys chosen in mixed space (so the test decides their slots), counters up to
2^32 - 1, every fan-in boundary and histogram tier.  Every result is compared, key by key and
counter by counter, with a plain numpy restatement: int64 counters combined, clamped at cs, and
dropped when <= 0."""
import math
import os

import numpy as np
import pytest

from tests.util import (Operand, boundary_mixed, clustered_mixed, counter_mix, distinct_raw, edge_mixed, key_view,
                        mixed_from_top32, ref_hist, uniform_mixed, unmix_np, view_keys, words)

pytestmark = pytest.mark.gpu

KS = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64]
U32 = (1 << 32) - 1
CS_LIST = [1, 2, 255, 5000, 2**31 - 1, 2**31, 2**32 - 2, 2**32 - 1]
UNIFORM_V = [2, 255, 2**31 - 1, 2**31, 3_000_000_000, 2**32 - 1]
HIST_LENS = [2, 15, 16, 17, 511, 512, 513, 5001]
MODES = ["min", "max", "sum", "diff", "left", "right"]
UNION, INTERSECT, KMERS_SUBTRACT, COUNTERS_SUBTRACT = 0, 1, 2, 3
E_ARG, E_CAPACITY = -1, -6


@pytest.fixture(scope="module")
def E():
    from khoice_amd import build as kbuild
    from khoice_amd import engine
    kbuild.build_library()
    return engine


@pytest.fixture(scope="module")
def eng(E):
    e = E.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_tickets(E):
    """Second context whose ordered kernels take their parts by atomic ticket (KHOICE_TICKETS)."""
    old = os.environ.get("KHOICE_TICKETS")
    os.environ["KHOICE_TICKETS"] = "1"
    try:
        e = E.Engine(0)
    finally:
        if old is None:
            del os.environ["KHOICE_TICKETS"]
        else:
            os.environ["KHOICE_TICKETS"] = old
    yield e
    e.close()


# ---------------------------------------------------------------- construction
def planner_slots(total, nsets, W):
    """setop_prepare / setop_plan's first slot count (same cap with or without payload)."""
    cap = 4096 if W == 1 else 2048
    zg = 5.0 * math.sqrt(max(1, nsets))
    x = 0.5 * (-zg + math.sqrt(zg * zg + 4.0 * cap))
    target = max(16, min(cap * 92 // 100, int(x * x)))
    return max(1, -(-total // target))


# ---------------------------------------------------------------- reference
class Pair:
    """Key alignment of two operands (independent of their counters)."""

    def __init__(self, k, ka, kb):
        self.k = k
        va, vb = key_view(ka), key_view(kb)
        self.u, inv = np.unique(np.concatenate([va, vb]), return_inverse=True)
        inv = inv.reshape(-1)
        self.ia, self.ib = inv[:va.shape[0]], inv[va.shape[0]:]
        self.ha = np.zeros(self.u.shape[0], dtype=bool)
        self.hb = np.zeros(self.u.shape[0], dtype=bool)
        self.ha[self.ia] = True
        self.hb[self.ib] = True

    def combine(self, ca_in, cb_in, op, mode):
        """Unclamped int64 result counter of every key of the pair (<= 0: not in the result)."""
        ca = np.zeros(self.u.shape[0], dtype=np.int64)
        cb = np.zeros(self.u.shape[0], dtype=np.int64)
        ca[self.ia] = ca_in
        cb[self.ib] = cb_in
        both = self.ha & self.hb
        comb = {"min": np.minimum(ca, cb), "max": np.maximum(ca, cb), "sum": ca + cb,
                "diff": ca - cb, "left": ca, "right": cb}[mode]
        if op == UNION:
            return np.where(both, comb, ca + cb)
        if op == INTERSECT:
            return np.where(both, comb, 0)
        if op == KMERS_SUBTRACT:
            return np.where(self.ha & ~self.hb, ca, 0)
        return np.where(self.ha, ca - cb, 0)

    def result(self, c, cs):
        c = np.minimum(c, cs)
        keep = c > 0
        return view_keys(self.u[keep], self.k), c[keep]


def ref_union(k, operands, cs=None):
    """Keys and int64 counter sums of an n-ary union, clamped at cs (unclamped when cs is None)."""
    if not operands or sum(o.keys.shape[0] for o in operands) == 0:
        return np.zeros((0, words(k)), dtype=np.uint64), np.zeros(0, dtype=np.int64)
    v = np.concatenate([key_view(o.keys) for o in operands])
    c = np.concatenate([o.counts for o in operands])
    u, inv = np.unique(v, return_inverse=True)
    tot = np.zeros(u.shape[0], dtype=np.int64)
    np.add.at(tot, inv.reshape(-1), c)
    return view_keys(u, k), (tot if cs is None else np.minimum(tot, cs))


def assert_set(got, keys, counts, what):
    gk, gc = got.download_sorted()
    assert gk.shape[0] == keys.shape[0], (what, "size", gk.shape[0], keys.shape[0])
    bad_k = np.nonzero((gk != keys).any(axis=1))[0]
    assert bad_k.size == 0, (what, "key", int(bad_k[0]), gk[bad_k[0]], keys[bad_k[0]])
    bad_c = np.nonzero(gc.astype(np.int64) != counts)[0]
    assert bad_c.size == 0, (what, "counter", int(bad_c[0]), int(gc[bad_c[0]]), int(counts[bad_c[0]]))


BINARY_OPS = ([(UNION, m, False) for m in MODES] + [(INTERSECT, m, False) for m in MODES] +
              [(KMERS_SUBTRACT, "left", False), (KMERS_SUBTRACT, "left", True),
               (COUNTERS_SUBTRACT, "diff", False), (COUNTERS_SUBTRACT, "diff", True)])


def run_binary_matrix(eng, k, a, b, cs_list, what):
    """Every binary operation (both operand orders for the subtractions) at every cs."""
    pab, pba = Pair(k, a.keys, b.keys), Pair(k, b.keys, a.keys)
    for op, mode, swap in BINARY_OPS:
        x, y, p = (b, a, pba) if swap else (a, b, pab)
        c = p.combine(x.counts, y.counts, op, mode)
        for cs in cs_list:
            keys, counts = p.result(c, cs)
            got = eng.simple(x.set, y.set, op, mode, cs)
            assert_set(got, keys, counts, (what, k, op, mode, swap, cs))
            got.free()


# ---------------------------------------------------------------- input validation and the 2^31 line
@pytest.mark.parametrize("k", KS)
def test_upload_rejects_keys_beyond_4k_and_zero_counters(eng, E, k):
    W = words(k)
    good = np.array([[1, 0][:W]], dtype=np.uint64)
    if k not in (32, 64):
        bad = good.copy()
        bad[0, W - 1] |= np.uint64(1) << np.uint64(2 * k - 64 * (W - 1))   # the key 4^k (+ 1)
        with pytest.raises(E.KhoiceError) as ei:
            eng.upload(k, np.concatenate([good * 0, bad]))
        assert ei.value.code == E_ARG
        top = good.copy()
        top[0, W - 1] = np.uint64(1 << 63)                                    # stray top bit
        with pytest.raises(E.KhoiceError) as ei:
            eng.upload(k, top)
        assert ei.value.code == E_ARG
    with pytest.raises(E.KhoiceError) as ei:
        eng.upload(k, np.concatenate([good * 0, good]), np.array([3, 0], dtype=np.uint32))
    assert ei.value.code == E_ARG
    s = eng.upload(k, good, np.array([7], dtype=np.uint32))                 # still usable
    keys, counts = s.download_sorted()
    assert (keys == good).all() and counts.tolist() == [7]


@pytest.mark.parametrize("k", [31, 33])
def test_counters_of_2_31_and_above_are_exact(eng, k):
    rng = np.random.default_rng(k)
    a = Operand(eng, k, distinct_raw(k, uniform_mixed(k, 3000, rng)))
    for v in (2**31, 3_000_000_000, U32):
        b = a.with_uniform(eng, v)
        got = eng.intersect(b.set, b.set, "min")                 # cs: the operands' counter_max
        _, counts = got.download_sorted()
        assert len(got) == 3000 and (counts == v).all(), (v, counts[:4])
        assert (eng.simple(b.set, b.set, COUNTERS_SUBTRACT, "diff", U32).download()[0].shape[0]) == 0
        d = eng.simple(b.set, a.set, COUNTERS_SUBTRACT, "diff", U32).download()[1]
        assert (d == v - 1).all()
    # fan-in above 128: the partial sums must not stop at 2^31 - 1
    v = 2**31 // 100
    parts = [a.with_uniform(eng, v) for _ in range(129)]
    u = eng.union_sum([p.set for p in parts], U32)
    assert (u.download()[1] == 129 * v).all()
    u, h = eng.union_sum([p.set for p in parts], 200 * v, hist_len=16)
    assert (u.download()[1] == 129 * v).all() and int(h[15]) == 3000


# ---------------------------------------------------------------- binary operations
def pool_for(k, rng, n_uniform, nsets=2):
    """Distinct mixed keys: uniform ones, the four edge keys and runs on the slot boundaries the
    planner can pick for operands drawn from this pool."""
    W = words(k)
    if 4 ** k <= 4 * n_uniform:
        mixed = view_keys(np.arange(4 ** k, dtype=np.uint64), k)
    else:
        mixed = uniform_mixed(k, n_uniform, rng)
    est = planner_slots(int(1.3 * n_uniform), nsets, W)
    parts = [mixed, edge_mixed(k), boundary_mixed(k, rng, range(max(2, est - 3), est + 4))]
    v = np.unique(np.concatenate([key_view(p) for p in parts]))
    return view_keys(v, k)


@pytest.mark.parametrize("k", KS)
def test_binary_operations_on_constructed_sets(eng, k):
    rng = np.random.default_rng(100 + k)
    mixed = pool_for(k, rng, 6000)
    raw = unmix_np(k, mixed)
    n = raw.shape[0]
    ina = rng.random(n) < 0.7
    inb = rng.random(n) < 0.6
    ina[:2] = True                    # the edge keys (first and last mixed keys) in both operands
    inb[:2] = True
    ina[-2:] = True
    inb[-2:] = True
    ka, kb = raw[ina], raw[inb]
    a1, b1 = Operand(eng, k, ka), Operand(eng, k, kb)
    cfgs = [("one", a1, b1)]
    for i, v in enumerate(UNIFORM_V):
        cfgs.append((f"uni{v}", a1.with_uniform(eng, v), b1.with_uniform(eng, UNIFORM_V[(i + 2) % 6])))
    aa = Operand(eng, k, ka, counter_mix(rng, ka.shape[0], CS_LIST))
    ba = Operand(eng, k, kb, counter_mix(rng, kb.shape[0], CS_LIST))
    cfgs.append(("arrays", aa, ba))
    cfgs.append(("array-uniform", aa, b1.with_uniform(eng, 3_000_000_000)))
    for name, a, b in cfgs:
        run_binary_matrix(eng, k, a, b, CS_LIST, name)


@pytest.mark.parametrize("k", [1, 17, 32, 33, 64])
def test_binary_operations_nested_identical_disjoint_empty(eng, k):
    rng = np.random.default_rng(200 + k)
    raw = distinct_raw(k, np.concatenate([uniform_mixed(k, 5000, rng), edge_mixed(k)]))
    n = raw.shape[0]
    perm = rng.permutation(n)
    a = Operand(eng, k, raw, counter_mix(rng, n, CS_LIST))
    half = raw[perm[: n // 2]]
    nested = Operand(eng, k, half, counter_mix(rng, half.shape[0], CS_LIST))
    copy = Operand(eng, k, raw, a.counts)
    lo, hi = raw[perm[: n // 2]], raw[perm[n // 2:]]
    d1 = Operand(eng, k, lo, counter_mix(rng, lo.shape[0]))
    d2 = Operand(eng, k, hi).with_uniform(eng, 2**31)
    empty = Operand(eng, k, np.zeros((0, words(k)), dtype=np.uint64))
    cs_list = [1, 255, 2**31, U32]
    for name, x, y in [("nested", a, nested), ("nested-r", nested, a), ("same-handle", a, a),
                       ("identical", a, copy), ("disjoint", d1, d2), ("empty-r", a, empty),
                       ("empty-l", empty, a), ("both-empty", empty, empty)]:
        run_binary_matrix(eng, k, x, y, cs_list, name)


# ---------------------------------------------------------------- n-ary unions and histograms
@pytest.mark.parametrize("counted", [False, True])
@pytest.mark.parametrize("nsets", [1, 2, 3, 63, 64, 65, 127, 128, 129, 257])
def test_union_sum_and_histogram_at_every_fan_in(eng, nsets, counted):
    k = KS[(nsets + counted) % len(KS)]
    if k <= 2:
        k = 21 if counted else 41
    rng = np.random.default_rng(nsets * 2 + counted)
    pool = distinct_raw(k, np.concatenate([uniform_mixed(k, 2500, rng), edge_mixed(k)]))
    n = pool.shape[0]
    in_all = rng.random(n) < 0.03                     # some keys in every operand
    ops = []
    for g in range(nsets):
        sel = (rng.random(n) < rng.uniform(0.05, 0.6)) | in_all
        keys = pool[sel]
        if counted and g % 5 != 4:                    # a few uniform operands among counted ones
            ops.append(Operand(eng, k, keys, counter_mix(rng, keys.shape[0], HIST_LENS)))
        else:
            o = Operand(eng, k, keys)
            ops.append(o.with_uniform(eng, int(rng.integers(2, 600))) if counted else o)
    sets = [o.set for o in ops]
    keys, total = ref_union(k, ops)
    for hl in HIST_LENS:
        for cs in sorted({max(1, hl - 1), hl + 1, U32}):
            counts = np.minimum(total, cs)
            want = ref_hist(counts, hl)
            got, h = eng.union_sum(sets, cs, hist_len=hl)
            assert_set(got, keys, counts, ("union_sum", nsets, counted, hl, cs))
            assert (h == want).all(), ("union_sum hist", nsets, counted, hl, cs, np.nonzero(h != want)[0][:5])
            assert (got.histogram(hl) == want).all(), ("KmerSet.histogram", hl, cs)
            got.free()
            h2 = eng.union_histogram(sets, cs, hl)
            assert (h2 == want).all(), ("union_histogram", nsets, counted, hl, cs, np.nonzero(h2 != want)[0][:5])


def test_union_histogram_lds_descriptors_over_several_chains(eng):
    """65..128 operands (slice descriptors in LDS) and >= 128 slots: the histogram-only operation
    runs as several chains, so chains with slot0 != 0 read their operands through LDS."""
    k, nsets = 21, 100
    rng = np.random.default_rng(9)
    pool = distinct_raw(k, uniform_mixed(k, 40000, rng))
    ops = []
    for g in range(nsets):
        sel = rng.random(pool.shape[0]) < 0.1
        keys = pool[sel]
        ops.append(Operand(eng, k, keys, counter_mix(rng, keys.shape[0], HIST_LENS)) if g % 2 else Operand(eng, k, keys))
    total = sum(o.keys.shape[0] for o in ops)
    assert planner_slots(total, nsets, 1) >= 128
    sets = [o.set for o in ops]
    for hl, cs in [(16, 5000), (513, 5000), (5001, U32), (512, 100)]:
        keys, counts = ref_union(k, ops, cs)
        want = ref_hist(counts, hl)
        before = eng.stats()["setop_out"]
        got = eng.union_histogram(sets, cs, hl)
        assert (got == want).all(), (hl, cs, np.nonzero(got != want)[0][:5])
        assert eng.stats()["setop_out"] - before == keys.shape[0]
        u, h = eng.union_sum(sets, cs, hist_len=hl)
        assert_set(u, keys, counts, ("union_sum", hl, cs))
        assert (h == want).all()


@pytest.mark.parametrize("k", [15, 31, 33, 64])
def test_set_histogram_at_tier_edges(eng, k):
    rng = np.random.default_rng(300 + k)
    raw = distinct_raw(k, uniform_mixed(k, 20000, rng))
    c = counter_mix(rng, raw.shape[0], HIST_LENS)
    c[:600] = np.repeat(np.array([1, 14, 15, 16, 17, 510, 511, 512, 513, 5000, 5001, 5002], dtype=np.int64), 50)
    s = Operand(eng, k, raw, c)
    for hl in HIST_LENS:
        assert (s.set.histogram(hl) == ref_hist(c, hl)).all(), hl
        for v in (1, hl - 1, hl, U32):
            if v >= 1:
                assert (s.with_uniform(eng, v).set.histogram(hl) == ref_hist(np.full(raw.shape[0], v), hl)).all()


# ---------------------------------------------------------------- scale and order
@pytest.fixture(scope="module")
def big(eng):
    """Per W: two operands of 2.5 M keys sharing half of them, with counters over [1, 2^32 - 1]."""
    out = {}
    for k in (31, 47):
        rng = np.random.default_rng(k)
        pool = distinct_raw(k, uniform_mixed(k, 3_800_000, rng))
        n = pool.shape[0]
        perm = rng.permutation(n)
        a_idx, b_idx = perm[: 2 * n // 3], perm[n // 3:]
        ka, kb = pool[np.sort(a_idx)], pool[np.sort(b_idx)]
        out[k] = (ka, counter_mix(rng, ka.shape[0], CS_LIST), kb, counter_mix(rng, kb.shape[0], CS_LIST))
    return out


@pytest.mark.parametrize("k", [31, 47])
def test_large_operations_exact_in_index_and_ticket_order(eng, eng_tickets, big, k):
    ka, ca, kb, cb = big[k]
    p = Pair(k, ka, kb)
    results = {}
    for name, e in (("index", eng), ("ticket", eng_tickets)):
        a, b = Operand(e, k, ka, ca), Operand(e, k, kb, cb)
        assert e.stats()["order_fallbacks"] == 0
        for op, mode, cs in [(UNION, "sum", U32), (INTERSECT, "diff", 2**31), (COUNTERS_SUBTRACT, "diff", U32)]:
            keys, counts = p.result(p.combine(ca, cb, op, mode), cs)
            got = e.simple(a.set, b.set, op, mode, cs)
            assert_set(got, keys, counts, (name, k, op, mode, cs))
            results.setdefault((op, mode), []).append(got.download())
        one = Operand(e, k, ka).with_uniform(e, 1)
        u, h = e.union_sum([a.set, b.set, one.set], 5000, hist_len=513)
        keys, counts = ref_union(k, [a, b, one], 5000)
        assert_set(u, keys, counts, (name, k, "union3"))
        assert (h == ref_hist(counts, 513)).all()
    for key, (x, y) in results.items():
        assert (x[0] == y[0]).all() and (x[1] == y[1]).all(), key


def test_tiny_operand_against_millions(eng, big):
    k = 31
    ka, ca, _, _ = big[k]
    huge = Operand(eng, k, ka, ca)
    rng = np.random.default_rng(3)
    outside = distinct_raw(k, uniform_mixed(k, 50, rng))
    outside = outside[~np.isin(key_view(outside), key_view(ka))][:2]
    tk = np.concatenate([ka[[len(ka) // 2]], outside])
    tiny = Operand(eng, k, tk, np.array([2**31 + 5, 7, U32], dtype=np.int64))
    for x, y in [(tiny, huge), (huge, tiny)]:
        p = Pair(k, x.keys, y.keys)
        for op, mode in [(UNION, "sum"), (INTERSECT, "min"), (INTERSECT, "right"), (KMERS_SUBTRACT, "left"),
                         (COUNTERS_SUBTRACT, "diff")]:
            keys, counts = p.result(p.combine(x.counts, y.counts, op, mode), U32)
            assert_set(eng.simple(x.set, y.set, op, mode, U32), keys, counts, (op, mode, len(x.keys)))


# ---------------------------------------------------------------- re-plans
@pytest.mark.parametrize("R", [2, 8, 64])
def test_clustered_operands_replan_and_stay_exact(eng, R):
    """Slices confined to 1/R of the mixed key space (the receive side of the key-set exchange):
    the first plan spreads slots over the whole space, overflows and re-plans."""
    rng = np.random.default_rng(R)
    for k in (31, 47):
        start = int(rng.integers(0, (1 << 32) - (1 << 32) // R))
        pool = distinct_raw(k, clustered_mixed(k, 300_000, rng, 1.0 / R, start))
        ops = []
        for g in range(3):
            sel = rng.random(pool.shape[0]) < 0.5
            ops.append(Operand(eng, k, pool[sel], counter_mix(rng, int(sel.sum()))) if g else Operand(eng, k, pool[sel]))
        before = eng.stats()["retries"]
        keys, counts = ref_union(k, ops, 5000)
        u, h = eng.union_sum([o.set for o in ops], 5000, hist_len=17)
        assert_set(u, keys, counts, ("cluster", R, k))
        assert (h == ref_hist(counts, 17)).all()
        assert (eng.union_histogram([o.set for o in ops], 5000, 17) == h).all()
        if R >= 8:
            assert eng.stats()["retries"] > before, (R, k)
        p = Pair(k, ops[1].keys, ops[2].keys)
        keys, counts = p.result(p.combine(ops[1].counts, ops[2].counts, COUNTERS_SUBTRACT, "diff"), U32)
        assert_set(eng.simple(ops[1].set, ops[2].set, COUNTERS_SUBTRACT, "diff", U32), keys, counts, ("cluster-sub", R, k))


def _engine_still_works(eng):
    k = 33
    rng = np.random.default_rng(1)
    a = Operand(eng, k, distinct_raw(k, uniform_mixed(k, 1000, rng)), None)
    keys, counts = ref_union(k, [a, a], 255)
    assert_set(eng.union_sum([a.set, a.set], 255), keys, counts, "after capacity failure")


@pytest.mark.parametrize("k", [23, 31, 33, 64])
def test_more_than_cap_keys_on_one_top32_fail_cleanly(eng, E, k):
    W = words(k)
    cap = 4096 if W == 1 else 2048
    rng = np.random.default_rng(k)
    top = np.full(cap * 3 // 2, int(rng.integers(0, 1 << 32)), dtype=np.uint64)
    raw = distinct_raw(k, mixed_from_top32(k, top, rng))
    assert raw.shape[0] > cap
    s = Operand(eng, k, raw)
    for call in (lambda: eng.union_sum([s.set], 255), lambda: eng.union_histogram([s.set, s.set], 255, 8),
                 lambda: eng.simple(s.set, s.set, INTERSECT, "min", 255)):
        with pytest.raises(E.KhoiceError) as ei:
            call()
        assert ei.value.code == E_CAPACITY
    _engine_still_works(eng)


@pytest.mark.parametrize("k", [31, 47])
def test_cluster_below_the_planner_floor(eng, E, k):
    """The slot target used to stop at 16 keys, and a set confined to 1/1024 of the space failed with KH_E_CAPACITY.
    The re-plan now goes down to one key per range: such a set, alone and united with itself, and one confined to
    1/256 of the space are answered exactly."""
    rng = np.random.default_rng(k + 5)
    tight = Operand(eng, k, distinct_raw(k, clustered_mixed(k, 120_000, rng, 1.0 / 1024, 12345)))
    r0 = eng.stats()["retries"]
    for ops in ([tight], [tight, tight]):
        u = eng.union_sum([o.set for o in ops], 255)
        keys, counts = ref_union(k, ops, 255)
        assert_set(u, keys, counts, "1/1024 cluster")
    assert eng.stats()["retries"] > r0                          # the first plan cannot hold it: it was re-planned
    _engine_still_works(eng)
    loose = Operand(eng, k, distinct_raw(k, clustered_mixed(k, 120_000, rng, 1.0 / 256, 1 << 31)))
    u = eng.union_sum([loose.set, loose.set], 255)
    keys, counts = ref_union(k, [loose, loose], 255)
    assert_set(u, keys, counts, "1/256 cluster")
    _engine_still_works(eng)
