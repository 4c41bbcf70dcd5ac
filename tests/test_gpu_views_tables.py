"""GPU: what the multi-GPU step (khoice_amd/dist.py) and experiment type 4 rest on, on CONSTRUCTED inputs:
  a. k_membership / membership_compute / kh_confusion_row: operands clustered in mixed space, so the interpolated
     window misses on either side and the search falls back to the whole set; every fan-in word boundary;
  b. k_table_add / k_table_hist: tables whose cells the test writes itself, every range shape and histogram tier;
  c. kh_set(s)_partition_bounds, kh_set_export_range / _device, kh_set_wrap_device, kh_set_from_device,
     kh_set_device_ptrs: the key-set exchange of dist.py carried out rank by rank in one process.
Every comparison is exact, against a few lines of numpy (kh_confusion_row: oracle/merge_oracle.py, bit for bit).

The unmarked tests prove the planted inputs on the CPU: that the window of k_membership really misses, on the left
for some pivot keys and on the right for others, and that the boundary keys sit on and one below every slot edge.

Limits, stated: partition bounds are read back for up to 2^20 parts (2^32 - 1 parts is an array of 32 GiB on either
side); the table histogram's grid cap is reached with one-byte cells only."""
import bisect
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import merge_oracle as MO
from tests.util import (MASK64, U32, boundary_mixed, clustered_mixed, counter_mix, distinct_raw, edge_mixed,
                        key_view, mix_np, mixed_from_top32, ref_hist, slot_np, top32_np, uniform_mixed, unmix_np,
                        view_keys, words)

KS = [1, 5, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64]
FAN_INS = [0, 1, 63, 64, 65, 127, 128, 129, 200]
NPARTS = [1, 2, 3, 7, 8, 64, 1000, 65536, 1 << 20]
EDGE_NPARTS = [2, 3, 7, 8, 64, 1000]              # every slot edge of these is planted; a sample for the larger ones
WORLDS = [1, 2, 3, 7, 8]
CS_LIST = [0, 1, 2, 15, 16, 255, 5000, U32]       # 0: no ceiling
HIST_LENS = [2, 15, 16, 17, 511, 512, 513, 5001]
E_ARG = -1


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
def torch():
    import torch as t
    return t


# ---------------------------------------------------------------- keys
def ints_to_keys(k, vals):
    out = np.zeros((len(vals), words(k)), dtype=np.uint64)
    for i, v in enumerate(vals):
        out[i, 0] = v & MASK64
        if words(k) == 2:
            out[i, 1] = v >> 64
    return out


def keys_to_ints(keys):
    if keys.shape[1] == 1:
        return [int(x) for x in keys[:, 0]]
    return [int(lo) | (int(hi) << 64) for lo, hi in zip(keys[:, 0], keys[:, 1])]


def uniq(k, *parts):
    """Distinct keys[n, W] of the parts, ascending."""
    parts = [p for p in parts if p.shape[0]]
    if not parts:
        return np.zeros((0, words(k)), dtype=np.uint64)
    return view_keys(np.unique(np.concatenate([key_view(p) for p in parts])), k)


def member(pv, sv):
    """bool[len(pv)]: pv[i] occurs in sv (key_view arrays)."""
    if not sv.shape[0]:
        return np.zeros(pv.shape[0], dtype=bool)
    u, inv = np.unique(np.concatenate([sv, pv]), return_inverse=True)
    inv = inv.reshape(-1)
    has = np.zeros(u.shape[0], dtype=bool)
    has[inv[:sv.shape[0]]] = True
    return has[inv[sv.shape[0]:]]


def lower_bound(k, op_sorted, keys):
    """Index of the first key of op_sorted (ascending mixed keys) that is not below keys[i]."""
    if words(k) == 1:
        return np.searchsorted(op_sorted[:, 0], keys[:, 0], side="left").astype(np.int64)
    ops = keys_to_ints(op_sorted)
    return np.array([bisect.bisect_left(ops, v) for v in keys_to_ints(keys)], dtype=np.int64)


# ---------------------------------------------------------------- a. membership: the planted case
CLUSTERS = ("low", "high", "mid")
OPERAND_ORDER = ("uniform_a", "low", "high", "mid", "one", "empty", "pivot_copy", "extremes", "uniform_b")


@functools.lru_cache(maxsize=None)
def membership_case(k):
    """Operands and pivot in MIXED space (ascending, distinct).  The clusters take 1 % of the space (a quarter of it
    while 4^k is small): for a key inside or beside one, the interpolation of k_membership, which takes the operand for
    uniform, lands far from the answer."""
    rng = np.random.default_rng(5000 + k)
    space = 4 ** k
    frac = 0.01 if k >= 15 else 0.25
    width = int((1 << 32) * frac)
    nu = max(1, min(3000, space // 3))
    ops = {
        "uniform_a": uniq(k, uniform_mixed(k, nu, rng)),
        "uniform_b": uniq(k, uniform_mixed(k, max(1, nu // 3), rng)),
        "low": uniq(k, clustered_mixed(k, 20000, rng, frac, 0)),
        "high": uniq(k, clustered_mixed(k, 20000, rng, frac, (1 << 32) - width)),
        "mid": uniq(k, clustered_mixed(k, 20000, rng, frac, (1 << 31) - width // 2)),
        "one": uniq(k, uniform_mixed(k, 1, rng)),
        "empty": np.zeros((0, words(k)), dtype=np.uint64),
        "extremes": ints_to_keys(k, sorted({0, space - 1})),
    }
    beside = set()
    for m in ops.values():            # first and last key of every operand, and the keys just below and above them
        if m.shape[0]:
            for v in keys_to_ints(m[[0, -1]]):
                beside.update(x for x in (v - 1, v, v + 1) if 0 <= x < space)
    inside = [ops[c][::13] for c in CLUSTERS]
    absent = uniform_mixed(k, min(2000, space), rng)
    pivot = uniq(k, ints_to_keys(k, sorted(beside)), absent, *inside)
    ops["pivot_copy"] = pivot.copy()
    return ops, pivot


def window(k, op, pivot):
    """est and rad of k_membership for every pivot key against one operand, and the true lower bound."""
    n = op.shape[0]
    est = ((top32_np(k, pivot) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)      # __umul64hi(top32 << 32, n)
    rad = int(np.float32(4.0) * np.sqrt(np.float32(n))) + 64                           # 4.0f * sqrtf((float)n) + 64
    return est, rad, lower_bound(k, op, pivot)


@pytest.mark.parametrize("k", KS)
def test_cpu_membership_window_misses_on_both_sides(k):
    ops, pivot = membership_case(k)
    assert [name for name in OPERAND_ORDER if name not in ops] == []
    margin = 8
    for name in ("uniform_a", "uniform_b", "one", "extremes"):
        est, rad, lb = window(k, ops[name], pivot)
        assert ((lb >= est - rad) & (lb <= est + rad)).all(), (k, name)
    if k == 1:                        # 4 keys: every window is the whole set
        return
    need = 50 if k >= 15 else 3
    left, right = {}, {}
    for name in CLUSTERS:
        op = ops[name]
        n = op.shape[0]
        est, rad, lb = window(k, op, pivot)
        left[name] = int(((est - rad > 0) & (lb < est - rad - margin)).sum())
        right[name] = int(((est + rad < n) & (lb > est + rad + margin)).sum())
        # keys of the pivot inside the cluster are among them
        assert member(key_view(pivot), key_view(op)).sum() >= n // 13
    assert right["low"] >= need and left["high"] >= need, (k, left, right)
    if k >= 15:                       # (a quarter of 1024 keys in the middle is too close to uniform to miss)
        assert left["mid"] >= need and right["mid"] >= need, (k, left, right)
    # the pivot copy is searched with its own keys: both kinds of cluster are in it, so both sides miss there too
    est, rad, lb = window(k, ops["pivot_copy"], pivot)
    if k >= 15:
        assert int((lb < est - rad - margin).sum()) >= need and int((lb > est + rad + margin).sum()) >= need


def ref_masks(pv, set_views):
    """Python int per pivot key: bit d = set d holds it."""
    masks = [0] * pv.shape[0]
    for d, sv in enumerate(set_views):
        for i in np.nonzero(member(pv, sv))[0]:
            masks[i] |= 1 << d
    return masks


def got_masks(masks):
    return [sum(int(masks[i, w]) << (64 * w) for w in range(masks.shape[1])) for i in range(masks.shape[0])]


def check_membership(eng, k, pivot_set, piv_raw_sorted, counts_sorted, sets, set_raws, what):
    """membership + confusion_row of one pivot handle against numpy / the oracle, on every pivot key."""
    keys, counts, masks = eng.membership(pivot_set, sets)
    n = piv_raw_sorted.shape[0]
    assert keys.shape == piv_raw_sorted.shape and masks.shape == (n, max(1, (len(sets) + 63) // 64)), what
    assert (keys == piv_raw_sorted).all(), (what, "keys are not the pivot's in ascending canonical order")
    assert (counts.astype(np.int64) == counts_sorted).all(), (what, "counts do not follow their keys")
    pv = key_view(piv_raw_sorted)
    want = ref_masks(pv, [key_view(r) for r in set_raws])
    got = got_masks(masks)
    bad = [i for i in range(n) if got[i] != want[i]]
    assert not bad, (what, "mask", bad[0], hex(got[bad[0]]), hex(want[bad[0]]), len(bad))
    codes = keys_to_ints(piv_raw_sorted)
    pivot_db = dict(zip(codes, (int(c) for c in counts_sorted)))
    set_dbs = [dict.fromkeys(keys_to_ints(r), 1) for r in set_raws]
    want_row, want_unique = MO.confusion_row(pivot_db, set_dbs)
    row, unique = eng.confusion_row(pivot_set, sets)
    assert unique == want_unique, (what, unique, want_unique)
    assert row.tolist() == list(want_row), (what, "confusion row differs", row.tolist()[:4], list(want_row)[:4])
    return want


def sorted_pivot(k, piv_raw, counts):
    order = np.argsort(key_view(piv_raw), kind="stable")
    return piv_raw[order], np.asarray(counts, dtype=np.int64)[order]


def wrapped_copy(eng, torch, k, s, pad=1):
    """A zero-copy set over a larger torch buffer into which `s` was exported `pad` records in (an odd offset)."""
    n, w = len(s), words(k)
    kbuf = torch.full(((n + 2 * pad + 1) * w,), -1, dtype=torch.int64, device="cuda:0")
    cbuf = torch.full((n + 2 * pad + 1,), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    s.export_device(kbuf.data_ptr() + 8 * w * pad, cbuf.data_ptr() + 4 * pad)
    return eng.wrap_device(k, n, kbuf.data_ptr() + 8 * w * pad, cbuf.data_ptr() + 4 * pad), (kbuf, cbuf)


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_membership_on_clustered_operands(eng, torch, k):
    ops, pivot = membership_case(k)
    rng = np.random.default_rng(k)
    set_raws = [unmix_np(k, ops[name]) for name in OPERAND_ORDER]
    sets = [eng.upload(k, r[rng.permutation(r.shape[0])]) for r in set_raws]
    piv_raw = unmix_np(k, pivot)
    n = piv_raw.shape[0]
    counts = counter_mix(rng, n)
    counts[:3] = [U32, 1, 2**31][:min(3, n)]
    counted = eng.upload(k, piv_raw, counts.astype(np.uint32))
    keys_s, counts_s = sorted_pivot(k, piv_raw, counts)
    want = check_membership(eng, k, counted, keys_s, counts_s, sets, set_raws, (k, "counted"))
    copy_bit = 1 << OPERAND_ORDER.index("pivot_copy")
    assert all(m & copy_bit for m in want)                            # the reference itself: every key is in the copy
    assert any(m == copy_bit for m in want) or k < 15                 # ... and some are in nothing else
    uniform = eng.upload(k, piv_raw).set_counts(7)
    check_membership(eng, k, uniform, keys_s, np.full(n, 7), sets, set_raws, (k, "uniform"))
    wrapped, keep = wrapped_copy(eng, torch, k, counted)
    check_membership(eng, k, wrapped, keys_s, counts_s, sets, set_raws, (k, "wrapped"))
    del keep


@pytest.mark.gpu
@pytest.mark.parametrize("nsets", FAN_INS)
def test_membership_at_every_fan_in(eng, nsets):
    for k in (21, 47):
        rng = np.random.default_rng(100 * nsets + k)
        pool = distinct_raw(k, np.concatenate([uniform_mixed(k, 1500, rng), edge_mixed(k)]))
        others = distinct_raw(k, uniform_mixed(k, 300, rng))
        n = pool.shape[0]
        hold = rng.random((nsets, n)) < rng.uniform(0.02, 0.5, size=(nsets, 1))
        hold[:, :40] = False
        if nsets >= 7:                    # shares that are no power of two: keys held by exactly 3 and by exactly 7 sets
            hold[[0, nsets // 2, nsets - 1], 0] = True
            hold[np.linspace(0, nsets - 1, 7).astype(int), 1] = True
        if nsets >= 65:                   # keys whose bits 63 and 64 differ, either way, and keys in the last set only
            hold[63, 2], hold[64, 3] = True, True
            hold[nsets - 1, 4] = True
        set_raws = [np.concatenate([pool[hold[d]], others[rng.random(others.shape[0]) < 0.3]]) for d in range(nsets)]
        sets = [eng.upload(k, r) for r in set_raws]
        counts = counter_mix(rng, n)
        pivot = eng.upload(k, pool, counts.astype(np.uint32))
        keys_s, counts_s = sorted_pivot(k, pool, counts)
        want = check_membership(eng, k, pivot, keys_s, counts_s, sets, set_raws, (k, nsets))
        pop = [bin(m).count("1") for m in want]
        assert 0 in pop
        if nsets >= 7:
            assert 3 in pop and 7 in pop
        if nsets >= 65:
            assert any((m >> 63) & 1 and not (m >> 64) & 1 for m in want)
            assert any((m >> 64) & 1 and not (m >> 63) & 1 for m in want)
            assert any(m == 1 << (nsets - 1) for m in want)


# ---------------------------------------------------------------- b. occurrence table
def ref_table_hist(cells, cs, hist_len):
    c = np.asarray(cells)
    c = c[c > 0].astype(np.int64)
    if cs:
        c = np.minimum(c, cs)
    return np.bincount(np.minimum(c, hist_len - 1), minlength=hist_len).astype(np.uint64)


def written_cells(cell_bytes, rng):
    """A few thousand cells: every tier value, runs of zeros, and 16-byte vectors that are zero but for one byte."""
    per = 16 // cell_bytes
    values = [0, 1, 15, 16, 17, 255]
    if cell_bytes == 4:
        values += [511, 512, 513, 5000, 5001, 2**31, 2**32 - 1]
    parts = [rng.choice(np.array(values, dtype=np.uint64), size=2048),
             np.zeros(512, dtype=np.uint64)]
    for b in range(16):               # one non-zero BYTE of a vector, in each of its 16 positions
        v = np.zeros(per, dtype=np.uint64)
        v[b // cell_bytes] = 1 + b if cell_bytes == 1 else (0xA1 + b) << (8 * (b % 4))
        parts += [v, np.zeros(per * int(rng.integers(0, 3)), dtype=np.uint64)]
    sparse = np.zeros(1024, dtype=np.uint64)
    idx = rng.choice(1024, size=40, replace=False)
    sparse[idx] = rng.choice(np.array(values[1:], dtype=np.uint64), size=40)
    parts += [sparse, rng.choice(np.array(values, dtype=np.uint64), size=37)]      # the table ends off a vector
    return np.concatenate(parts)


def upload_cells(torch, cells, cell_bytes):
    if cell_bytes == 1:
        t = torch.from_numpy(cells.astype(np.uint8)).to("cuda:0")
    else:
        t = torch.from_numpy(cells.astype(np.uint32).view(np.int32)).to("cuda:0")
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0
    return t


def range_shapes(per, ncell):
    """(lo, hi) with lo at the vector alignments within 128 bytes and every range length the kernel distinguishes."""
    lens = sorted(set([0] + list(range(1, 16)) + [per - 1, per, per + 1] +
                      [m * per + t for m in (3, 64) for t in range(0, 16)]))
    out = []
    for a in (0, 1, 2, 3, 4, 5, 7, 8):
        out += [(a * per, a * per + ln) for ln in lens]
    out += [(ncell - ln, ncell) for ln in lens if (ncell - ln) % per == 0] + [(0, ncell)]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("cell_bytes", [1, 4])
def test_table_histogram_of_written_cells(eng, torch, cell_bytes):
    rng = np.random.default_rng(cell_bytes)
    cells = written_cells(cell_bytes, rng)
    ncell, per = cells.shape[0], 16 // cell_bytes
    assert ncell % per != 0
    table = upload_cells(torch, cells, cell_bytes)
    for lo, hi in range_shapes(per, ncell):
        got = eng.table_histogram(table.data_ptr(), cell_bytes, lo, hi, 0, 5001)
        want = ref_table_hist(cells[lo:hi], 0, 5001)
        assert (got == want).all(), (cell_bytes, lo, hi, np.nonzero(got != want)[0][:5])
    for lo, hi in [(0, ncell), (3 * per, ncell - 5), (2048 - per, 2048 + 600)]:
        for cs in CS_LIST:
            for hl in HIST_LENS:
                got = eng.table_histogram(table.data_ptr(), cell_bytes, lo, hi, cs, hl)
                want = ref_table_hist(cells[lo:hi], cs, hl)
                assert (got == want).all(), (cell_bytes, lo, hi, cs, hl, np.nonzero(got != want)[0][:5])
    assert (table.cpu().numpy().view(np.uint8 if cell_bytes == 1 else np.uint32) == cells).all()


@pytest.mark.gpu
@pytest.mark.parametrize("cell_bytes,ncell", [(1, (1 << 20) + 16 * 7 + 3), (4, (1 << 20) + 4 * 7 + 3),
                                              (1, 16 * (4096 * 1024 + 1000) + 5)])
def test_table_histogram_over_several_blocks(eng, torch, cell_bytes, ncell):
    """More than one block of 1024 vectors; the last case is past the grid cap of 4096 blocks, where a block strides."""
    rng = np.random.default_rng(ncell % 1000)
    values = np.array([1, 2, 15, 16, 17, 255] + ([511, 512, 513, 5000, 5001, 2**32 - 1] if cell_bytes == 4 else []),
                      dtype=np.uint8 if cell_bytes == 1 else np.uint32)
    cells = np.zeros(ncell, dtype=values.dtype)
    idx = rng.integers(0, ncell, size=ncell // 50)
    cells[idx] = values[rng.integers(0, values.shape[0], size=idx.shape[0])]
    cells[-3:] = [255, 0, 7]
    cells[ncell // 2: ncell // 2 + 3000] = values[rng.integers(0, values.shape[0], size=3000)]     # a dense stretch
    table = upload_cells(torch, cells, cell_bytes)
    per = 16 // cell_bytes
    for lo, hi, cs, hl in [(0, ncell, 5000, 5001), (per * 999, ncell, 16, 17), (0, ncell - 9, 0, 512)]:
        got = eng.table_histogram(table.data_ptr(), cell_bytes, lo, hi, cs, hl)
        want = ref_table_hist(cells[lo:hi], cs, hl)
        assert (got == want).all(), (cell_bytes, ncell, lo, hi, cs, hl, np.nonzero(got != want)[0][:5])


def table_cells(torch, table, cell_bytes):
    torch.cuda.synchronize()
    return table.cpu().numpy().view(np.uint8 if cell_bytes == 1 else np.uint32).astype(np.int64)


@pytest.mark.gpu
def test_table_add_saturates_at_the_cell_width(eng, torch):
    k = 5
    rng = np.random.default_rng(55)
    codes = np.unique(np.concatenate([rng.choice(4 ** k, size=300, replace=False), [0, 4 ** k - 1]])).astype(np.uint64)
    on = np.zeros(4 ** k, dtype=bool)
    on[codes.astype(np.int64)] = True
    plain = eng.upload(k, codes.reshape(-1, 1))
    counted = eng.upload(k, codes.reshape(-1, 1), counter_mix(rng, codes.shape[0]).astype(np.uint32))
    nine = plain.set_counts(9)
    forms = [plain, counted, nine]        # a cell counts SETS: counters, uniform or not, do not enter
    table = torch.zeros(4 ** k, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    done = 0
    for times in (1, 2, 3, 254, 255, 256, 300):
        while done < times:
            eng.table_add_set(forms[done % 3], table.data_ptr(), 1)
            done += 1
        eng.sync()
        cells = table_cells(torch, table, 1)
        assert (cells == np.where(on, min(times, 255), 0)).all(), times
    h = eng.table_histogram(table.data_ptr(), 1, 0, 4 ** k, 0, 300)
    assert int(h[255]) == codes.shape[0] and int(h.sum()) == codes.shape[0]
    # four-byte cells stop at 2^32 - 1
    start = np.where(on, 2**32 - 2, 3).astype(np.uint32)
    table4 = upload_cells(torch, start, 4)
    for times, top in ((1, 2**32 - 1), (2, 2**32 - 1)):
        eng.table_add_set(forms[times], table4.data_ptr(), 4)
        eng.sync()
        assert (table_cells(torch, table4, 4) == np.where(on, top, 3)).all(), times
    h = eng.table_histogram(table4.data_ptr(), 4, 0, 4 ** k, 0, 5001)
    assert int(h[3]) == 4 ** k - codes.shape[0] and int(h[5000]) == codes.shape[0]


@pytest.mark.gpu
@pytest.mark.parametrize("cell_bytes", [1, 4])
def test_table_of_four_cells_and_of_4_16_cells(eng, torch, cell_bytes):
    dtype = torch.uint8 if cell_bytes == 1 else torch.int32
    # k = 1: the whole table is shorter than one 16-byte vector
    table = torch.zeros(4, dtype=dtype, device="cuda:0")
    torch.cuda.synchronize()
    a = eng.upload(1, np.array([[0], [3]], dtype=np.uint64))
    b = eng.upload(1, np.array([[3]], dtype=np.uint64), np.array([U32], dtype=np.uint32))
    for s in (a, b, a):
        eng.table_add_set(s, table.data_ptr(), cell_bytes)
    eng.table_add_set(eng.upload(1, np.zeros((0, 1), dtype=np.uint64)), table.data_ptr(), cell_bytes)
    eng.sync()
    assert table_cells(torch, table, cell_bytes).tolist() == [2, 0, 0, 3]
    assert eng.table_histogram(table.data_ptr(), cell_bytes, 0, 4, 0, 5).tolist() == [0, 0, 1, 1, 0]
    assert eng.table_histogram(table.data_ptr(), cell_bytes, 0, 4, 2, 5).tolist() == [0, 0, 2, 0, 0]
    assert eng.table_histogram(table.data_ptr(), cell_bytes, 0, 1, 0, 2).tolist() == [0, 1]
    if cell_bytes == 4:
        return
    # k = 16: 4^16 one-byte cells, a small set that holds the first and the last cell
    k = 16
    rng = np.random.default_rng(16)
    raw = distinct_raw(k, np.concatenate([uniform_mixed(k, 5000, rng), mix_np(k, edge_mixed(k))]))
    assert raw[:, 0].min() == 0 and raw[:, 0].max() == 4 ** k - 1
    s, half = eng.upload(k, raw), eng.upload(k, raw[::2])
    table = torch.zeros(4 ** k, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    eng.table_add_set(s, table.data_ptr(), 1)
    eng.table_add_set(half, table.data_ptr(), 1)
    eng.sync()
    idx = torch.from_numpy(raw[:, 0].astype(np.int64)).to("cuda:0")
    want = np.ones(raw.shape[0], dtype=np.int64)
    want[::2] = 2
    assert (table[idx].cpu().numpy() == want).all()
    assert int(torch.count_nonzero(table)) == raw.shape[0]
    lo = (4 ** k // 3) // 16 * 16
    h = sum(eng.table_histogram(table.data_ptr(), 1, a_, b_, 0, 4) for a_, b_ in ((0, lo), (lo, 4 ** k)))
    assert h.tolist() == [0, raw.shape[0] // 2, (raw.shape[0] + 1) // 2, 0]


@pytest.mark.gpu
def test_table_calls_refused_leave_the_table_alone(eng, E, torch):
    rng = np.random.default_rng(3)
    cells = rng.integers(0, 256, size=4 ** 5).astype(np.uint8)
    table = upload_cells(torch, cells, 1)
    small = eng.upload(5, np.array([[1], [7]], dtype=np.uint64))
    big = eng.upload(17, np.array([[1], [7]], dtype=np.uint64))
    calls = [lambda: eng.table_add_set(big, table.data_ptr(), 1),
             lambda: eng.table_add_set(small, table.data_ptr(), 2),
             lambda: eng.table_histogram(table.data_ptr(), 2, 0, 64, 0, 16),
             lambda: eng.table_histogram(table.data_ptr(), 1, 8, 64, 0, 16),
             lambda: eng.table_histogram(table.data_ptr(), 4, 2, 64, 0, 16),
             lambda: eng.table_histogram(table.data_ptr(), 1, 64, 48, 0, 16),
             lambda: eng.table_histogram(table.data_ptr() + 4, 1, 0, 64, 0, 16),
             lambda: eng.table_histogram(table.data_ptr(), 1, 0, 64, 0, 1)]
    for i, call in enumerate(calls):
        with pytest.raises(E.KhoiceError) as ei:
            call()
        assert ei.value.code == E_ARG, i
    eng.sync()
    assert (table_cells(torch, table, 1) == cells).all()
    assert (eng.table_histogram(table.data_ptr(), 1, 16, 64, 0, 256) == ref_table_hist(cells[16:64], 0, 256)).all()


# ---------------------------------------------------------------- c. slices and views
def sampled_edge_mixed(k, rng, nparts, nsample=150):
    """boundary_mixed for a sample of the slot edges of a large slot count (the first and the last among them)."""
    r = np.unique(np.concatenate([[1, nparts - 1], rng.integers(1, nparts, size=nsample)]))
    t = np.array([-(-(int(x) << 32) // nparts) for x in r], dtype=np.uint64)
    return mixed_from_top32(k, np.concatenate([t, t - np.uint64(1)]), rng)


@functools.lru_cache(maxsize=None)
def bounds_sets(k):
    """Mixed keys (ascending, distinct) of the sets whose slot bounds are tested; None stands for an empty set."""
    rng = np.random.default_rng(7000 + k)
    edges = uniq(k, boundary_mixed(k, rng, EDGE_NPARTS, per=2), sampled_edge_mixed(k, rng, 65536),
                 sampled_edge_mixed(k, rng, 1 << 20), edge_mixed(k))
    cluster = uniq(k, clustered_mixed(k, 4000, rng, 0.01, int(0.37 * (1 << 32))))
    empty = np.zeros((0, words(k)), dtype=np.uint64)
    return [empty, edges, edge_mixed(k), empty, cluster, uniq(k, uniform_mixed(k, 1, rng)), empty]


def ref_bounds(k, mixed_sorted, nparts):
    slot = slot_np(k, mixed_sorted, nparts)
    b = np.searchsorted(slot, np.arange(nparts + 1, dtype=np.uint64), side="left").astype(np.uint64)
    b[0], b[nparts] = 0, mixed_sorted.shape[0]
    return b


@pytest.mark.parametrize("k", KS)
def test_cpu_boundary_keys_sit_on_every_slot_edge(k):
    sets = bounds_sets(k)
    assert [s.shape[0] == 0 for s in sets] == [True, False, False, True, False, False, True]
    edges = sets[1]
    tops = top32_np(k, edges)
    assert (np.diff(slot_np(k, edges, 1000).astype(np.int64)) >= 0).all()          # ascending keys, ascending slots
    if 2 * k < 32:                    # fewer than 32 key bits: the top 32 bits move in steps, the edges are rounded down
        return
    for n in EDGE_NPARTS:
        r = np.arange(1, n, dtype=np.uint64)
        t = np.array([-(-(int(x) << 32) // n) for x in r], dtype=np.uint64)
        assert np.isin(t, tops).all() and np.isin(t - np.uint64(1), tops).all(), (k, n)
        assert ((t * np.uint64(n)) >> np.uint64(32) == r).all()                     # first top-32 value of slot r
        assert (((t - np.uint64(1)) * np.uint64(n)) >> np.uint64(32) == r - np.uint64(1)).all()   # last of slot r - 1
    for n in (65536, 1 << 20):
        s = slot_np(k, edges, n)
        first = (top32_np(k, edges) - np.uint64(1)) * np.uint64(n) >> np.uint64(32) != s
        assert int((first & (tops > 0)).sum()) >= 100, (k, n)                       # keys on the first value of a slot
    assert keys_to_ints(sets[2])[0] == 0 and keys_to_ints(sets[2])[-1] == 4 ** k - 1


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_partition_bounds_on_slot_edges(eng, k):
    mixed = bounds_sets(k)
    sets = [eng.upload(k, unmix_np(k, m)) for m in mixed]
    for nparts in NPARTS:
        want = [ref_bounds(k, m, nparts) for m in mixed]
        got = eng.partition_bounds(sets, nparts)
        assert got.shape == (len(sets), nparts + 1)
        for i in range(len(sets)):
            assert (got[i] == want[i]).all(), (k, nparts, i, np.nonzero(got[i] != want[i])[0][:5])
        for i in (0, 1, 2, 4, 6) if nparts <= 65536 else (1,):
            one = sets[i].partition_bounds(nparts)
            assert (one == want[i]).all(), (k, nparts, i, "single", np.nonzero(one != want[i])[0][:5])
        assert (eng.partition_bounds(sets[1:2], nparts)[0] == want[1]).all()        # one set in one call


@pytest.mark.gpu
def test_partition_bounds_of_130_sets_and_null_handles(eng, E):
    for k in (31, 33):
        rng = np.random.default_rng(k)
        mixed = [uniq(k, uniform_mixed(k, int(rng.integers(0, 400)) if i % 11 else 0, rng)) for i in range(130)]
        sets = [eng.upload(k, unmix_np(k, m)) for m in mixed]
        for nparts in (1, 7, 1000):
            got = eng.partition_bounds(sets, nparts)
            for i, m in enumerate(mixed):
                assert (got[i] == ref_bounds(k, m, nparts)).all(), (k, nparts, i)
    # a NULL handle, first or later, is a bad argument and nothing is written
    lib = E.load_library()
    for arr in ((C.c_void_p * 2)(None, sets[1]._h), (C.c_void_p * 2)(sets[1]._h, None)):
        out = np.full(2 * 4, 77, dtype=np.uint64)
        rc = lib.kh_sets_partition_bounds(eng._ctx, arr, 2, 3, out.ctypes.data_as(C.POINTER(C.c_uint64)))
        assert rc == E_ARG and (out == 77).all()
    other = eng.upload(21, np.array([[5]], dtype=np.uint64))
    with pytest.raises(E.KhoiceError) as ei:
        eng.partition_bounds([sets[1], other], 3)
    assert ei.value.code != E_ARG                                                    # a k mismatch keeps its own code


def stored(k, raw, counts):
    """What the engine stores for an uploaded set: (mixed keys ascending, their counters)."""
    mixed = mix_np(k, raw)
    order = np.argsort(key_view(mixed), kind="stable")
    return mixed[order], np.asarray(counts, dtype=np.int64)[order]


def export_checked(eng, torch, k, s, mixed, counts, lo, hi, with_counts):
    w, n = words(k), hi - lo
    kbuf = torch.full(((n + 2) * w,), -1, dtype=torch.int64, device="cuda:0")
    cbuf = torch.full((n + 2,), -1, dtype=torch.int32, device="cuda:0") if with_counts else None
    torch.cuda.synchronize()
    s.export_range(lo, hi, kbuf.data_ptr(), cbuf.data_ptr() if with_counts else None)
    eng.sync()
    gk = kbuf.cpu().numpy().view(np.uint64).reshape(-1, w)
    assert (gk[:n] == mixed[lo:hi]).all(), (k, lo, hi, "keys")
    assert (gk[n:] == np.uint64(MASK64)).all(), (k, lo, hi, "wrote past the range")
    if with_counts:
        gc = cbuf.cpu().numpy().view(np.uint32).astype(np.int64)
        assert (gc[:n] == counts[lo:hi]).all(), (k, lo, hi, "counters")
        assert (gc[n:] == U32).all(), (k, lo, hi, "wrote counters past the range")
    return kbuf, cbuf


@pytest.mark.gpu
@pytest.mark.parametrize("k", [15, 32, 33, 64])
def test_export_wrap_and_import(eng, E, torch, k):
    rng = np.random.default_rng(k)
    raw = distinct_raw(k, np.concatenate([uniform_mixed(k, 5000, rng), edge_mixed(k)]))
    n = raw.shape[0]
    c = counter_mix(rng, n)
    forms = [("counted", eng.upload(k, raw, c.astype(np.uint32)), c),
             ("plain", eng.upload(k, raw), np.ones(n, dtype=np.int64)),
             ("uniform", eng.upload(k, raw).set_counts(2**31 + 9), np.full(n, 2**31 + 9, dtype=np.int64))]
    for name, s, counts in forms:
        mixed, cnt = stored(k, raw, counts)
        kp, cp = s.device_ptrs()
        assert kp and bool(cp) == (name == "counted")
        for lo, hi in [(0, 0), (n, n), (5, 5), (0, n), (1, n), (2, n - 1), (3, 4), (7, 1000), (1000, 1007), (n - 1, n)]:
            for with_counts in (True, False):
                kbuf, cbuf = export_checked(eng, torch, k, s, mixed, cnt, lo, hi, with_counts)
                m = hi - lo
                if with_counts:          # what came out is a set again: copied in, and wrapped where it lies
                    back = eng.from_device(k, m, kbuf.data_ptr() if m else 0, cbuf.data_ptr() if m else None)
                    wrap = eng.wrap_device(k, m, kbuf.data_ptr() if m else 0, cbuf.data_ptr() if m else None)
                    for got in (back, wrap):
                        gk, gc = got.download()
                        assert (gk == unmix_np(k, mixed[lo:hi])).all() and (gc == cnt[lo:hi]).all(), (k, name, lo, hi)
                elif m:
                    wrap = eng.wrap_device(k, m, kbuf.data_ptr(), None, uniform=0)       # 0 means 1
                    assert wrap.info()["uniform"] == 1 and not wrap.info()["has_counts"]
                    gk, gc = wrap.download()
                    assert (gk == unmix_np(k, mixed[lo:hi])).all() and (gc == 1).all()
                    assert len(eng.from_device(k, m, kbuf.data_ptr(), None)) == m
        for bad_lo, bad_hi in [(2, 1), (0, n + 1), (n + 1, n + 1)]:
            with pytest.raises(E.KhoiceError) as ei:
                s.export_range(bad_lo, bad_hi, kp, None)
            assert ei.value.code == E_ARG
        # export_device: the whole set, at an odd record offset of a larger buffer; a view of it is the set
        wrapped, keep = wrapped_copy(eng, torch, k, s)
        gk, gc = wrapped.download()
        assert (gk == unmix_np(k, mixed)).all() and (gc == cnt).all(), (k, name)
        kb = keep[0].cpu().numpy().view(np.uint64).reshape(-1, words(k))
        assert (kb[0] == np.uint64(MASK64)).all() and (kb[n + 1:] == np.uint64(MASK64)).all()
        cb = keep[1].cpu().numpy().view(np.uint32)
        assert cb[0] == U32 and (cb[n + 1:] == U32).all()
    # empty handles take part in operations like any other
    e1, e2 = eng.from_device(k, 0, 0, None), eng.wrap_device(k, 0, 0, None, uniform=0)
    assert len(e1) == 0 and len(e2) == 0 and e2.info()["uniform"] == 1
    u = eng.union_sum([e1, forms[0][1], e2], U32)
    gk, gc = u.download_sorted()
    keys_s, counts_s = sorted_pivot(k, raw, c)
    assert (gk == keys_s).all() and (gc == counts_s).all()
    assert (eng.partition_bounds([e1, e2], 3) == 0).all()


@pytest.mark.gpu
def test_export_fills_uniform_counters_beyond_one_grid(eng, torch):
    """k_fill_u32 runs at most 2048 blocks of 256 threads: above 524288 counters a thread writes more than one."""
    k = 31
    rng = np.random.default_rng(31)
    raw = distinct_raw(k, uniform_mixed(k, 2048 * 256 + 70_001, rng))
    n = raw.shape[0]
    assert n - 1 > 2048 * 256 + 256
    s = eng.upload(k, raw).set_counts(77)
    mixed, cnt = stored(k, raw, np.full(n, 77, dtype=np.int64))
    export_checked(eng, torch, k, s, mixed, cnt, 1, n, True)
    export_checked(eng, torch, k, s, mixed, cnt, 0, 2048 * 256 + 1, True)


@functools.lru_cache(maxsize=None)
def group_sets_case(k, world):
    """Ten group sets over one pool (uniform keys, the slot edges of `world` parts, the extreme keys): raw keys and
    counters; 0..4 carry counters, 5..9 are uniform (one of them with 3 keys only, one empty)."""
    rng = np.random.default_rng(9000 + 10 * k + world)
    pool = distinct_raw(k, np.concatenate([uniform_mixed(k, 12000, rng), edge_mixed(k),
                                           boundary_mixed(k, rng, [world], per=3)]))
    n = pool.shape[0]
    out = []
    for g in range(10):
        sel = rng.random(n) < rng.uniform(0.1, 0.5)
        if g == 7:
            sel = np.zeros(n, dtype=bool)
            sel[rng.choice(n, size=3, replace=False)] = True
        if g == 8:
            sel[:] = False
        keys = pool[sel]
        uniform = None if g < 5 else (1, 2**31, 6, 1, 77)[g - 5]
        counts = counter_mix(rng, keys.shape[0], [5000]) if g < 5 else np.full(keys.shape[0], uniform, dtype=np.int64)
        out.append((keys, counts, uniform))
    return out


def upload_groups(eng, k, case):
    sets = []
    for keys, counts, uniform in case:
        if uniform is None:
            sets.append(eng.upload(k, keys, counts.astype(np.uint32)))
        else:
            s = eng.upload(k, keys)
            sets.append(s if uniform == 1 else s.set_counts(uniform))
    return sets


def ref_union_mixed(k, case):
    """(mixed keys ascending, int64 counter sums) of the union of the group sets."""
    mixed = np.concatenate([key_view(mix_np(k, keys)) for keys, _, _ in case if keys.shape[0]])
    counts = np.concatenate([c for keys, c, _ in case if keys.shape[0]])
    u, inv = np.unique(mixed, return_inverse=True)
    tot = np.zeros(u.shape[0], dtype=np.int64)
    np.add.at(tot, inv.reshape(-1), counts)
    return view_keys(u, k), tot


@pytest.mark.gpu
@pytest.mark.parametrize("world,k", [(1, 31), (2, 33), (3, 17), (7, 64), (8, 32), (2, 16), (3, 47)])
def test_exchange_rank_by_rank_in_one_process(eng, torch, world, k):
    """The property the key-set exchange of dist.py rests on: cut at the bounds, unioned rank by rank, the slices
    give the union of the whole sets, with both ways of making a slice (a view in place; an export that is wrapped)."""
    from khoice_amd import dist as D
    ops = D.EngineOps(eng, torch.device("cuda:0"))
    case = group_sets_case(k, world)
    sets = upload_groups(eng, k, case)
    w = words(k)
    bounds = np.asarray(ops.partition_bounds_all(sets, world), dtype=np.int64)
    for g, (keys, _, _) in enumerate(case):
        assert (bounds[g] == ref_bounds(k, stored(k, keys, np.zeros(keys.shape[0]))[0], world).astype(np.int64)).all()
    assert any(int(bounds[g][j]) % 2 for g in range(10) for j in range(1, world)) or world == 1      # odd offsets
    ukeys, utot = ref_union_mixed(k, case)
    for cs, hl in ((5000, 513), (U32, 16)):
        want_counts = np.minimum(utot, cs)
        for way in ("view", "export"):
            hist = np.zeros(hl, dtype=np.uint64)
            got_keys, got_counts, keep = [], [], []
            for j in range(world):
                slices = []
                for g in range(10):
                    lo, hi = int(bounds[g][j]), int(bounds[g][j + 1])
                    if hi <= lo:
                        continue
                    if way == "view":
                        slices.append(ops.view_range(sets[g], lo, hi))
                    else:
                        kt = torch.empty((hi - lo) * w, dtype=torch.int64, device="cuda:0")
                        ct = torch.empty(hi - lo, dtype=torch.int32, device="cuda:0")
                        ops.export_range(sets[g], lo, hi, kt, ct)
                        keep.append((kt, ct))
                        slices.append(ops.wrap(k, hi - lo, kt, ct))
                ops.flush()
                if not slices:
                    continue
                hist += eng.union_histogram(slices, cs, hl)
                u, h2 = eng.union_sum(slices, cs, hist_len=hl)
                gk, gc = u.download()
                got_keys.append(gk)
                got_counts.append(gc.astype(np.int64))
                assert (h2 == ref_hist(gc, hl)).all()
            assert (hist == ref_hist(want_counts, hl)).all(), (world, k, way, cs, hl)
            gk, gc = np.concatenate(got_keys), np.concatenate(got_counts)
            assert gk.shape == ukeys.shape and (gk == unmix_np(k, ukeys)).all(), (world, k, way, "keys in rank order")
            assert (gc == want_counts).all(), (world, k, way, cs)
            del keep


@pytest.mark.gpu
@pytest.mark.parametrize("cell_bytes", [1, 4])
def test_table_form_rank_by_rank(eng, torch, cell_bytes):
    """dist.across_groups_table without the collectives: per-rank histograms over its cell ranges add up."""
    k = 9
    case = group_sets_case(k, 8)
    sets = upload_groups(eng, k, case)
    ncell = 4 ** k
    table = torch.zeros(ncell, dtype=torch.uint8 if cell_bytes == 1 else torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    for s in sets:
        eng.table_add_set(s, table.data_ptr(), cell_bytes)
    eng.sync()
    cells = np.zeros(ncell, dtype=np.int64)
    for keys, _, _ in case:
        cells[keys[:, 0].astype(np.int64)] += 1
    assert (table_cells(torch, table, cell_bytes) == cells).all()
    for cs, hl in ((5000, 5001), (3, 16), (0, 2)):
        want = ref_table_hist(cells, cs, hl)
        for world in WORLDS:
            hist = np.zeros(hl, dtype=np.uint64)
            for rank in range(world):
                lo = (rank * ncell // world) // 16 * 16
                hi = ncell if rank == world - 1 else ((rank + 1) * ncell // world) // 16 * 16
                hist += eng.table_histogram(table.data_ptr(), cell_bytes, lo, hi, cs, hl)
            assert (hist == want).all(), (cell_bytes, cs, hl, world)
