"""Shared helpers for the parity tests (oracle dict <-> engine arrays)."""
import re

import numpy as np

MASK64 = (1 << 64) - 1


def words(k):
    return 1 if k <= 32 else 2


def db_to_arrays(db, k):
    """oracle dict{int code: count} -> (keys[n, W] uint64 sorted by k-mer, counts[n])."""
    w = words(k)
    codes = sorted(db)
    keys = np.zeros((len(codes), w), dtype=np.uint64)
    for i, c in enumerate(codes):
        keys[i, 0] = c & MASK64
        if w == 2:
            keys[i, 1] = c >> 64
    counts = np.array([db[c] for c in codes], dtype=np.uint32)
    return keys, counts


def set_to_db(kset):
    keys, counts = kset.download()
    if keys.shape[1] == 1:
        codes = [int(x) for x in keys[:, 0]]
    else:
        codes = [int(lo) | (int(hi) << 64) for lo, hi in zip(keys[:, 0], keys[:, 1])]
    db = dict(zip(codes, (int(c) for c in counts)))
    assert len(db) == len(codes), "engine returned duplicate keys"
    return db


def random_dna(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def multiset_text(keys, counts, k):
    """(keys[n, W] uint64 sorted by k-mer, counts[n]) -> the sorted "KMER<TAB>count<LF>" text of a dump -s."""
    alpha = "ACGT"
    out = []
    for i in range(keys.shape[0]):
        code = int(keys[i, 0]) | ((int(keys[i, 1]) << 64) if keys.shape[1] == 2 else 0)
        out.append("".join(alpha[(code >> (2 * (k - 1 - j))) & 3] for j in range(k)) + "\t" + str(int(counts[i])) + "\n")
    return "".join(out)


def check_multiset_case(case, keys, counts, cs):
    """One case of tests/golden/kmer_multiset.json (the reference's own get_canonical_kmer over
    process_read_into_kmers, Counter'ed) against an implementation's sorted (keys, counts); `cs` is the counter
    ceiling the implementation ran with (it must not be reached unless the case says so)."""
    import hashlib
    k = case["k"]
    assert keys.shape[0] == case["distinct"], (case["kind"], k, keys.shape[0], case["distinct"])
    if case["max_count"] <= cs:
        assert int(counts.sum()) == case["total"]
        text = multiset_text(keys, counts, k)
        assert hashlib.sha256(text.encode()).hexdigest() == case["sha256"], (case["kind"], k, len(case["seq"]))
        if "multiset" in case:
            assert text == "".join(f"{km}\t{c}\n" for km, c in case["multiset"])
    else:   # saturating counters (KMC's documented -cs; not a reference-pinned rule): the k-mer set still has to agree
        assert "multiset" not in case or [km for km, _ in case["multiset"]] == [ln.split("\t")[0] for ln in multiset_text(keys, counts, k).splitlines()]


# ---------------------------------------------------------------- key mixing, vectorised
# A numpy restatement of kh_mix64 / kh_unmix64 / kh_round / kh_mix / kh_unmix / kh_top32
# (khoice_amd/csrc/kh_common.h), so that tests can choose keys in MIXED space — and so their slots —
# for millions of keys at once.  Checked against kh_mix_host / kh_unmix_host in tests/test_abi.py.
MIX_C1 = 0xff51afd7ed558ccd
MIX_C1_INV = pow(MIX_C1, -1, 1 << 64)
MIX_C3 = 0x9e3779b97f4a7c15


def _mask(nbits):
    return np.uint64(MASK64 if nbits >= 64 else (1 << nbits) - 1)


def _mix64(x, n, c):
    m, s = _mask(n), np.uint64((n + 1) >> 1)
    with np.errstate(over="ignore"):
        x = x ^ (x >> s)
        x = (x * np.uint64(c)) & m
        return x ^ (x >> s)


def _round(v, c):
    with np.errstate(over="ignore"):
        v = v ^ (v >> np.uint64(32))
        v = v * np.uint64(c)
        return v ^ (v >> np.uint64(29))


def mix_np(k, keys):
    """keys[n, W] uint64 (k-mer codes) -> mixed keys[n, W]."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1, words(k))
    out = keys.copy()
    if k <= 32:
        out[:, 0] = _mix64(keys[:, 0], 2 * k, MIX_C1)
    else:
        out[:, 0] = _mix64(keys[:, 0], 64, MIX_C1)
        out[:, 1] = keys[:, 1] ^ (_round(out[:, 0], MIX_C3) & _mask(2 * k - 64))
    return out


def unmix_np(k, mixed):
    """mixed keys[n, W] -> k-mer codes[n, W] (inverse of mix_np)."""
    mixed = np.ascontiguousarray(mixed, dtype=np.uint64).reshape(-1, words(k))
    out = mixed.copy()
    if k <= 32:
        out[:, 0] = _mix64(mixed[:, 0], 2 * k, MIX_C1_INV)
    else:
        out[:, 1] = mixed[:, 1] ^ (_round(mixed[:, 0], MIX_C3) & _mask(2 * k - 64))
        out[:, 0] = _mix64(mixed[:, 0], 64, MIX_C1_INV)
    return out


def top32_np(k, mixed):
    """Top 32 bits of the 2k-bit mixed key (left-aligned when 2k < 32), as uint64."""
    mixed = np.asarray(mixed, dtype=np.uint64).reshape(-1, words(k))
    n = 2 * k
    if k <= 32:
        lo = mixed[:, 0]
        return (lo >> np.uint64(n - 32)) if n >= 32 else ((lo << np.uint64(32 - n)) & _mask(32))
    nh = n - 64
    hi, lo = mixed[:, 1], mixed[:, 0]
    if nh >= 32:
        return (hi >> np.uint64(nh - 32)) & _mask(32)
    return ((hi << np.uint64(32 - nh)) | (lo >> np.uint64(32 + nh))) & _mask(32)


def mixed_from_top32(k, top, rng):
    """Mixed keys[n, W] whose top 32 bits are top[n] (uint64 < 2^32), the bits below them random.
    For 2k < 32 the top 32 bits keep only the key's 2k bits: top is rounded down to that grid."""
    top = np.asarray(top, dtype=np.uint64)
    n, w = 2 * k, words(k)
    out = np.zeros((top.shape[0], w), dtype=np.uint64)
    rnd = rng.integers(0, 1 << 63, size=(top.shape[0], 2), dtype=np.uint64) * np.uint64(2) + \
        rng.integers(0, 2, size=(top.shape[0], 2), dtype=np.uint64)
    if w == 1:
        if n >= 32:
            out[:, 0] = (top << np.uint64(n - 32)) | (rnd[:, 0] & _mask(n - 32))
        else:
            out[:, 0] = top >> np.uint64(32 - n)
        return out
    nh = n - 64
    if nh >= 32:
        out[:, 1] = (top << np.uint64(nh - 32)) | (rnd[:, 1] & _mask(nh - 32))
        out[:, 0] = rnd[:, 0]
    else:
        out[:, 1] = top >> np.uint64(32 - nh)
        out[:, 0] = ((top & _mask(32 - nh)) << np.uint64(32 + nh)) | (rnd[:, 0] & _mask(32 + nh))
    return out


def key_view(keys):
    """keys[n, W] -> 1-D array whose order and equality are those of the k-mers (for np.unique etc.)."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    if keys.shape[1] == 1:
        return keys[:, 0].copy()
    v = np.empty(keys.shape[0], dtype=[("hi", "<u8"), ("lo", "<u8")])
    v["hi"], v["lo"] = keys[:, 1], keys[:, 0]
    return v


def view_keys(v, k):
    """Inverse of key_view."""
    if words(k) == 1:
        return np.asarray(v, dtype=np.uint64).reshape(-1, 1)
    out = np.empty((v.shape[0], 2), dtype=np.uint64)
    out[:, 0], out[:, 1] = v["lo"], v["hi"]
    return out


# ---------------------------------------------------------------- planted keys: choose bucket and fine bin
# A numpy restatement of kh_slot (kh_common.h) and fine_bin (kh_kernels.hip), and texts whose k-mers are chosen by
# them, so that a test decides how many keys a bucket of the batched build holds and how they fall into the fine
# bins of its distribution sort.  tests/test_gpu_build_edges.py proves every construction on the C oracle's keys.
M32 = (1 << 32) - 1


def slot_np(k, mixed, nslots):
    """kh_slot: slot of each mixed key among nslots equal-width, order-preserving slots."""
    return (top32_np(k, mixed) * np.uint64(nslots)) >> np.uint64(32)


def fine_bin_np(k, mixed, nslots, fine_bits):
    """fine_bin: the fine bin (of 2^fine_bits) of each mixed key inside its slot."""
    return ((top32_np(k, mixed) * np.uint64(nslots)) & np.uint64(M32)) >> np.uint64(32 - fine_bits)


def _rev_pairs64(x):
    """The 32 two-bit groups of each uint64 in reverse order."""
    x = ((x >> np.uint64(2)) & np.uint64(0x3333333333333333)) | ((x & np.uint64(0x3333333333333333)) << np.uint64(2))
    x = ((x >> np.uint64(4)) & np.uint64(0x0F0F0F0F0F0F0F0F)) | ((x & np.uint64(0x0F0F0F0F0F0F0F0F)) << np.uint64(4))
    return x.byteswap()


def revcomp_np(k, keys):
    """keys[n, W] uint64 (k-mer codes) -> codes of their reverse complements."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1, words(k))
    out = np.empty_like(keys)
    if k <= 32:
        out[:, 0] = _rev_pairs64(~keys[:, 0]) >> np.uint64(64 - 2 * k)
        return out
    s = 128 - 2 * k
    rlo, rhi = _rev_pairs64(~keys[:, 0]), _rev_pairs64(~keys[:, 1])      # the 128-bit reversal is (rlo, rhi)
    if s == 0:
        out[:, 0], out[:, 1] = rhi, rlo
    else:
        out[:, 0] = (rhi >> np.uint64(s)) | (rlo << np.uint64(64 - s))
        out[:, 1] = rlo >> np.uint64(s)
    return out


def planted_codes(k, nb, b, f, n, rng, fine_bits):
    """n distinct canonical k-mer codes[n, W] whose mixed key lies in slot b of nb slots and, unless f is None, in fine
    bin f of that slot.  The 32-bit product (top32 * nb) is chosen first: p = b << 32 | f << (32 - fine_bits) | r;
    top = ceil(p / nb) is kept when top * nb still has slot b and fine bin f."""
    assert 2 * k >= 40 and 0 <= b < nb
    sh = 32 - fine_bits
    lo = (b << 32) | ((f << sh) if f is not None else 0)
    span = (1 << sh) if f is not None else (1 << 32)
    tops_all = None
    if span <= (1 << 20):
        p = np.uint64(lo) + np.arange(span, dtype=np.uint64)
        tops_all = np.unique((p + np.uint64(nb - 1)) // np.uint64(nb))
    got = np.zeros((0, words(k)), dtype=np.uint64)
    for _ in range(200):
        m = 4 * (n - got.shape[0]) + 64
        if tops_all is not None:
            top = tops_all[rng.integers(0, tops_all.shape[0], size=m)]
        else:
            p = np.uint64(lo) + rng.integers(0, span, size=m, dtype=np.uint64)
            top = (p + np.uint64(nb - 1)) // np.uint64(nb)
        top = top[top <= np.uint64(M32)]
        prod = top * np.uint64(nb)
        ok = (prod >> np.uint64(32)) == np.uint64(b)
        if f is not None:
            ok &= ((prod & np.uint64(M32)) >> np.uint64(sh)) == np.uint64(f)
        codes = unmix_np(k, mixed_from_top32(k, top[ok], rng))
        rc = revcomp_np(k, codes)
        if words(k) == 1:
            canon = codes[:, 0] <= rc[:, 0]
        else:
            canon = (codes[:, 1] < rc[:, 1]) | ((codes[:, 1] == rc[:, 1]) & (codes[:, 0] <= rc[:, 0]))
        codes = codes[canon]
        both = np.concatenate([got, codes])
        _, first = np.unique(key_view(both), return_index=True)
        got = both[np.sort(first)]
        if got.shape[0] >= n:
            return got[:n]
    raise AssertionError(f"no {n} canonical keys in slot {b}/{nb}, fine bin {f}")


def codes_text(k, keys):
    """keys[n, W] uint64 -> the n k-mers as ASCII rows uint8[n, k]."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1, words(k))
    out = np.empty((keys.shape[0], k), dtype=np.uint8)
    alpha = np.frombuffer(b"ACGT", dtype=np.uint8)
    for j in range(k):
        bit = 2 * (k - 1 - j)
        out[:, j] = alpha[((keys[:, bit >> 6] >> np.uint64(bit & 63)) & np.uint64(3)).astype(np.intp)]
    return out


def planted_text(k, keys, mult, npos, rng, head=b""):
    """A text of exactly npos k-mer start positions: `head`, then keys[i] written mult[i] times, every copy closed by
    one N, in shuffled order, then N to the end.  N adds positions but no keys."""
    rows = codes_text(k, keys)
    order = rng.permutation(np.repeat(np.arange(rows.shape[0]), np.asarray(mult, dtype=np.int64)))
    body = np.full((order.shape[0], k + 1), ord("N"), dtype=np.uint8)
    body[:, :k] = rows[order]
    text = bytes(head) + body.tobytes()
    pad = npos + k - 1 - len(text)
    assert pad >= 0, (npos, len(text))
    return text + b"N" * pad


def random_dna_np(rng, n, alphabet=b"ACGT"):
    """n random bases as bytes (numpy generator: millions of bases in milliseconds)."""
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), size=n)].tobytes()


# ---- the plan constants the planted cases lean on (the test modules read them out of the sources)
MEAN = {1: 3700, 2: 1750}        # KH_TUNE_MEAN_W1, KH_BUCKET_MEAN_W2: k-mer positions per bucket
CAP = {1: 4096, 2: 2048}         # KH_SORT_CAP_W1 / _W2: keys a bucket sorts in LDS
FINE_BITS = 13                   # KH_TUNE_FINE_BITS


class Planted:
    """Families of planted keys for one text of `nb` buckets."""

    def __init__(self, k, nb, seed):
        self.k, self.w, self.nb = k, words(k), nb
        self.rng = np.random.default_rng(seed)
        self.keys = np.zeros((0, self.w), dtype=np.uint64)
        self.mult = np.zeros(0, dtype=np.int64)

    def add(self, b, f, n, mult=1, avoid=()):
        """n distinct keys in bucket b (fine bin f, or spread over the bucket when f is None, outside the fine bins
        `avoid`), each written mult times (an int or one per key).  Returns the keys."""
        got = planted_codes(self.k, self.nb, b, f, n + 8 * len(avoid), self.rng, FINE_BITS)
        if avoid:
            fine = fine_bin_np(self.k, mix_np(self.k, got), self.nb, FINE_BITS)
            got = got[~np.isin(fine, np.array(avoid, dtype=np.uint64))]
        got = got[:n]
        assert got.shape[0] == n
        if self.keys.shape[0]:
            assert not np.isin(key_view(got), key_view(self.keys)).any()
        self.keys = np.concatenate([self.keys, got])
        self.mult = np.concatenate([self.mult, np.broadcast_to(np.asarray(mult, dtype=np.int64), (n,))])
        return got

    def text(self, head=b""):
        return planted_text(self.k, self.keys, self.mult, self.nb * MEAN[self.w], self.rng, head)


def grid_sub_ranges(k, ngenomes, fan, hash_form):
    """S of build_once's grid mode for `ngenomes` genomes that all have a whole number of buckets of k-mer positions,
    the same number each (kh_engine.cpp: 'sub-ranges per bucket'); fan: genomes of the largest group."""
    w = words(k)
    cap = 4096 if (w == 1 and hash_form) else CAP[w]
    zg = 5.0 * np.sqrt(fan)
    x = 0.5 * (-zg + np.sqrt(zg * zg + 4.0 * cap))
    target = max(16, min(cap * 92 // 100, int(x * x)))
    per_bucket = ngenomes * MEAN[w]
    return -(-per_bucket // target)


# ---------------------------------------------------------------- constructed sets
# Keys chosen in MIXED space (so a test decides their slots and how they cluster), counters over the whole u32 range,
# and the host copy of an uploaded set: shared by the modules that test set operations, views and tables.
U32 = (1 << 32) - 1


def edge_mixed(k):
    """Mixed keys 0, 1, max - 1, max: the first and the last slot."""
    m = (1 << (2 * k)) - 1
    vals = sorted({0, 1, m - 1, m})
    return np.array([[v & (2**64 - 1), v >> 64][:words(k)] for v in vals], dtype=np.uint64)


def boundary_mixed(k, rng, slots, per=3):
    """Runs of keys whose top 32 bits are ceil(r * 2^32 / n) or one below, for every n in `slots`."""
    tops = []
    for n in slots:
        for r in range(1, n):
            t = -(-(r << 32) // n)
            tops += [t] * per + [t - 1] * per
    if not tops:
        return np.zeros((0, words(k)), dtype=np.uint64)
    return mixed_from_top32(k, np.array(tops, dtype=np.uint64), rng)


def uniform_mixed(k, n, rng):
    return mixed_from_top32(k, rng.integers(0, 1 << 32, size=n, dtype=np.uint64), rng)


def clustered_mixed(k, n, rng, frac, start=0):
    """n mixed keys whose top 32 bits lie in [start, start + 2^32 * frac)."""
    width = max(1, int((1 << 32) * frac))
    return mixed_from_top32(k, np.uint64(start) + rng.integers(0, width, size=n, dtype=np.uint64), rng)


def distinct_raw(k, mixed):
    """Distinct mixed keys -> their k-mer codes (what kh_set_upload takes), in random order."""
    v = np.unique(key_view(mixed))
    return unmix_np(k, view_keys(v, k))


def counter_mix(rng, n, extra=()):
    """Counters over [1, 2^32 - 1] with mass at the histogram tiers, near 2^31, near 2^32 and near
    every value of `extra` (the cs values of a test)."""
    centres = [2**31 - 1, 2**31, U32 - 2] + list(extra)
    kind = rng.integers(0, 6, size=n)
    c = np.empty(n, dtype=np.int64)
    c[kind == 0] = rng.integers(1, 16, size=int((kind == 0).sum()))
    c[kind == 1] = rng.integers(16, 520, size=int((kind == 1).sum()))
    c[kind == 2] = rng.integers(500, 6000, size=int((kind == 2).sum()))
    c[kind == 3] = rng.integers(1, U32 + 1, size=int((kind == 3).sum()), dtype=np.int64)
    near = rng.choice(np.array(centres, dtype=np.int64), size=int((kind >= 4).sum()))
    c[kind >= 4] = near + rng.integers(-2, 3, size=near.shape[0])
    return np.clip(c, 1, U32)


class Operand:
    """Host copy (keys[n, W] k-mer codes, int64 counters) of a set uploaded to the engine."""

    def __init__(self, eng, k, keys, counts=None, uniform=None):
        self.k, self.keys = k, keys
        n = keys.shape[0]
        if counts is not None:
            self.counts = np.asarray(counts, dtype=np.int64)
            self.set = eng.upload(k, keys, self.counts.astype(np.uint32))
        else:
            base = eng.upload(k, keys)
            self.counts = np.full(n, 1 if uniform is None else uniform, dtype=np.int64)
            self.set = base if uniform is None else base.set_counts(uniform)

    def with_uniform(self, eng, v):
        o = Operand.__new__(Operand)
        o.k, o.keys = self.k, self.keys
        o.counts = np.full(self.keys.shape[0], v, dtype=np.int64)
        o.set = self.set.set_counts(v)
        return o


def ref_hist(counts, hist_len):
    return np.bincount(np.minimum(np.asarray(counts, dtype=np.int64), hist_len - 1),
                       minlength=hist_len).astype(np.uint64)


# ---------------------------------------------------------------- the hash-set modules of the super-k-mer form
# What tests/test_gpu_skm_hashsets.py (one-word keys) and tests/test_gpu_skm2_hashsets.py (two-word keys) share: the
# layout of chosen keys over genomes, the parser of the engine's [skm] debug line, and the comparison of one
# kh_exp1_run call with the C restatement together with the kernels that did the work.
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
PAIRS = [(5000, 80), (2, 5)]          # (cs, hist_len): nothing clamps / both clamp


def revcomp(s):
    return "".join(COMP[ch] for ch in reversed(s))


def two_kmer(s, m):
    """A record of two k-mers, s and a neighbour, both holding A^m: s + C, or C + s when A^m starts s."""
    return s + "C" if s.find("A" * m) > 0 else "C" + s


def skm_layout(keys, ngen, group_size, m, extra_records=()):
    """Lone records of `keys` in ngen genomes (groups of group_size): key i in genome i % ngen; every third also in
    genome (i + ngen // 2) % ngen (with 40 genomes: identical records in both halves of the 64-bit mask, which must
    not merge); every even one again in its genome as its reverse complement (another record, the same key: a
    repeat); every i % 4 == 1 again inside a two-k-mer record (two_kmer)."""
    recs = [[] for _ in range(ngen)]
    for i, s in enumerate(keys):
        g = i % ngen
        recs[g].append(s)
        if i % 3 == 0:
            recs[(g + ngen // 2) % ngen].append(s)
        if i % 2 == 0:
            recs[g].append(revcomp(s))
        elif i % 4 == 1:
            recs[g].append(two_kmer(s, m))
    for j, r in enumerate(extra_records):
        recs[(7 * j) % ngen].append(r)
    return ["N".join(r).encode() for r in recs], [g // group_size for g in range(ngen)]


def records_of(seqs, g):
    return seqs[g].decode().split("N")


def instances(seqs, k):
    return sum(max(0, len(r) - k + 1) for g in range(len(seqs)) for r in records_of(seqs, g))


def memo_in(cache):
    """A decorator that keeps a case builder's results in `cache` (the CPU and the GPU tests use the same inputs)."""
    def deco(fn):
        def f(*a):
            key = (fn.__name__,) + a
            if key not in cache:
                cache[key] = fn(*a)
            return cache[key]
        f.__name__ = fn.__name__
        f.__doc__ = fn.__doc__
        return f
    return deco


SKM_SLOT = re.compile(r"\[skm\] k=(\d+) m=(\d+) .*slot: mean [\d.]+ max (\d+) cap (\d+) .*expanded: (\d+) k-mers \| "
                      r"errors (\d+) spilled (\d+) overfull slots (\d+)")
SKM_PLAN = re.compile(r"\[skm\] k=\d+ m=\d+ w=(\d+) nmax=\d+ positions=(\d+) records=(\d+) .* nb1=(\d+) S=(\d+) nslots=(\d+) \| "
                      r"coarse: mean \d+ max (\d+) cap (\d+) \|")


def skm_line(err):
    """The one [skm] line (KHOICE_SKM_DEBUG=1) of a call: how full the regions were, and the plan's geometry."""
    lines = SKM_SLOT.findall(err)
    assert len(lines) == 1, err
    k, m, slot_max, cap, expanded, errors, spilled, overfull = (int(x) for x in lines[0])
    w, positions, records, nb1, S, nslots, coarse_max, cap1 = (int(x) for x in SKM_PLAN.findall(err)[0])
    return dict(k=k, m=m, slot_max=slot_max, cap=cap, expanded=expanded, errors=errors, spilled=spilled, overfull=overfull,
                w=w, positions=positions, records=records, nb1=nb1, S=S, nslots=nslots, coarse_max=coarse_max, cap1=cap1)


def exp1_run_stats(eng, seqs, group_of, k, cs, hist_len, kernels, counters):
    """(result, {name: launches of the kernel class / growth of the counter during the call})"""
    eng.profile(True)
    st0 = eng.stats()
    got = eng.exp1_run(seqs, group_of, k, cs=cs, hist_len=hist_len)
    st1 = eng.stats()
    eng.profile(False)
    did = {n: st1["kernels"][n]["launches"] - st0["kernels"][n]["launches"] for n in kernels}
    for n in counters:
        did[n] = st1[n] - st0[n]
    return got, did


def exp1_same(got, want):
    for f in ("within_hist", "across_hist", "distinct_per_seq"):
        assert got[f].shape == want[f].shape and (got[f] == want[f]).all(), f


# what tests/test_gpu_skm_union_chain.py, tests/test_gpu_skm_union_claims.py and their followers share
UNION_KERNELS = ("skm_union", "skm_big", "union_tagged")
UNION_COUNTERS = ("retries", "big_slots")
SKM_NSLOTS = re.compile(r"\[skm\] k=\d+ .* nslots=(\d+) \|")


def run_checked(eng, capfd, seqs, group_of, k, cs=5000, hist_len=5001):
    """One call against the oracle, a second that must give the same; -> (the [skm] line's nslots, what ran)."""
    from oracle import c_oracle as CO
    want = CO.exp1(seqs, group_of, k, cs=cs, hist_len=hist_len)
    capfd.readouterr()
    got, did = exp1_run_stats(eng, seqs, group_of, k, cs, hist_len, UNION_KERNELS, UNION_COUNTERS)
    err = capfd.readouterr().err
    exp1_same(got, want)
    again, did2 = exp1_run_stats(eng, seqs, group_of, k, cs, hist_len, UNION_KERNELS, UNION_COUNTERS)
    capfd.readouterr()
    exp1_same(again, got)
    assert did2 == did
    found = SKM_NSLOTS.findall(err)
    assert len(found) == 1, err
    return int(found[0]), did, err


def fitted(seqs, k, n):
    """(the texts, the last one cut by fewer than n bases; KHOICE_SKM_MEAN) for which nslots = ceil(positions / mean)
    is exactly n."""
    positions = sum(len(s) - k + 1 for s in seqs)
    mean = positions // n
    assert mean >= 64 and positions - n * mean < len(seqs[-1]) - k
    return seqs[:-1] + [seqs[-1][:len(seqs[-1]) - (positions - n * mean)]], mean


def exp1_check(eng, capfd, seqs, group_of, k, expect, kernels, counters):
    """The oracle's answer at every (cs, hist_len) of PAIRS, twice each with identical statistics; expect: {stat: n}
    (exactly n) or {stat: (n, None)} (at least n).  Returns the engine's stderr of the first run of each pair."""
    from oracle import c_oracle as CO
    errs = []
    for cs, hl in PAIRS:
        want = CO.exp1(seqs, group_of, k, cs=cs, hist_len=hl)
        capfd.readouterr()
        got, did = exp1_run_stats(eng, seqs, group_of, k, cs, hl, kernels, counters)
        errs.append(capfd.readouterr().err)
        exp1_same(got, want)
        for n, v in expect.items():
            assert (did[n] >= v[0]) if isinstance(v, tuple) else (did[n] == v), (n, did, errs[-1][-3000:])
        again, did2 = exp1_run_stats(eng, seqs, group_of, k, cs, hl, kernels, counters)
        capfd.readouterr()
        assert did2 == did
        exp1_same(again, want)
    return errs


# ---------------------------------------------------------------- device-resident texts, read where they lie
# tests/test_gpu_device_texts.py: the texts of a case lie in ONE array of random bases (the arena) at chosen byte
# offsets from 256-byte aligned addresses, so a kernel that reads past a text's end reads valid bases of the same
# allocation: an over-read shows as extra k-mers, never as a fault.
ARENA_ALIGNED = (0, 16)          # offsets from a 256-aligned base that the library reads in place (pointer mod 16 == 0)
ARENA_UNALIGNED = (1, 8, 15)     # offsets it packs with a device-to-device copy
ARENA_TAIL = 4096                # bytes of the arena behind the end of the last text, at least
ARENA_MAX = 1 << 20


def canon_positions(text, k):
    """The canonical code of every k-mer position of a text of ACGT, in order (rolling; plain ints, any k)."""
    val = {65: 0, 67: 1, 71: 2, 84: 3}
    mask, top = (1 << (2 * k)) - 1, 2 * (k - 1)
    fw = rc = 0
    out = []
    for i, b in enumerate(text):
        v = val[b]
        fw = ((fw << 2) | v) & mask
        rc = (rc >> 2) | ((3 - v) << top)
        if i >= k - 1:
            out.append(min(fw, rc))
    return out


class Arena:
    """texts[i] (bytes, or None for the text given as pointer 0 with length 0) at offset classes[i] from a 256-byte
    aligned address of its own; behind[i] (a byte value or None) is written right behind the text.  host: the arena;
    at[i]: the text's offset in it (None for a None text)."""

    def __init__(self, texts, classes, behind, seed):
        rng = np.random.default_rng(seed)
        self.texts, self.at, cursor = list(texts), [], 256
        for t, c in zip(texts, classes):
            if t is None:
                self.at.append(None)
                continue
            self.at.append(((cursor + 255) & ~255) + c)
            cursor = self.at[-1] + len(t) + 64
        self.host = np.frombuffer(random_dna_np(rng, cursor + ARENA_TAIL + 256), dtype=np.uint8).copy()
        for t, a, f in zip(texts, self.at, behind):
            if t is None:
                continue
            self.host[a:a + len(t)] = np.frombuffer(t, dtype=np.uint8)
            if f is not None:
                self.host[a + len(t)] = f
        self.dev = None

    def upload(self):
        """The arena in one device tensor whose first byte is 256-byte aligned -> [(pointer, length)] of the texts."""
        import torch
        n = self.host.shape[0]
        dev = torch.from_numpy(self.host).to("cuda:0")
        shift = (-dev.data_ptr()) & 255
        if shift:                                    # offsets are counted from a 256-byte aligned address
            dev2 = torch.empty(n + 256, dtype=torch.uint8, device="cuda:0")
            shift = (-dev2.data_ptr()) & 255
            dev2[shift:shift + n] = dev
            dev = dev2
        torch.cuda.synchronize()
        self.dev, self.shift = dev, shift
        base = dev.data_ptr() + shift
        assert base % 256 == 0
        return [(0, 0) if t is None else (base + a, len(t)) for t, a in zip(self.texts, self.at)]

    def download(self):
        import torch
        torch.cuda.synchronize()
        return self.dev[self.shift:self.shift + self.host.shape[0]].cpu().numpy()
