"""Shared helpers for the parity tests (oracle dict <-> engine arrays)."""
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
