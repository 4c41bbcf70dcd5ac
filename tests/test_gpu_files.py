"""GPU: the layer the reference workflow talks to (khoice_amd/csrc/kh_io.cpp): kh_save / kh_load of the
<prefix>.kmc_pre + <prefix>.kmc_suf container, kh_dump_sorted, kh_histogram_file, kh_write_histogram_text,
kh_build_fasta, and kh_set_counter_max through every producer, at every key width and counter width.

  a. the container is read and written here by an INDEPENDENT reader and writer (struct + numpy, from the documented
     layout): what the library writes must decode to the host copy of the set, and what the writer writes must load
     to the same set and be written back byte for byte.  That pins the format in both directions;
  b. sets are uploaded from keys chosen in mixed space (both ends of the key space, the all-A k-mer, the largest
     canonical code, for two-word keys pairs whose high words order against their low words), with counters at every
     width (1 .. 2^32 - 1), plain, uniform and empty, and PRODUCED: the three views of one batched build, a
     set_counts view, a union and an intersection with ceilings above 255, a zero-copy view of torch memory;
  c. damaged pairs: every header field, every size, and bodies of the right size that break what the consumers rely
     on (ascending, distinct, inside the key space, no zero counter).  All of these are host-side refusals: no kernel
     is ever given bad data.
Every comparison is exact, against oracle/kmer_oracle.py or a few lines of numpy.

The unmarked tests prove the constructed inputs on the CPU (the order traps, the listed counters, the header whose
record count wraps, each damaged body) and run kh_write_histogram_text, which needs no device."""
import ctypes as C
import functools
import gzip
import os
import struct

import numpy as np
import pytest

from oracle import kmer_oracle as O
from tests.util import (MASK64, U32, counter_mix, db_to_arrays, distinct_raw, edge_mixed, key_view, mix_np,
                        random_dna_np, uniform_mixed, unmix_np, view_keys, words)

KS = [1, 2, 16, 31, 32, 33, 48, 63, 64]
LISTED = [1, 255, 256, 65535, 65536, 2**24 - 1, 2**24, 2**31, 2**32 - 1]      # every counter width and its neighbour
UNIFORMS = {"uniform_1": 1, "uniform_7": 7, "uniform_big": 2**31 + 9}
COUNTED = ["counted", "counted_b", "counted_c"]          # the listed counters rotate through them (4^1 is 4 keys)
UPLOADED = COUNTED + ["plain"] + list(UNIFORMS) + ["empty_counted", "empty_plain", "empty_uniform"]
PRODUCED = ["batch0", "batch1", "batch2", "plain_batch0", "plain_batch1", "plain_batch2", "batch1_set_counts",
            "union_5000", "intersect_70000", "wrapped_counted", "wrapped_plain"]
FORMS = UPLOADED + PRODUCED
HIST_CMAX = [1, 2, 255, 256, 65535]
E_ARG, E_IO, E_FORMAT = -1, -3, -4


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


# ---------------------------------------------------------------- the container, read and written independently
# <prefix>.kmc_pre, 48 bytes: "KHAMDPRE", u32 version = 1, k, words, has_counts, uniform, counter_max, u64 n, u64 mix_id
# <prefix>.kmc_suf: "KHAMDSUF", n * words little-endian u64 mixed keys ascending (word 0 low), n u32 counters if has_counts
PRE = struct.Struct("<8s6I2Q")
FIELDS = ("version", "k", "words", "has_counts", "uniform", "counter_max", "n", "mix_id")


def pack_pre(h, magic=b"KHAMDPRE"):
    return PRE.pack(magic, *[h[f] for f in FIELDS])


def pack_suf(keys, counts, magic=b"KHAMDSUF"):
    body = np.ascontiguousarray(keys, dtype="<u8").tobytes()
    if counts is not None:
        body += np.asarray(counts).astype("<u4").tobytes()
    return magic + body


def write_pair(prefix, pre, suf):
    with open(prefix + ".kmc_pre", "wb") as fh:
        fh.write(pre)
    if suf is not None:
        with open(prefix + ".kmc_suf", "wb") as fh:
            fh.write(suf)


def raw_pair(prefix):
    return open(prefix + ".kmc_pre", "rb").read(), open(prefix + ".kmc_suf", "rb").read()


def read_pair(prefix):
    """(header dict, mixed keys[n, W] uint64, counters[n] int64 or None); every byte of both files is accounted for."""
    pre, suf = raw_pair(prefix)
    assert PRE.size == 48 and len(pre) == 48, len(pre)
    magic, *vals = PRE.unpack(pre)
    assert magic == b"KHAMDPRE" and suf[:8] == b"KHAMDSUF"
    h = dict(zip(FIELDS, vals))
    n, w = h["n"], h["words"]
    keys = np.frombuffer(suf, dtype="<u8", count=n * w, offset=8).reshape(n, w).astype(np.uint64)
    end = 8 + 8 * n * w
    counts = None
    if h["has_counts"]:
        counts = np.frombuffer(suf, dtype="<u4", count=n, offset=end).astype(np.int64)
        end += 4 * n
    assert len(suf) == end, (len(suf), end)
    return h, keys, counts


# ---------------------------------------------------------------- host copies of the sets
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


def largest_canonical(k):
    """The largest code that is not above its reverse complement: T^h A^h, with a C in the middle when k is odd."""
    h = k // 2
    return O.encode("T" * h + ("C" if k % 2 else "") + "A" * h)


def order_traps(k):
    """Two-word codes (high word below 4, so they exist from k = 33 on): two pairs that the high word orders one way
    and the low word the other, and a pair that differs in the low word only."""
    if words(k) == 1:
        return []
    hi_lo = [(1, MASK64), (2, 0), (2, 7), (3, 3), (1, 1), (1, 1 << 63)]
    return [(hi << 64) | lo for hi, lo in hi_lo]


@functools.lru_cache(maxsize=None)
def host_keys(k):
    """Distinct k-mer codes[n, W] in shuffled order: both ends of the MIXED key space, a few hundred uniform keys, the
    all-A k-mer, the largest canonical code and the order traps (4^k keys at most)."""
    rng = np.random.default_rng(100 + k)
    raw = distinct_raw(k, np.concatenate([edge_mixed(k), uniform_mixed(k, 300, rng)]))
    raw = np.concatenate([raw, ints_to_keys(k, [0, largest_canonical(k)] + order_traps(k))])
    raw = view_keys(np.unique(key_view(raw)), k)
    return raw[rng.permutation(raw.shape[0])]


class Host:
    """What a set must hold: k-mer codes keys[n, W], int64 counters, and what kh_set_info / _counter_max report."""

    def __init__(self, k, keys, counts, has_counts, uniform=1, counter_max=255):
        self.k, self.keys, self.counts = k, keys, np.asarray(counts, dtype=np.int64)
        self.n = keys.shape[0]
        self.has_counts, self.uniform, self.counter_max = bool(has_counts and self.n), uniform, counter_max
        assert self.counts.shape == (self.n,)

    @classmethod
    def from_db(cls, k, db, has_counts, uniform=1, counter_max=255):
        keys, counts = db_to_arrays(db, k)
        return cls(k, keys, counts, has_counts, uniform, counter_max)

    def info(self):
        return {"n": self.n, "k": self.k, "words": words(self.k), "has_counts": self.has_counts, "uniform": self.uniform}

    def header(self, mix_id):
        return {"version": 1, "k": self.k, "words": words(self.k), "has_counts": int(self.has_counts),
                "uniform": self.uniform, "counter_max": self.counter_max, "n": self.n, "mix_id": mix_id}

    def by_kmer(self):
        order = np.argsort(key_view(self.keys), kind="stable")
        return self.keys[order], self.counts[order]

    def stored(self):
        """(mixed keys ascending, their counters): the body of the suffix file."""
        mixed = mix_np(self.k, self.keys)
        order = np.argsort(key_view(mixed), kind="stable")
        return mixed[order], self.counts[order]

    def db(self):
        return dict(zip(keys_to_ints(self.keys), (int(c) for c in self.counts)))


@functools.lru_cache(maxsize=None)
def batch_texts(k):
    """Three short cleaned texts (records, N runs, a stretch that repeats) for one kh_build_batch."""
    rng = np.random.default_rng(7 + k)
    out = []
    for length in (700, 300, 900):
        body = random_dna_np(rng, length)
        rep = body[:k + 20]
        out.append(body + b"N" + rep * 3 + b"\n" + random_dna_np(rng, 2 * k + 5) + b"NN" + rep)
    return out


def batch_db(k, i):
    return O.count_records(batch_texts(k)[i].decode().split("\n"), k, 1, O.KMC_DEFAULT_CX, 255)


def operand_hosts(k):
    """Three overlapping operands of the union and the intersection: two counted, one uniform."""
    a, b = host_case(k, "counted"), host_case(k, "counted_b")
    n = a.n
    return [Host(k, a.keys[:max(1, 2 * n // 3)], a.counts[:max(1, 2 * n // 3)], True),
            Host(k, b.keys[n // 3:], b.counts[n // 3:], True), host_case(k, "uniform_7")]


@functools.lru_cache(maxsize=None)
def host_case(k, form):
    keys = host_keys(k)
    n = keys.shape[0]
    rng = np.random.default_rng(1000 * k + FORMS.index(form))
    if form in COUNTED:
        rot = 4 * COUNTED.index(form)
        counts = counter_mix(rng, n)
        m = min(n, len(LISTED))
        counts[:m] = (LISTED[rot:] + LISTED[:rot])[:m]
        return Host(k, keys, counts, True)
    if form == "plain":
        return Host(k, keys, np.ones(n), False)
    if form in UNIFORMS:
        v = UNIFORMS[form]
        return Host(k, keys, np.full(n, v), False, v, max(v, 255))
    if form.startswith("empty"):
        v = 7 if form == "empty_uniform" else 1
        return Host(k, keys[:0], np.zeros(0), False, v, 255)
    if form.startswith("batch") and form[-1].isdigit():
        return Host.from_db(k, batch_db(k, int(form[-1])), True)
    if form.startswith("plain_batch"):
        return Host.from_db(k, O.set_counts(batch_db(k, int(form[-1])), 1), False)
    if form == "batch1_set_counts":
        return Host.from_db(k, O.set_counts(batch_db(k, 1), 9), False, 9, 255)
    if form == "union_5000":
        return Host.from_db(k, O.union_sum([h.db() for h in operand_hosts(k)], 5000), True, 1, 5000)
    if form == "intersect_70000":
        a, b, _ = operand_hosts(k)
        return Host.from_db(k, O.intersect(a.db(), b.db(), "sum", cs=70000), True, 1, 70000)
    if form == "wrapped_counted":
        return Host(k, keys, host_case(k, "counted_c").counts, True)
    if form == "wrapped_plain":
        return Host(k, keys, np.full(n, 3), False, 3, 255)
    raise KeyError(form)


# ---------------------------------------------------------------- damage, done with the independent writer
def flipped_words(h):
    return 3 - h["words"]


HEADER_DAMAGE = {
    # name: (header field, new value from the good header) -> KH_E_FORMAT
    "version_2": ("version", lambda h: 2),
    "k_0": ("k", lambda h: 0),
    "k_65": ("k", lambda h: 65),
    "words_of_the_other_width": ("words", flipped_words),
    "mix_id_one_bit": ("mix_id", lambda h: h["mix_id"] ^ (1 << 17)),
    "n_plus_1": ("n", lambda h: h["n"] + 1),
    "n_minus_1": ("n", lambda h: h["n"] - 1),
    "n_plus_2_62": ("n", lambda h: h["n"] + (1 << 62)),
    "has_counts_flipped": ("has_counts", lambda h: 1 - h["has_counts"]),
}
FILE_DAMAGE = {
    # name: (pre, suf) -> (pre, suf) -> KH_E_FORMAT
    "pre_empty": lambda pre, suf: (b"", suf),
    "pre_one_byte_short": lambda pre, suf: (pre[:-1], suf),
    "pre_magic": lambda pre, suf: (b"KHAMDPRF" + pre[8:], suf),
    "suf_one_byte_short": lambda pre, suf: (pre, suf[:-1]),
    "suf_one_byte_long": lambda pre, suf: (pre, suf + b"\0"),
    "suf_magic": lambda pre, suf: (pre, b"KHAMDSUG" + suf[8:]),
}
DAMAGE = list(HEADER_DAMAGE) + list(FILE_DAMAGE)


def damaged_pair(name, h, keys, counts):
    """(pre, suf) of the good pair (h, keys, counts) with one thing wrong."""
    if name in HEADER_DAMAGE:
        field, new = HEADER_DAMAGE[name]
        return pack_pre(dict(h, **{field: new(h)})), pack_suf(keys, counts)
    return FILE_DAMAGE[name](pack_pre(h), pack_suf(keys, counts))


BODY_DAMAGE = ["swapped", "duplicated", "outside_key_space", "zero_counter", "uniform_0"]


def damaged_body(name, k, h, keys, counts):
    """(header, keys, counts) of the right size that no consumer may be given, and the records that differ."""
    keys = keys.copy()
    counts = None if counts is None else counts.copy()
    n = keys.shape[0]
    i = n // 2
    if name == "swapped":
        keys[[i, i + 1]] = keys[[i + 1, i]]
        return h, keys, counts, [i, i + 1]
    if name == "duplicated":
        keys[i + 1] = keys[i]
        return h, keys, counts, [i + 1]
    if name == "outside_key_space":        # the last key stays the largest: only the key space is broken
        assert (2 * k) % 64
        keys[n - 1, -1] |= np.uint64(1 << 63)
        return h, keys, counts, [n - 1]
    if name == "zero_counter":
        counts[i] = 0
        return h, keys, counts, [i]
    if name == "uniform_0":
        return dict(h, uniform=0), keys, counts, []
    raise KeyError(name)


def body_cases():
    return [(k, form, name) for k in (31, 33) for form in ("counted", "plain") for name in BODY_DAMAGE
            if (name == "zero_counter") <= (form == "counted") and (name == "uniform_0") <= (form == "plain")]


# ---------------------------------------------------------------- self-checks without a GPU
def test_cpu_largest_canonical_code_by_enumeration():
    for k in (1, 2, 3, 4, 5, 6):
        canon = [c for c in range(4 ** k) if O.decode(c, k) <= O.reverse_complement(O.decode(c, k))]
        assert max(canon) == largest_canonical(k), k


@pytest.mark.parametrize("k", KS)
def test_cpu_constructed_keys_hold_their_edges(k):
    keys = host_keys(k)
    codes = keys_to_ints(keys)
    assert len(set(codes)) == len(codes) and max(codes) < 4 ** k
    assert len(codes) == 4 ** k if k <= 2 else len(codes) >= 300
    assert 0 in codes and largest_canonical(k) in codes
    mixed = keys_to_ints(mix_np(k, keys))
    assert {0, 1, 4 ** k - 2, 4 ** k - 1} <= set(mixed)                     # both ends of the mixed space
    assert (unmix_np(k, mix_np(k, keys)) == keys).all()
    if words(k) == 2:
        have = {(int(hi), int(lo)) for lo, hi in keys}
        against = [(a, b) for a in have for b in have if a[0] < b[0] and a[1] > b[1] and a[0] and b[0] < 4]
        low_only = [(a, b) for a in have for b in have if a[0] == b[0] and a[1] < b[1]]
        assert len(against) >= 2 and len(low_only) >= 1, k
        traps = order_traps(k)
        assert all(t in codes for t in traps)
        t = ints_to_keys(k, traps)
        for a, b in ((0, 1), (2, 3)):      # ordered by the high word, against the low words
            assert t[a, 1] < t[b, 1] and t[a, 0] > t[b, 0]
        assert t[4, 1] == t[5, 1] and t[4, 0] != t[5, 0]
        # the stored order is the order of the MIXED keys, which is neither
        st, _ = host_case(k, "plain").stored()
        hi, lo = [int(x) for x in st[:, 1]], [int(x) for x in st[:, 0]]
        assert hi == sorted(hi) and lo != sorted(lo)
        assert (st != host_case(k, "plain").by_kmer()[0]).any()


@pytest.mark.parametrize("k", KS)
def test_cpu_counters_hold_every_listed_value(k):
    seen = set()
    for form in COUNTED:
        h = host_case(k, form)
        assert h.counts.min() >= 1 and h.counts.max() <= U32
        seen |= set(int(c) for c in h.counts)
    assert set(LISTED) <= seen, sorted(set(LISTED) - seen)
    if k > 2:
        assert set(LISTED) <= set(int(c) for c in host_case(k, "counted").counts)
    u = host_case(k, "union_5000")
    assert u.counts.max() == 5000 and (u.counts > 255).any()
    i = host_case(k, "intersect_70000")
    assert i.n >= 1 and i.counts.max() == 70000
    assert [host_case(k, f).n for f in UPLOADED if f.startswith("empty")] == [0, 0, 0]
    assert all(host_case(k, f"batch{j}").n > 0 for j in range(3))


def test_cpu_record_count_plus_2_62_wraps_to_the_true_size():
    for rec in (8, 12, 16, 20):            # one or two key words, with and without a counter
        for n in (0, 1, 309):
            assert (8 + (n + (1 << 62)) * rec) % (1 << 64) == 8 + n * rec
            assert n + (1 << 62) > ((8 + n * rec) - 8) // rec                      # what the loader's guard compares
    for k, form in ((31, "plain"), (31, "counted"), (33, "plain"), (33, "counted")):
        h = host_case(k, form)
        assert 8 * words(k) + 4 * h.has_counts in (8, 12, 16, 20)
        pre, suf = damaged_pair("n_plus_2_62", h.header(5), *good_body(h))
        assert PRE.unpack(pre)[7] == h.n + (1 << 62) and len(suf) == 8 + h.n * (8 * words(k) + 4 * h.has_counts)


def good_body(h):
    keys, counts = h.stored()
    return keys, (counts if h.has_counts else None)


@pytest.mark.parametrize("k,form,name", body_cases())
def test_cpu_damaged_body_differs_in_the_intended_record(k, form, name):
    h = host_case(k, form)
    keys, counts = good_body(h)
    good = keys_to_ints(keys)
    assert all(a < b for a, b in zip(good, good[1:])) and max(good) < 4 ** k
    hdr, bk, bc, where = damaged_body(name, k, h.header(5), keys, counts)
    assert bk.shape == keys.shape and (bc is None) == (counts is None)
    key_diff = np.nonzero((bk != keys).any(axis=1))[0].tolist()
    cnt_diff = [] if counts is None else np.nonzero(bc != counts)[0].tolist()
    assert sorted(key_diff + cnt_diff) == where, (name, key_diff, cnt_diff)
    assert len(pack_suf(bk, bc)) == len(pack_suf(keys, counts))                   # the right size
    assert (hdr != h.header(5)) == (name == "uniform_0")
    ints = keys_to_ints(bk)
    asc = all(a < b for a, b in zip(ints, ints[1:]))
    assert asc == (name not in ("swapped", "duplicated"))
    inside = all(v < 4 ** k for v in ints)
    assert inside == (name != "outside_key_space")
    if name == "outside_key_space" and words(k) == 2:
        assert max(keys_to_ints(unmix_np(k, bk))) >= 4 ** k                         # it unmixes to no k-mer


def test_cpu_independent_writer_and_reader_agree(tmp_path):
    for k, form in ((31, "counted"), (33, "plain"), (64, "uniform_big"), (1, "empty_counted")):
        h = host_case(k, form)
        keys, counts = good_body(h)
        prefix = str(tmp_path / f"p{k}")
        write_pair(prefix, pack_pre(h.header(0xABCDEF0123456789)), pack_suf(keys, counts))
        hdr, gk, gc = read_pair(prefix)
        assert hdr == h.header(0xABCDEF0123456789) and (gk == keys).all()
        assert (gc is None) == (counts is None) and (gc is None or (gc == counts).all())
        assert os.path.getsize(prefix + ".kmc_pre") == 48
        assert os.path.getsize(prefix + ".kmc_suf") == 8 + h.n * (8 * words(k) + 4 * h.has_counts)


# ---------------------------------------------------------------- kh_write_histogram_text (host only)
def hist_values():
    vals = [0, 2**64 - 1]
    for d in range(1, 20):
        vals += [10**d - 1, 10**d]
    return [v for v in vals if v < 2**64]


def test_write_histogram_text_lines_and_limits(E, tmp_path):
    lib = E.load_library()
    vals = hist_values()
    assert {len(str(v)) for v in vals} == set(range(1, 21))                  # every digit count of a u64
    hist = np.array([777] + vals + [5, 6, 7], dtype=np.uint64)               # hist[0] is never printed
    path = str(tmp_path / "h.txt")

    def call(cmax, length=hist.shape[0]):
        return lib.kh_write_histogram_text(path.encode(), hist.ctypes.data_as(C.POINTER(C.c_uint64)), length, cmax)
    for cmax in (1, 2, len(vals), hist.shape[0] - 2, hist.shape[0] - 1, hist.shape[0], hist.shape[0] + 40, 65535):
        assert call(cmax) == 0
        want = "".join(f"{c}\t{int(hist[c]) if c < hist.shape[0] else 0}\n" for c in range(1, cmax + 1))
        assert open(path).read() == want, cmax
        assert os.listdir(tmp_path) == ["h.txt"]
        os.remove(path)
    # a tail beyond cmax is dropped, NOT folded into line cmax (kh_histogram_file folds)
    assert call(3) == 0
    assert open(path).read() == f"1\t{vals[0]}\n2\t{vals[1]}\n3\t{vals[2]}\n"
    # a shorter array than cmax + 1: the missing lines read 0
    assert call(6, 4) == 0
    assert open(path).read() == f"1\t{vals[0]}\n2\t{vals[1]}\n3\t{vals[2]}\n4\t0\n5\t0\n6\t0\n"
    os.remove(path)
    for cmax in (0, 1 << 24):
        assert call(cmax) == E_ARG
        assert os.listdir(tmp_path) == []
    assert lib.kh_write_histogram_text(str(tmp_path / "no" / "h.txt").encode(),
                                       hist.ctypes.data_as(C.POINTER(C.c_uint64)), 4, 3) == E_IO
    assert os.listdir(tmp_path) == []


# ---------------------------------------------------------------- the sets on the device
def wrapped(eng, torch, h, with_counts):
    """A zero-copy set over torch memory, one record into buffers filled with ones: (set, what keeps it alive)."""
    mixed, cnt = h.stored()
    n, w = h.n, words(h.k)
    kbuf = torch.full(((n + 3) * w,), -1, dtype=torch.int64, device="cuda:0")
    cbuf = torch.full((n + 3,), -1, dtype=torch.int32, device="cuda:0")
    kbuf[w:(n + 1) * w] = torch.from_numpy(mixed.reshape(-1).view(np.int64)).to("cuda:0")
    cbuf[1:n + 1] = torch.from_numpy(cnt.astype(np.uint32).view(np.int32)).to("cuda:0")
    torch.cuda.synchronize()
    s = eng.wrap_device(h.k, n, kbuf.data_ptr() + 8 * w, cbuf.data_ptr() + 4 if with_counts else None,
                        uniform=h.uniform)
    return s, (kbuf, cbuf)


def upload(eng, h, with_counts):
    return eng.upload(h.k, h.keys, h.counts.astype(np.uint32) if with_counts else None)


def make_sets(eng, torch, k):
    """Every form of FORMS at one k: {form: set}, and what has to outlive them."""
    out, keep = {}, []
    for form in COUNTED + ["empty_counted"]:
        out[form] = upload(eng, host_case(k, form), True)
    for form in ("plain", "empty_plain"):
        out[form] = upload(eng, host_case(k, form), False)
    for form, v in UNIFORMS.items():
        out[form] = out["plain"].set_counts(v)
    out["empty_uniform"] = out["empty_plain"].set_counts(7)
    for with_counts, name in ((True, "batch"), (False, "plain_batch")):
        for i, s in enumerate(eng.build_batch(list(batch_texts(k)), k, with_counts=with_counts)):
            out[f"{name}{i}"] = s
    out["batch1_set_counts"] = out["batch1"].set_counts(9)
    ops = [upload(eng, h, True) for h in operand_hosts(k)[:2]] + [out["uniform_7"]]
    out["union_5000"] = eng.union_sum(ops, cs=5000)
    out["intersect_70000"] = eng.intersect(ops[0], ops[1], "sum", cs=70000)
    for form, with_counts in (("wrapped_counted", True), ("wrapped_plain", False)):
        out[form], bufs = wrapped(eng, torch, host_case(k, form), with_counts)
        keep.append(bufs)
    assert sorted(out) == sorted(FORMS)
    return out, keep


@pytest.fixture(scope="module")
def made(eng, torch):
    cache = {}

    def get(k, form):
        if k not in cache:
            cache[k] = make_sets(eng, torch, k)
        return cache[k][0][form]
    yield get
    cache.clear()


@pytest.fixture(scope="module")
def mix_id(eng, tmp_path_factory):
    """The fingerprint of the key mixing, copied from a file the library wrote (opaque to this module)."""
    prefix = str(tmp_path_factory.mktemp("mix") / "e")
    eng.upload(5, np.zeros((0, 1), dtype=np.uint64)).save(prefix)
    return read_pair(prefix)[0]["mix_id"]


def same_set(s, h, what):
    assert s.info() == h.info(), (what, s.info(), h.info())
    assert s.counter_max() == h.counter_max, (what, s.counter_max(), h.counter_max)
    keys, counts = s.download_sorted()
    wk, wc = h.by_kmer()
    assert keys.shape == wk.shape and (keys == wk).all(), (what, "keys")
    assert (counts.astype(np.int64) == wc).all(), (what, "counters")


def pair_names(d):
    return sorted(os.listdir(d))


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_batch_sets_are_views_at_offsets(made, k):
    """The three sets of one batched build share a buffer: their keys lie one behind the other, not at offset 0."""
    w = words(k)
    for name in ("batch", "plain_batch"):
        sets = [made(k, f"{name}{i}") for i in range(3)]
        ptrs = [s.device_ptrs() for s in sets]
        spans = sorted((kp, kp + 8 * w * len(s)) for (kp, _), s in zip(ptrs, sets))
        assert all(kp for kp, _ in ptrs) and len({kp for kp, _ in ptrs}) == 3
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), spans
        assert spans[-1][0] - spans[0][0] < (1 << 24)                         # one allocation, three offsets
        assert all(bool(cp) == (name == "batch") for _, cp in ptrs)
    kp1, _ = made(k, "batch1").device_ptrs()
    assert made(k, "batch1_set_counts").device_ptrs() == (kp1, None)          # set_counts shares its input's keys


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k", KS)
def test_round_trip(eng, made, mix_id, tmp_path, k, form):
    h, s = host_case(k, form), made(k, form)
    same_set(s, h, (k, form, "before the save"))
    prefix = str(tmp_path / "db")
    s.save(prefix)
    assert pair_names(tmp_path) == ["db.kmc_pre", "db.kmc_suf"]
    back = eng.load(prefix)
    assert back.info() == s.info() and back.counter_max() == s.counter_max()
    same_set(back, h, (k, form, "loaded"))
    back.save(str(tmp_path / "again"))
    assert raw_pair(str(tmp_path / "again")) == raw_pair(prefix)
    # the independent reader: this set's header, this set's n keys (none of a neighbour's), its counters
    hdr, keys, counts = read_pair(prefix)
    assert hdr == h.header(mix_id), (hdr, h.header(mix_id))
    wk, wc = h.stored()
    assert keys.shape == wk.shape and (keys == wk).all()
    assert (counts is not None) == h.has_counts
    if h.has_counts:
        assert (counts == wc).all()


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k", KS)
def test_foreign_pair_loads_to_the_same_set(eng, mix_id, tmp_path, k, form):
    h = host_case(k, form)
    prefix = str(tmp_path / "foreign")
    write_pair(prefix, pack_pre(h.header(mix_id)), pack_suf(*good_body(h)))
    back = eng.load(prefix)
    same_set(back, h, (k, form))
    back.save(str(tmp_path / "ours"))
    assert raw_pair(str(tmp_path / "ours")) == raw_pair(prefix)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [16, 33])
def test_counter_max_through_every_producer(eng, torch, made, tmp_path, k):
    text = batch_texts(k)[0]
    for c in (1, 255, 256, 5000):
        b = eng.build(text, k, cs=c)
        assert b.counter_max() == c
        assert int(b.download()[1].max()) <= c
    a, b = made(k, "counted"), made(k, "counted_b")
    for cs in (1, 255, 256, 5000, 70000, U32):
        assert eng.union_sum([a, b], cs=cs).counter_max() == cs
        assert eng.intersect(a, b, "sum", cs=cs).counter_max() == cs
        assert eng.kmers_subtract(a, made(k, "batch0"), cs=cs).counter_max() == cs
    wide = made(k, "union_5000")
    assert wide.counter_max() == 5000
    for v in (1, 7, 255, 256, 5000, 2**31 + 9, U32):                          # not the input's ceiling
        assert wide.set_counts(v).counter_max() == max(v, 255), v
    # these take the kmc_tools default without looking at the counters they are given
    h = host_case(k, "counted")
    assert h.counts.max() > 65535
    assert a.counter_max() == 255 and made(k, "wrapped_counted").counter_max() == 255
    kp, cp = a.device_ptrs()
    assert eng.from_device(k, h.n, kp, cp).counter_max() == 255
    # a loaded set: what was saved
    for form, want in (("union_5000", 5000), ("intersect_70000", 70000), ("uniform_big", 2**31 + 9), ("counted", 255)):
        prefix = str(tmp_path / form)
        made(k, form).save(prefix)
        assert eng.load(prefix).counter_max() == want == read_pair(prefix)[0]["counter_max"]


@pytest.mark.gpu
def test_saves_are_atomic_and_replace(eng, E, made, tmp_path):
    k = 33
    prefix = str(tmp_path / "db")
    made(k, "counted").save(prefix)
    assert pair_names(tmp_path) == ["db.kmc_pre", "db.kmc_suf"]
    first = raw_pair(prefix)
    made(k, "batch1_set_counts").save(prefix)                                  # over an existing pair
    assert pair_names(tmp_path) == ["db.kmc_pre", "db.kmc_suf"]
    assert raw_pair(prefix) != first
    same_set(eng.load(prefix), host_case(k, "batch1_set_counts"), "replaced")
    hdr, keys, counts = read_pair(prefix)
    assert hdr["uniform"] == 9 and counts is None and keys.shape[0] == host_case(k, "batch1_set_counts").n
    with pytest.raises(E.KhoiceError) as ei:
        made(k, "counted").save(str(tmp_path / "no_such_dir" / "db"))
    assert ei.value.code == E_IO and "no_such_dir" in str(ei.value)
    assert pair_names(tmp_path) == ["db.kmc_pre", "db.kmc_suf"] and raw_pair(prefix)[0] == pack_pre(hdr)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k", KS)
def test_sorted_dump_is_the_oracles_text(made, tmp_path, k, form):
    path = tmp_path / "dump.txt"
    made(k, form).dump_sorted(str(path))
    assert os.listdir(tmp_path) == ["dump.txt"]
    want = O.dump_sorted_text(host_case(k, form).db(), k)
    assert (want == "") == form.startswith("empty")
    assert path.read_text() == want


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["counted", "union_5000", "uniform_7", "uniform_big", "empty_counted"])
@pytest.mark.parametrize("k", KS)
def test_histogram_file_folds_above_cmax(E, made, tmp_path, k, form):
    s, db = made(k, form), host_case(k, form).db()
    path = tmp_path / "hist.txt"
    for cmax in HIST_CMAX:
        s.histogram_file(cmax, str(path))
        text = path.read_text()
        assert text == O.histogram_text(db, cmax), (k, form, cmax)
        last = int(text.splitlines()[-1].split("\t")[1])
        assert last == sum(1 for c in db.values() if c >= cmax)               # counters above cmax fold into line cmax
        assert os.listdir(tmp_path) == ["hist.txt"]
        os.remove(path)
    for cmax in (0, 1 << 24):
        with pytest.raises(E.KhoiceError) as ei:
            s.histogram_file(cmax, str(path))
        assert ei.value.code == E_ARG
        assert os.listdir(tmp_path) == []


# ---------------------------------------------------------------- damaged pairs
def refused(eng, E, prefix, code):
    with pytest.raises(E.KhoiceError) as ei:
        eng.load(prefix)
    assert ei.value.code == code, (ei.value.code, str(ei.value))
    assert os.path.basename(prefix) + ".kmc_" in str(ei.value), str(ei.value)     # the message names the file
    return str(ei.value)


@pytest.mark.gpu
@pytest.mark.parametrize("damage", DAMAGE + ["suf_missing"])
@pytest.mark.parametrize("form", ["counted", "plain"])
@pytest.mark.parametrize("k", [31, 33])
def test_damaged_pair_is_refused(eng, E, made, tmp_path, k, form, damage):
    """Record sizes 8, 12, 16 and 20: one- and two-word keys, with and without a counter."""
    good, bad = str(tmp_path / "good"), str(tmp_path / "bad")
    made(k, form).save(good)
    hdr, keys, counts = read_pair(good)
    assert hdr["n"] > 0 and (pack_pre(hdr), pack_suf(keys, counts)) == raw_pair(good)
    if damage == "suf_missing":
        write_pair(bad, pack_pre(hdr), None)
        refused(eng, E, bad, E_IO)
    else:
        write_pair(bad, *damaged_pair(damage, hdr, keys, counts))
        refused(eng, E, bad, E_FORMAT)
    same_set(eng.load(good), host_case(k, form), "the good pair after a refusal")


@pytest.mark.gpu
@pytest.mark.parametrize("k,form,name", body_cases())
def test_damaged_body_of_the_right_size_is_refused(eng, E, made, tmp_path, k, form, name):
    """A body that is not ascending, distinct, inside the key space and free of zero counters would make every
    consumer (set operations, membership, the index, partition bounds) return wrong numbers: kh_load refuses it."""
    good, bad = str(tmp_path / "good"), str(tmp_path / "bad")
    made(k, form).save(good)
    hdr, keys, counts = read_pair(good)
    bh, bk, bc, where = damaged_body(name, k, hdr, keys, counts)
    write_pair(bad, pack_pre(bh), pack_suf(bk, bc))
    assert [os.path.getsize(bad + e) for e in (".kmc_pre", ".kmc_suf")] == \
           [os.path.getsize(good + e) for e in (".kmc_pre", ".kmc_suf")]
    msg = refused(eng, E, bad, E_FORMAT)
    if where:
        assert f"record {where[-1]}" in msg, msg                              # the first offending record
    same_set(eng.load(good), host_case(k, form), "the good pair after a refusal")


# ---------------------------------------------------------------- kh_build_fasta
def fasta_texts():
    a = "ACGTTGCATTGACCGTAGGCTAACGGTTACCGATCGGATTACAGGCATCGTAGCTAACGTTAGC"
    b = "TTGACGGCATTAGCCGATCAGGCTTAACGGATCGCATTAGGCAATCGGCTAGCTTAGGCATCGA"
    rep = (a[:40] + "N") * 4 + (b[10:55] + "N") * 3       # k-mers that -ci2 -cx5 keeps and -cs3 clamps, at k = 33 too
    return {
        "crlf": f">r1 one\r\n{a}\r\n{b[:30]}\r\n>r2\r\n{rep}\r\n{a}\r\n".encode(),
        "no_final_newline": f">r1\n{a}{b}\n>r2\n{rep}{b}".encode(),
        "empty_record": f">e1\n>e2\n{a}\n{a[10:]}\n>e3\n\n>r4\n{rep}\n".encode(),
        "header_last": f">r1\n{b}\n{a}\n{rep}\n>the end".encode(),
        "gt_inside_a_line": f">r1\n{a}>{b}\n{a[:50]}>\n{rep}\n".encode(),
        "leading_blank_lines": f"\n\n\n>r1\n{a}\n\n{b}\n{rep}\n".encode(),
        "lower_case_and_n": f">r1\n{a.lower()}\n{b[:20]}N{b[20:]}\n{rep.lower()}nn{a}\n>r2\n{a[:33]}n{a[33:].lower()}{b}\n".encode(),
    }


FASTA_PARAMS = ((1, None, 255), (2, 5, 3))               # (ci, cx, cs); no cx: the engine's NO_MAX, the oracle's default


def fasta_want(data, k, ci, cx, cs):
    return O.build(data, k, ci, O.KMC_DEFAULT_CX if cx is None else cx, cs)


def test_cpu_fasta_texts_hold_their_cases():
    t = fasta_texts()
    assert t["crlf"].count(b"\r\n") == t["crlf"].count(b"\n") >= 6
    assert not t["no_final_newline"].endswith(b"\n") and t["no_final_newline"][-1:] in b"ACGT"
    assert b">e1\n>e2\n" in t["empty_record"] and b">e3\n\n>" in t["empty_record"]
    assert t["header_last"].endswith(b"\n>the end")
    assert any(b">" in ln[1:] for ln in t["gt_inside_a_line"].split(b"\n"))
    assert t["leading_blank_lines"].startswith(b"\n\n\n>")
    low = t["lower_case_and_n"]
    assert any(c in low for c in b"acgt") and b"N" in low and b"n" in low
    for name, data in t.items():
        for k in (5, 33):
            full = fasta_want(data, k, 1, None, 255)
            cut = fasta_want(data, k, 2, 5, 3)
            assert cut and len(cut) < len(full), (name, k)                     # -ci and -cx both drop something ...
            assert max(full.values()) > 5 or k == 33
            assert max(cut.values()) == 3 and min(cut.values()) >= 2           # ... and -cs clamps what is left
    assert max(fasta_want(t["crlf"], 5, 1, None, 255).values()) > 5


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(fasta_texts()))
def test_build_fasta_is_the_oracles_build(eng, E, tmp_path, name):
    data = fasta_texts()[name]
    plain, packed = tmp_path / "g.fa", tmp_path / "g.fa.gz"
    plain.write_bytes(data)
    with gzip.open(packed, "wb") as fh:
        fh.write(data)
    for k in (5, 33):
        for ci, cx, cs in FASTA_PARAMS:
            want = fasta_want(data, k, ci, cx, cs)
            wk, wc = db_to_arrays(want, k)
            for path in (plain, packed):
                s = eng.build_fasta(str(path), k, ci, E.NO_MAX if cx is None else cx, cs)
                keys, counts = s.download_sorted()
                assert keys.shape == wk.shape and (keys == wk).all(), (name, k, ci, path.name)
                assert (counts == wc).all(), (name, k, ci, path.name)
                assert s.counter_max() == cs
    if name == "crlf":
        assert b"\r\n" in data and eng.read_fasta(str(plain)).count(b"\r") == 0
