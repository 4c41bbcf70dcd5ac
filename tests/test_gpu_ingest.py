"""Device-side FASTA ingest (kh_ingest_fasta: parallel inflate + stream-compaction kernels) against the
library's own CPU reader kh_read_fasta, byte for byte, AND against the oracle's independent reader
(oracle/kmer_oracle.py fasta_records: the k-mer database of every file must be the one the oracle builds from
the raw bytes), on inputs built to hit every rule of the -fm reader and every tile boundary.

The large files at the end carry a chosen byte pattern at the tile boundaries 1023|1024 and 2047|2048, where
k_fasta_scan starts another trip over 1024 tile summaries and has only `out` and `carry` to go by; they are compared
with kh_read_fasta and with a restatement of the three rules of kh_ingest.hip's header comment in plain Python.  The
unmarked test proves on the CPU that every built file has its pattern at those offsets."""
import ctypes
import functools
import gzip
import os
import random

import numpy as np
import pytest

from oracle import kmer_oracle as O
from tests.util import random_dna, set_to_db


@pytest.fixture(scope="module")
def eng():
    from khoice_amd import build as kbuild
    from khoice_amd import engine as E
    kbuild.build_library()
    e = E.Engine(0)
    yield e
    e.close()


def cases():
    rng = random.Random(2024)
    seq = random_dna(rng, 30_000, "ACGTN")
    wrapped = "\n".join(seq[i:i + 70] for i in range(0, len(seq), 70))
    out = {
        "wrapped": ">r1 some description\n" + wrapped + "\n>r2\n" + wrapped[:5000] + "\n",
        "crlf": ">r1\r\n" + wrapped.replace("\n", "\r\n") + "\r\n>r2\r\nACGT\r\n",
        "no_trailing_newline": ">r1\n" + wrapped,
        "sequence_first": wrapped[:300] + "\n>r1\nACGTACGT\n",
        "consecutive_headers": ">a\n>b\n>c\nACGT\n>d\n>e\nGGCC\n>f\n",
        "blank_lines": "\n\n>r1\n\nACGT\n\n\nTTGA\n\n>r2\n\n",
        "gt_inside_line": ">r1\nAC>GT\nA>\n>r2\n>>\nAC\n",
        "long_header": ">" + "h" * 9000 + "\nACGT\n>" + "x" * 4095 + "\n" + seq[:100] + "\n",
        "unwrapped": ">r1\n" + seq + "\n>r2\n" + seq[::-1] + "\n",
        "empty": "",
        "header_only": ">nothing here",
        "newlines_only": "\n\n\n",
        "cr_before_header": "ACGT\n\r>hdr\nGG\n\r\rAC\n",
        "lower_iupac": ">r\nacgtnryswkm\nACGT\n",
        "tile_edges": ">r\n" + "A" * 4093 + "\n>" + "h" * 4094 + "\n" + "C" * 8190 + "\n>z\nG\n",
    }
    for i in range(12):       # fuzz: every structure byte, lengths straddling tiles
        n = rng.choice([1, 15, 16, 17, 4095, 4096, 4097, 8192, 20_000, 70_000])
        out[f"fuzz{i}"] = "".join(rng.choice("ACGTN>\n\n\r" if i % 2 else "ACGT>\n") for _ in range(n))
    return out


@pytest.mark.gpu
def test_device_clean_equals_cpu_reader(eng, tmp_path):
    paths, names = [], []
    for name, text in cases().items():
        for gz in (False, True):
            p = str(tmp_path / (name + (".fna.gz" if gz else ".fa")))
            if gz:
                with gzip.open(p, "wb") as fh:
                    fh.write(text.encode())
            else:
                with open(p, "wb") as fh:
                    fh.write(text.encode())
            paths.append(p)
            names.append(name + ("/gz" if gz else "/plain"))
    for threads in (1, 7):
        texts = eng.ingest_fasta(paths, threads=threads)
        assert len(texts.seqs) == len(paths)
        for i, (p, name) in enumerate(zip(paths, names)):
            want = eng.read_fasta(p)
            got = texts.download(i)
            assert got == want, (name, threads, len(got), len(want))
        texts.free()


def oracle_cases():
    """Inputs on which the oracle's reader and the product's are specified alike: line ends LF or CRLF (a CR that
    is not followed by LF is outside what either documents: the oracle keeps it as a run-breaking symbol, the
    product drops it — product-defined, covered by the byte comparison above)."""
    rng = random.Random(77)
    out = {name: text for name, text in cases().items() if "\r" not in text}
    out["crlf"] = cases()["crlf"]
    for i in range(16):       # fuzz without stray CRs: every structure byte, lengths straddling the 4 KB tiles
        n = rng.choice([1, 15, 16, 17, 4095, 4096, 4097, 8191, 8192, 8193, 20_000, 70_000])
        text = "".join(rng.choice("ACGTN>\n\n" if i % 2 else "ACGTacgtRY>\n") for _ in range(n))
        out[f"ofuzz{i}"] = text
        if i % 4 == 0:
            out[f"ofuzz{i}_crlf"] = text.replace("\n", "\r\n")
    return out


@pytest.mark.gpu
def test_device_clean_gives_the_oracles_kmers(eng, tmp_path):
    """f2 against an implementation that shares no code with the product: raw file bytes -> oracle FASTA reader
    -> oracle counting, versus file -> kh_ingest_fasta (device clean) -> kh_build_batch, and versus file ->
    kh_read_fasta -> kh_build_batch."""
    items = list(oracle_cases().items())
    paths = []
    for j, (name, text) in enumerate(items):
        p = str(tmp_path / (name + (".fna.gz" if j % 2 else ".fa")))
        with (gzip.open(p, "wb") if j % 2 else open(p, "wb")) as fh:
            fh.write(text.encode())
        paths.append(p)
    texts = eng.ingest_fasta(paths, threads=5)
    for k in (3, 12):
        dev_sets = eng.build_batch(texts.seqs, k)
        host_sets = eng.build_batch([eng.read_fasta(p) for p in paths], k)
        for (name, text), ds, hs in zip(items, dev_sets, host_sets):
            want = O.count_records(O.fasta_records(text.encode()), k)
            assert set_to_db(ds) == want, (name, k, "device clean")
            assert set_to_db(hs) == want, (name, k, "host reader")
    texts.free()


@pytest.mark.gpu
def test_ingested_texts_feed_the_fused_step(eng, tmp_path):
    """gz genomes -> kh_ingest_fasta -> kh_exp1_run on the resident texts == the same from host texts."""
    from khoice_amd import synth
    root = str(tmp_path)
    synth.write_dataset_tree(root, 3, 2, 150_000)
    names = [(num, g[:-len(".fna.gz")]) for num in (1, 2, 3)
             for g in sorted(os.listdir(os.path.join(root, f"data/dataset_{num}")))]
    paths = [os.path.join(root, f"data/dataset_{n}/{g}.fna.gz") for n, g in names]
    group_of = [n - 1 for n, _ in names]
    texts = eng.ingest_fasta(paths)
    host = [eng.read_fasta(p) for p in paths]
    a = eng.exp1_run(texts.seqs, group_of, 31, hist_len=64)
    b = eng.exp1_run(host, group_of, 31, hist_len=64)
    assert (a["within_hist"] == b["within_hist"]).all() and (a["across_hist"] == b["across_hist"]).all()
    assert (a["distinct_per_seq"] == b["distinct_per_seq"]).all()
    texts.free()
    with pytest.raises(Exception):
        eng.ingest_fasta([paths[0], os.path.join(root, "missing.fna.gz")])


@pytest.mark.gpu
def test_batched_runner_without_databases_matches_with_databases(tmp_path):
    """run_batched(keep_databases=False) — device ingest, fused step, histogram files written from
    arrays, CSV stage fed from memory — gives byte-identical CSVs and histogram files."""
    from khoice_amd import synth
    from khoice_amd.workflow import exp_type_1 as W
    outs = []
    for keep in (True, False):
        root = str(tmp_path / f"keep_{keep}")
        os.makedirs(root)
        synth.write_dataset_tree(root, 3, 2, 120_000)
        res = W.run_batched(root, [21, 31], 3, keep_databases=keep)
        hist = {}
        for k in (21, 31):
            for num in (1, 2, 3):
                rel = f"step_4/k_{k}/dataset_{num}/dataset_{num}_k{k}_hist.txt"
                hist[rel] = open(os.path.join(root, rel)).read()
            rel = f"step_8/k_{k}/all_datasets_k{k}_hist.txt"
            hist[rel] = open(os.path.join(root, rel)).read()
        outs.append((res["within"], res["across"], hist))
    assert outs[0][0] == outs[1][0] and outs[0][1] == outs[1][1]
    assert outs[0][2] == outs[1][2]


# ---------------------------------------------------------------- the second trip of k_fasta_scan
TILE = 4096
TRIP = 1024 * TILE                    # bytes that one trip of k_fasta_scan covers: also the read piece of ingest_read
SIZES = {"1024_tiles": TRIP, "1024_tiles_plus_1": TRIP + 1, "2049_tiles": 2049 * TILE}
# way -> (bytes that end exactly at the boundary, bytes that start there); the first byte after the boundary alone is
# what the file of 1024 tiles + 1 byte keeps
WAYS = {
    "header_at_boundary_separator_due": (b"ACGTTGCA\n", b">h2 starts a tile\nGGCC\n"),
    "header_at_boundary_nothing_kept": (b"ACGT\n>" + b"e" * 6000 + b"\n\n\r\n", b">h2 follows a header\nGGCC\n"),
    "inside_header_line": (b"ACGT\n>a header that runs over the bound", b"ary and on\nGGCC\n"),
    "inside_sequence_line": (b"ACGTACGTAC", b"GTTTGACA\nGGCC\n"),
    "between_cr_and_lf": (b"ACGTTGCA\r", b"\n>h2\r\nGGCC\r\n"),
}


def clean_rules(raw):
    """The three rules of kh_ingest.hip's header comment, line by line."""
    out, kept_since_header = [], False
    for line in raw.split(b"\n"):
        if line.lstrip(b"\r")[:1] == b">":                 # 1. a header line is dropped ...
            if kept_since_header:
                out.append(b"\n")                          # 3. ... after one separator, if sequence was kept since the last
            kept_since_header = False
        else:
            kept = line.replace(b"\r", b"")                # 2. a sequence line is kept but for its line ends
            if kept:
                out.append(kept)
                kept_since_header = True
    return b"".join(out)


def filler(nbytes, rng, header_free_tail=3 * TILE):
    """Exactly nbytes of whole lines: rows of 70 bases, about one header row in 400 (none in the last three tiles, so
    that what a boundary pattern needs from earlier tiles has to be carried), a last line that takes the remainder."""
    assert nbytes >= 142
    nrows = nbytes // 71 - 1
    rows = np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.choice(5, size=(nrows, 71), p=[.248, .248, .248, .248, .008])]
    rows[:, 70] = ord("\n")
    hdr = np.nonzero(rng.random(nrows) < 0.0025)[0]
    hdr = hdr[hdr < nrows - header_free_tail // 71 - 2]
    rows[hdr, 0] = ord(">")
    rows[hdr, 1:70] = ord("h")
    rest = nbytes - nrows * 71
    last = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=rest)].copy()
    last[-1] = ord("\n")
    return rows.tobytes() + last.tobytes()


@functools.lru_cache(maxsize=None)
def boundary_file(way, size):
    before, after = WAYS[way]
    rng = np.random.default_rng(len(before) * 1000 + len(after))
    total = SIZES["1024_tiles_plus_1" if size == "1024_tiles" else size]
    parts, pos = [], 0
    for b in (TRIP, 2 * TRIP):
        if b < total:
            tail = after[:total - b] if total - b < len(after) else after
            parts += [filler(b - len(before) - pos, rng), before, tail]
            pos = b + len(tail)
    if total > pos:
        parts.append(filler(total - pos, rng))
    raw = b"".join(parts)
    assert len(raw) == total
    return raw[:SIZES[size]]


def line_start(raw, p):
    return p == 0 or raw[p - 1:p] == b"\n"


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("way", list(WAYS))
def test_cpu_boundary_files_have_their_pattern(way, size):
    raw = boundary_file(way, size)
    n = len(raw)
    assert n == SIZES[size] and (n + TILE - 1) // TILE == {"1024_tiles": 1024, "1024_tiles_plus_1": 1025, "2049_tiles": 2049}[size]
    before, after = WAYS[way]
    bounds = [b for b in (TRIP, 2 * TRIP) if b <= n]
    assert len(bounds) == (2 if size == "2049_tiles" else 1)
    for b in bounds:
        assert raw[b - len(before):b] == before and raw[b:b + len(after)] == after[:n - b]
        last_hdr = raw.rfind(b"\n>", 0, b)
        if way == "header_at_boundary_separator_due":
            assert line_start(raw, b) and raw[b - 2:b - 1] in b"ACGT"
            assert b - last_hdr > 3 * TILE                       # the sequence kept since the last header lies tiles back
        elif way == "header_at_boundary_nothing_kept":
            assert line_start(raw, b) and raw[last_hdr + 1:last_hdr + 3] == b">e"
            assert b - last_hdr > TILE + 1000                    # a whole tile inside that header line
            assert raw[last_hdr + 1:b].count(b"\n") == 3 and clean_rules(raw[last_hdr + 1:b]) == b""
        elif way == "inside_header_line":
            assert last_hdr + 1 == b - len(before) + 5 and b"\n" not in raw[last_hdr + 1:b]
        elif way == "inside_sequence_line":
            assert not line_start(raw, b) and raw[raw.rfind(b"\n", 0, b) + 1:raw.rfind(b"\n", 0, b) + 2] != b">"
            assert raw[b - 1:b] in b"ACGT" and after[:1] in b"ACGT"
        else:
            assert raw[b - 1:b] == b"\r" and after[:1] == b"\n"
        if b < n:
            assert raw[b:b + 1] == after[:1]
    # the rules give a text without two separators in a row, none at the start, and shorter than the file
    want = clean_rules(raw)
    assert b"\n\n" not in want and not want.startswith(b"\n") and b"\r" not in want and b">" not in want
    assert 0.9 * n < len(want) < n


def download(texts, i):
    """DeviceTexts.download into a numpy buffer (megabytes at a time)."""
    ptr, n = texts.seqs[i]
    buf = np.empty(max(n, 1), dtype=np.uint8)
    if n:
        rc = ctypes.CDLL("libamdhip64.so").hipMemcpy(ctypes.c_void_p(buf.ctypes.data), ctypes.c_void_p(ptr),
                                                     ctypes.c_size_t(n), 2)             # hipMemcpyDeviceToHost
        assert rc == 0, rc
    return buf[:n].tobytes()


def first_difference(a, b):
    if len(a) != len(b):
        return ("length", len(a), len(b))
    x, y = np.frombuffer(a, dtype=np.uint8), np.frombuffer(b, dtype=np.uint8)
    d = np.nonzero(x != y)[0]
    return None if not d.size else ("byte", int(d[0]), a[max(0, int(d[0]) - 20):int(d[0]) + 20], b[max(0, int(d[0]) - 20):int(d[0]) + 20])


@pytest.mark.gpu
@pytest.mark.parametrize("way", list(WAYS))
def test_scan_carries_state_into_its_next_trip(eng, tmp_path, way):
    paths, wants = [], []
    for size in SIZES:
        raw = boundary_file(way, size)
        p = str(tmp_path / f"{way}_{size}.fa")
        with open(p, "wb") as fh:
            fh.write(raw)
        paths.append(p)
        wants.append(clean_rules(raw))
        assert first_difference(eng.read_fasta(p), wants[-1]) is None, (way, size, "host reader against the rules")
    for threads in (1, 3):
        texts = eng.ingest_fasta(paths, threads=threads)
        for i, size in enumerate(SIZES):
            assert texts.seqs[i][1] == len(wants[i]), (way, size, threads, texts.seqs[i][1], len(wants[i]))
            assert first_difference(download(texts, i), wants[i]) is None, (way, size, threads)
        texts.free()


@pytest.mark.gpu
def test_gzip_of_several_members(eng, tmp_path):
    """Concatenated gzip members: the size in the trailer is the last member's, so the host buffer of ingest_read has to
    grow while it reads (from nothing when the trailer is below the file size), across 4 MiB read pieces."""
    rng = np.random.default_rng(5)
    third = TRIP // 2 + 12345
    a = filler(third, rng)[:-9] + b"ACGTACGT"                # member 1 ends inside a sequence line
    b = b"GGCC\n" + filler(third, rng)                      # member 2 ends with a line end:
    c = b">planted at a member seam\n" + filler(third, rng)   # ... and member 3 opens with a header line
    tiny = b"TTGACA\n>last\nAC"
    files = {"three_members": [a, b, c], "tiny_last_member": [a + b, c, tiny], "tiny_first_member": [tiny, c + a]}
    paths, wants = [], []
    for name, members in files.items():
        p = str(tmp_path / (name + ".fna.gz"))
        with open(p, "wb") as fh:
            for m in members:
                fh.write(gzip.compress(m, compresslevel=1))
        raw = b"".join(members)
        assert len(raw) > TRIP and os.path.getsize(p) < len(raw)
        paths.append(p)
        wants.append(clean_rules(raw))
    assert b"ACGTACGTGGCC" in wants[0] and b"\n" + clean_rules(c)[:20] in wants[0]
    with open(paths[1], "rb") as fh:                             # the trailer of this file is no guide at all
        assert int.from_bytes(fh.read()[-4:], "little") == len(tiny) < os.path.getsize(paths[1])
    for p, want in zip(paths, wants):
        assert first_difference(eng.read_fasta(p), want) is None, (p, "host reader against the rules")
    for threads in (1, 3):
        texts = eng.ingest_fasta(paths, threads=threads)
        for i, name in enumerate(files):
            assert first_difference(download(texts, i), wants[i]) is None, (name, threads)
        texts.free()
