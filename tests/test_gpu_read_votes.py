"""kh_read_votes / kh_exp6_run (experiment type 6, read level) against the plain-Python restatement of
src/merge_lists.py:160-179 (tests/read_level_oracle.py): per read the votes compared as float64 with ==, the tie masks
and the unmatched counts, every read of every call; then the files of the reference (tests/golden/
merge_lists_read_level.json) through `merge_lists.main -r --seed`, `Engine.exp6_run` and the batched workflow."""
import functools
import gzip
import json
import os
import random

import numpy as np
import pytest

from khoice_amd import merge_lists as ML
from oracle import kmer_oracle as O
from tests import read_level_oracle as RL

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "merge_lists_read_level.json")))["cases"]
TILE = 256                      # positions per workgroup of k_read_masks
KS = (5, 13, 31, 32, 33, 41, 63, 64)
NSETS = (1, 2, 3, 5, 7, 64, 66)
NREADS = (0, 1, 3, 4, 5, 300)
KH_E_ARG, KH_E_KMISMATCH = -1, -5


@pytest.fixture(scope="module")
def eng():
    from khoice_amd import build as kbuild
    from khoice_amd import engine as E
    kbuild.build_library()
    e = E.Engine(0)
    yield e
    e.close()


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


@functools.lru_cache(maxsize=None)
def base_text(k):
    """5600 random bases; an even k gets reverse-complement palindromes of length k (k-mers equal to their reverse
    complement) planted every 500 bases."""
    rng = random.Random(100 + k)
    t = list(rand_seq(rng, 5600))
    if k % 2 == 0:
        for at in range(100, 5000, 500):
            half = rand_seq(rng, k // 2)
            t[at:at + k] = half + O.reverse_complement(half)
    return "".join(t)


def slice_text(k, d):
    """Set d's text: overlapping slices of the base text, so that position x of it lies in 1, 2, .. 7, 6, .. 1, 0 of
    the first seven sets as x grows; later sets are the same slices moved by a few bases."""
    lo = (d % 7) * 400 + (d // 7) * 37
    return base_text(k)[lo:lo + 2800]


def set_texts(k, nsets):
    """nsets >= 3: set 1 is empty and the last set is set 0 again (ties of two)."""
    texts = [slice_text(k, d) for d in range(nsets)]
    if nsets >= 2:
        texts[-1] = texts[0]
    if nsets >= 3:
        texts[1] = ""
    return texts


def kmers_of(text, k):
    return {RL.canonical(w) for w in O.windows(text, k)}


@functools.lru_cache(maxsize=None)
def reads_for(k):
    """300 reads of one call: the lengths 0, k-1, k, k+1; 63 .. 129 windows; 5000 bases over every depth of the slices;
    a read whose last base is the last position of a 256-position tile and one whose first base is the first of a
    tile; reads of random sequence; the rest short cuts of the base text."""
    rng = random.Random(200 + k)
    base = base_text(k)
    reads, special = [], {}
    def cut(n):
        at = rng.randrange(0, 5200 - n)
        return base[at:at + n]
    def total():
        return sum(len(r) + 1 for r in reads)
    for n in (0, k - 1, k, k + 1):
        reads.append(cut(n))
    for w in (63, 64, 65, 127, 128, 129):
        reads.append(cut(w + k - 1))
    special["long"] = len(reads)
    reads.append(base[400:5400])
    n = (-total() - 1) % TILE + 1                  # its newline is the first byte of a tile
    while n < k + 5:
        n += TILE
    special["ends_at_tile"] = len(reads)
    reads.append(cut(n))
    n = (-total() - 1) % TILE                      # the next read starts a tile
    while n < k + 5:
        n += TILE
    reads.append(cut(n))
    special["starts_at_tile"] = len(reads)
    reads.append(cut(2 * k + 70))
    for i in range(6):
        special.setdefault("random", len(reads))
        reads.append(rand_seq(rng, (k + 90, k, 3 * k, 200, k + 1, 64 + k)[i]))
    while len(reads) < 300:
        reads.append(cut(rng.randrange(0, 2 * k + 12)))
    return tuple(reads), special


def layout(reads):
    text = "".join(r + "\n" for r in reads).encode()
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    if reads:
        off[1:] = np.cumsum([len(r) + 1 for r in reads])
    return text, off


@functools.lru_cache(maxsize=None)
def want_for(k, nsets):
    reads, _ = reads_for(k)
    sets = [kmers_of(t, k) for t in set_texts(k, nsets)]
    return RL.reads_votes(reads, k, sets)


def device_sets(eng, k, nsets):
    w = 1 if k <= 32 else 2
    out = []
    for t in set_texts(k, nsets):
        out.append(eng.build(t.encode(), k, with_counts=False) if len(t) >= k else
                   eng.upload(k, np.zeros((0, w), dtype=np.uint64), None))
    return out


def compare(got, want, nsets, what):
    n = len(want)
    votes = np.array([[float(v) for v in w[0]] for w in want], dtype=np.float64).reshape(n, nsets)
    unm = np.array([w[2] for w in want], dtype=np.uint32)
    assert got["votes"].shape == votes.shape and got["votes"].dtype == np.float64
    bad = np.argwhere(got["votes"] != votes)
    assert bad.size == 0, (what, bad[:6].tolist(), [(got["votes"][tuple(b)], votes[tuple(b)]) for b in bad[:6]])
    assert (got["tie_masks"] == RL.tie_masks(want, nsets)).all(), what
    assert (got["unmatched"] == unm).all(), what


def test_the_reads_lie_where_their_names_say():
    for k in KS:
        reads, special = reads_for(k)
        _, off = layout(reads)
        assert len(reads) == 300
        assert [len(r) for r in reads[:4]] == [0, k - 1, k, k + 1]
        assert [len(r) - k + 1 for r in reads[4:10]] == [63, 64, 65, 127, 128, 129] and len(reads[special["long"]]) == 5000
        e, s = special["ends_at_tile"], special["starts_at_tile"]
        assert (int(off[e + 1]) - 1) % TILE == 0 and len(reads[e]) >= k      # the last base closes a tile
        assert int(off[s]) % TILE == 0 and len(reads[s]) >= k               # the first base opens one
        sets = [kmers_of(t, k) for t in set_texts(k, 9)]
        depth = {sum(RL.canonical(w) in s for s in sets) for w in O.windows(reads[special["long"]], k)}
        if k >= 13:                                                         # (all 512 canonical 5-mers are everywhere)
            assert depth >= set(range(0, 8))                                # len(M) = 1 .. 7 inside one read, and none
        assert len(depth) >= 4
        if k % 2 == 0:
            assert any(w == O.reverse_complement(w) for w in O.windows(reads[special["long"]], k))


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_votes_ties_and_unmatched_bit_for_bit(eng, k):
    nsets = 9                                              # seven slices, one of them empty, the last the first again
    reads, special = reads_for(k)
    want = want_for(k, nsets)
    text, off = layout(reads)
    got = eng.read_votes(text, off, k, device_sets(eng, k, nsets), want_votes=True, want_unmatched=True)
    compare(got, want, nsets, k)
    r = special["random"]
    if k >= 13:
        assert len(want[r][1]) == nsets and want[r][2] == len(reads[r]) - k + 1  # nothing matched: every set ties
    assert len(want[0][1]) == nsets and want[0][2] == 0                          # no window: every set ties
    assert any(len(w[1]) == 2 for w in want)                                     # the identical sets tie


@pytest.mark.gpu
@pytest.mark.parametrize("nsets", NSETS)
@pytest.mark.parametrize("k", (31, 33))
def test_numbers_of_sets(eng, k, nsets):
    reads, _ = reads_for(k)
    text, off = layout(reads)
    got = eng.read_votes(text, off, k, device_sets(eng, k, nsets), want_votes=True, want_unmatched=True)
    compare(got, want_for(k, nsets), nsets, (k, nsets))


@pytest.mark.gpu
@pytest.mark.parametrize("nreads", NREADS)
def test_numbers_of_reads(eng, nreads):
    k, nsets = 13, 9
    reads, _ = reads_for(k)
    text, off = layout(reads[:nreads])
    got = eng.read_votes(text, off, k, device_sets(eng, k, nsets), want_votes=True, want_unmatched=True)
    compare(got, want_for(k, nsets)[:nreads], nsets, nreads)
    only = eng.read_votes(text, off, k, device_sets(eng, k, nsets))               # the optional outputs left out
    assert set(only) == {"tie_masks"} and (only["tie_masks"] == got["tie_masks"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("k,nsets", [(31, 9), (41, 66)])
def test_several_batches_give_the_single_batch_outputs(eng, k, nsets, monkeypatch):
    reads, _ = reads_for(k)
    text, off = layout(reads)
    sets = device_sets(eng, k, nsets)
    one = eng.read_votes(text, off, k, sets, want_votes=True, want_unmatched=True)
    monkeypatch.setenv("KHOICE_READS_MAX_POS", str(len(text) // 4))
    eng.profile(True)
    n0 = eng.stats()["kernels"]["read_masks"]["launches"]
    many = eng.read_votes(text, off, k, sets, want_votes=True, want_unmatched=True)
    batches = eng.stats()["kernels"]["read_masks"]["launches"] - n0
    eng.profile(False)
    assert batches >= 3, batches
    for f in ("votes", "tie_masks", "unmatched"):
        assert (one[f] == many[f]).all(), f
    compare(many, want_for(k, nsets), nsets, (k, nsets))


@pytest.mark.gpu
@pytest.mark.parametrize("k", (32, 63))
def test_reads_in_a_device_buffer(eng, k):
    import torch
    nsets = 9
    reads, _ = reads_for(k)
    text, off = layout(reads)
    dev = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    sets = device_sets(eng, k, nsets)
    got = eng.read_votes((dev.data_ptr(), len(text)), off, k, sets, want_votes=True, want_unmatched=True)
    host = eng.read_votes(text, off, k, sets, want_votes=True, want_unmatched=True)
    for f in ("votes", "tie_masks", "unmatched"):
        assert (got[f] == host[f]).all(), f
    compare(got, want_for(k, nsets), nsets, k)


# ---------------------------------------------------------------- errors
def error_of(eng, reads, k, sets, **kw):
    from khoice_amd import engine as E
    text, off = layout(reads)
    with pytest.raises(E.KhoiceError) as ei:
        eng.read_votes(text, off, k, sets, **kw)
    return ei.value


@pytest.mark.gpu
def test_bad_symbols(eng):
    k = 21
    reads = list(reads_for(k)[0][:12])
    sets = device_sets(eng, k, 3)
    assert len(reads[4]) >= k and len(reads[9]) >= k and len(reads[1]) == k - 1
    bad = list(reads)
    bad[9] = bad[9][:3] + "N" + bad[9][4:]
    bad[4] = bad[4][:-1] + "N"
    err = error_of(eng, bad, k, sets)
    assert err.code == KH_E_ARG and "read 4 " in str(err), str(err)               # the lower of the two
    short = list(reads)
    short[1] = "N" * (k - 1)                                                      # shorter than k: no k-mer, no error
    text, off = layout(short)
    got = eng.read_votes(text, off, k, sets, want_votes=True, want_unmatched=True)
    compare(got, RL.reads_votes(short, k, [kmers_of(t, k) for t in set_texts(k, 3)]), 3, "short N")
    lower = list(reads)
    lower[6] = lower[6].lower()
    err = error_of(eng, lower, k, sets)
    assert err.code == KH_E_ARG and "read 6 " in str(err), str(err)


@pytest.mark.gpu
@pytest.mark.parametrize("k", (21, 41))
def test_check_set(eng, k):
    reads = list(reads_for(k)[0][:10])
    sets = device_sets(eng, k, 3)
    per_read = [kmers_of(r, k) for r in reads]
    everything = set().union(*per_read)
    only7 = sorted(per_read[7] - set().union(*(s for i, s in enumerate(per_read) if i != 7)))
    assert only7
    w = 1 if k <= 32 else 2

    def upload(kmers):
        keys = np.array([[(O.encode(m) >> (64 * j)) & (2**64 - 1) for j in range(w)] for m in sorted(kmers)], dtype=np.uint64)
        return eng.upload(k, keys.reshape(-1, w), None)
    text, off = layout(reads)
    full = eng.read_votes(text, off, k, sets, check=upload(everything), want_votes=True, want_unmatched=True)
    compare(full, RL.reads_votes(reads, k, [kmers_of(t, k) for t in set_texts(k, 3)], everything), 3, "check")
    err = error_of(eng, reads, k, sets, check=upload(everything - {only7[0]}))
    assert err.code == KH_E_ARG and "read 7 " in str(err), str(err)
    with pytest.raises(KeyError):
        RL.reads_votes(reads, k, [kmers_of(t, k) for t in set_texts(k, 3)], everything - {only7[0]})


@pytest.mark.gpu
def test_argument_errors(eng):
    k = 21
    reads = list(reads_for(k)[0][:5])
    err = error_of(eng, reads, k, [])
    assert err.code == KH_E_ARG
    err = error_of(eng, reads, k, device_sets(eng, k, 2) + device_sets(eng, 22, 1))
    assert err.code == KH_E_KMISMATCH
    err = error_of(eng, reads, k, device_sets(eng, k, 2), check=device_sets(eng, 22, 1)[0])
    assert err.code == KH_E_KMISMATCH
    for bad_k in (0, 65):
        assert error_of(eng, reads, bad_k, device_sets(eng, k, 2)).code == KH_E_ARG
    got = eng.read_votes(b"", np.zeros(1, dtype=np.uint64), k, device_sets(eng, k, 2), want_votes=True, want_unmatched=True)
    assert got["tie_masks"].shape == (0, 1) and got["votes"].shape == (0, 2) and got["unmatched"].shape == (0,)


# ---------------------------------------------------------------- the reference's files
def case_id(c):
    return f"n{c['num_datasets']}_k{c['k']}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", GOLDEN, ids=case_id)
def test_main_writes_the_references_files(case, tmp_path, monkeypatch):
    monkeypatch.delenv("KHOICE_READ_LEVEL_SEED", raising=False)
    n, k = case["num_datasets"], case["k"]
    for d in ("out/confusion_matrix", "out/values", "reads"):
        os.makedirs(tmp_path / d)
    pivots, inters = [], []
    for p in range(n):
        (tmp_path / "reads" / f"pivot_{p + 1}.fa").write_text(case["reads_files"][p])
        path = tmp_path / f"pivot_{p + 1}.txt"
        path.write_text(case["pivot_dumps"][p])
        pivots.append(str(path))
        for d in range(n):
            ipath = tmp_path / f"pivot_{p + 1}_intersect_dataset_{d + 1}.txt"
            ipath.write_text(case["intersection_dumps"][p * n + d])
            inters.append(str(ipath))
    (tmp_path / "pivots.txt").write_text("".join(x + "\n" for x in pivots))
    (tmp_path / "inters.txt").write_text("".join(x + "\n" for x in inters))
    rc = ML.main(["-n", str(n), "-p", str(tmp_path / "pivots.txt"), "-i", str(tmp_path / "inters.txt"),
                  "-o", str(tmp_path / "out") + "/", "-k", str(k), "-r", str(tmp_path / "reads") + "/",
                  "--seed", str(case["seed"])])
    assert rc == 0
    for name, text in case["outputs"].items():
        assert (tmp_path / "out" / name).read_text() == text, name


def golden_inputs(case, tmp_path):
    seqs = [g.encode() for gs in case["rest_of_set"] for g in gs]
    group_of = [d for d, gs in enumerate(case["rest_of_set"]) for _ in gs]
    reads = []
    for p, text in enumerate(case["reads_files"]):
        path = tmp_path / f"pivot_{p + 1}.fa"
        path.write_text(text)
        reads.append(ML.read_level_reads(str(path)))
    return seqs, group_of, reads


@pytest.mark.gpu
@pytest.mark.parametrize("case", GOLDEN, ids=case_id)
def test_exp6_run_gives_the_references_files(eng, case, tmp_path):
    n, k = case["num_datasets"], case["k"]
    seqs, group_of, reads = golden_inputs(case, tmp_path)
    res = eng.exp6_run(seqs, group_of, reads, k, cs=5000, hist_len=64)
    random.seed(case["seed"])
    assert ML.read_level_outputs(res["tie_masks"], n, str(k)) == case["outputs"]
    ref4 = eng.exp4_run(seqs, group_of, [], k, cs=5000, hist_len=64)
    assert (res["within_hist"] == ref4["within_hist"]).all() and res["within_hist"].sum() > 0
    assert (res["distinct_per_seq"] == ref4["distinct_per_seq"]).all()
    unions = [O.set_counts(O.union_sum([O.count_records([g], k) for g in gs], 5000), 1) for gs in case["rest_of_set"]]
    sets = [{O.decode(c, k) for c in u} for u in unions]
    for p in range(n):
        want = RL.reads_votes(RL.file_reads(case["reads_files"][p]), k, sets)
        assert (res["tie_masks"][p] == RL.tie_masks(want, n)).all(), p
        assert (res["unmatched"][p] == np.array([w[2] for w in want], dtype=np.uint32)).all(), p


@pytest.mark.gpu
def test_run_batched_on_a_tiny_tree(tmp_path):
    from khoice_amd.workflow import exp_type_6 as X6
    rng = random.Random(66)
    nd, seed, ks = 2, 4242, (7, 21)
    genomes, reads = {}, {}
    shared = rand_seq(rng, 500)
    for num in (1, 2):
        d = tmp_path / f"exp6_input/rest_of_set/dataset_{num}"
        os.makedirs(d)
        anc = shared + rand_seq(rng, 1500)
        for g in range(2):
            seq = "".join(c if rng.random() > 0.01 else rng.choice("ACGT") for c in anc)
            genomes[(num, f"genome_{g}")] = seq
            with gzip.open(d / f"genome_{g}.fna.gz", "wb") as fh:
                fh.write(f">genome_{g}\n{seq}\n".encode())
    for rt, n in (("illumina", 60), ("ont", 400)):
        d = tmp_path / f"exp6_input/pivot_reads_subset/{rt}"
        os.makedirs(d)
        for num in (1, 2):
            src = genomes[(num, "genome_0")]
            rs = []
            for i in range(40):
                m = rng.randrange(0, n)
                at = rng.randrange(0, len(src) - m)
                rs.append(src[at:at + m] if i % 6 else rand_seq(rng, m))
            reads[(rt, num)] = rs
            (d / f"pivot_{num}.fa").write_text("".join(f">r{i}\n{r}\n" for i, r in enumerate(rs)))
    res = X6.run_batched(str(tmp_path), ks, nd, seed)
    assert res["processes"] == 0
    for rt in ("illumina", "ont"):
        values = ""
        for k in sorted(str(k) for k in ks):
            sets = []
            for num in (1, 2):
                names = X6.rest_of_set(str(tmp_path), num)
                sets.append(set().union(*(kmers_of(genomes[(num, g)], int(k)) for g in names)))
            ties = [RL.tie_masks(RL.reads_votes(reads[(rt, num)], int(k), sets), nd) for num in (1, 2)]
            random.seed(seed)
            for name, text in ML.read_level_outputs(ties, nd, k).items():
                assert (tmp_path / f"exp6_accuracies/{rt}" / name).read_text() == text, (rt, name)
                if name.startswith("values/"):
                    values += text
        name = {"illumina": "short", "ont": "long"}[rt]
        assert open(res[f"{name}_acc"]).read() == X6.CSV_HEADER + values
        assert res[f"{name}_acc"].endswith(f"exp6_accuracies/trial_1_{name}_acc.csv")
