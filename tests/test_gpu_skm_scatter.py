"""The record build of k_skm_scatter (khoice_amd/csrc/kh_skm.hip): one descriptor per record, then the wave's records
built by its lanes in turn.  Bit-exact against the C restatement at every window width the engine picks for k = 17 .. 32,
on inputs that take the rare paths: runs longer than nmax k-mers (cut into several records), runs that go on into the
next thread and stop at a wave edge, N runs inside a record, sequences shorter than a sub-tile, and sub-tiles whose
records do not fit the staging array at once (the prefix flush).  The number of records is checked as well: it is a
function of the input alone."""
import random

import pytest

from khoice_amd import synth
from oracle import c_oracle as CO
from tests.util import random_dna

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from khoice_amd import build as kbuild
    from khoice_amd import engine as E
    kbuild.build_library()
    e = E.Engine(0)
    yield e
    e.close()


def run(eng, seqs, group_of, k, hist_len=5001):
    """(result, records written by the scatter, super-k-mer launches)"""
    eng.profile(True)
    st0 = eng.stats()
    got = eng.exp1_run(seqs, group_of, k, cs=5000, hist_len=hist_len)
    st1 = eng.stats()
    eng.profile(False)
    launches = st1["kernels"]["skm_union"]["launches"] - st0["kernels"]["skm_union"]["launches"]
    return got, st1["skm_records"] - st0["skm_records"], launches


def check(eng, seqs, group_of, k, hist_len=5001):
    want = CO.exp1(seqs, group_of, k, cs=5000, hist_len=hist_len)
    got, recs, launches = run(eng, seqs, group_of, k, hist_len)
    assert launches == 1, "the super-k-mer form did not run"
    assert (got["distinct_per_seq"] == want["distinct_per_seq"]).all()
    assert (got["within_hist"] == want["within_hist"]).all()
    assert (got["across_hist"] == want["across_hist"]).all()
    again, recs2, _ = run(eng, seqs, group_of, k, hist_len)   # same input, same records
    assert recs2 == recs > 0
    assert (again["within_hist"] == got["within_hist"]).all()
    return recs


def stress_set(seed=11):
    """Homopolymers and tandem repeats (minimizer runs far longer than nmax), N runs, short and sub-tile-sized pieces."""
    rng = random.Random(seed)
    body = random_dna(rng, 30_000)
    unit7 = random_dna(rng, 7)
    unit23 = random_dna(rng, 23)
    seqs = [
        body.encode(),
        ("A" * 3_000 + body[:4_000] + "C" * 70 + body[4_000:9_000]).encode(),     # homopolymers: one minimizer for long
        ((unit7 * 600) + body[9_000:12_000] + unit23 * 200).encode(),              # tandem repeats
        "".join(body[i:i + 37] + "N" for i in range(0, 12_000, 38)).encode(),     # an N every 38 bases: N inside records
        "".join(body[i:i + 2048] + "NN" for i in range(0, 12_000, 2050)).encode(),  # wave-sized pieces
        body[:500].encode(),                                                       # far shorter than a sub-tile
        body[:8_192 + 40].encode(),                                                # one sub-tile and a bit
        ("AC" * 3_000 + "A" * 33 + body[12_000:20_000]).encode(),
    ]
    return seqs, [i % 3 for i in range(len(seqs))]


# k -> window width: 17 .. 24 (m = 12) 6 .. 13, 25 .. 27 (m = 13) 13 .. 15, 28 .. 32 (m = 15 or 16) 14 .. 18
@pytest.mark.parametrize("k", list(range(17, 33)))
def test_scatter_every_window_width(eng, k):
    items = synth.species_set(2, 2, 40_000)
    seqs = [t for _, _, t in items]
    group_of = [s - 1 for s, _, _ in items]
    check(eng, seqs, group_of, k)


@pytest.mark.parametrize("k", [17, 21, 24, 27, 31, 32])
def test_scatter_long_runs_and_breaks(eng, k):
    seqs, group_of = stress_set()
    check(eng, seqs, group_of, k, hist_len=64)


@pytest.mark.parametrize("k", [17, 31])
def test_scatter_hard_genomes(eng, k):
    """GC-skewed genomes with pasted repeats (synth.hard_species_set): long runs at every offset."""
    items = synth.hard_species_set(2, 2, 60_000)
    seqs = [t for _, _, t in items]
    group_of = [s - 1 for s, _, _ in items]
    check(eng, seqs, group_of, k)


def test_scatter_staging_overflow(eng):
    """k = 17 (windows of 6): about 2300 records per 8192-position sub-tile on random bases, more than the 2048 staging
    entries, so most sub-tiles are appended in two rounds around a flush of the prefix of threads that fitted."""
    rng = random.Random(5)
    seqs = [random_dna(rng, 50_000).encode() for _ in range(3)]
    recs = check(eng, seqs, [0, 0, 1], 17)
    assert recs > 3 * 50_000 // 8    # short runs: many records per sub-tile


def test_scatter_shortest_windows(eng, monkeypatch):
    """k = 15, 16 (m = 11, windows of 5 and 6): the kernels take them when asked to."""
    monkeypatch.setenv("KHOICE_SKM_MIN_K", "15")
    seqs, group_of = stress_set(seed=12)
    for k in (15, 16):
        check(eng, seqs, group_of, k, hist_len=64)
