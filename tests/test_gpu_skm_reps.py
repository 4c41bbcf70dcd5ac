"""The histogram replicas of a super-k-mer run (SkmRun::hist_reps, khoice_amd/csrc/kh_engine.cpp): the workgroups of
the union add their bins to a few replicas in device memory (replica blockIdx.x % reps), which a kernel stores to the
pinned staging and the host sums.  Histograms and distinct counts against the C restatement where the union runs far
more workgroups than there are replicas, and with 72 and 73 bins, on either side of the width at which the union's
LDS stripes narrow."""
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


def check(eng, seqs, group_of, k, hist_len):
    want = CO.exp1(seqs, group_of, k, cs=5000, hist_len=hist_len)
    eng.profile(True)
    st0 = eng.stats()
    got = eng.exp1_run(seqs, group_of, k, cs=5000, hist_len=hist_len)
    st1 = eng.stats()
    eng.profile(False)
    assert st1["kernels"]["skm_union"]["launches"] - st0["kernels"]["skm_union"]["launches"] == 1, "the super-k-mer form did not run"
    assert st1["retries"] == st0["retries"]
    for f in ("distinct_per_seq", "within_hist", "across_hist"):
        assert (got[f] == want[f]).all(), f


def test_more_workgroups_than_replicas(eng):
    """3 x 200 kbp at k = 31: about 190 slots, a union workgroup each, into 8 replicas"""
    items = synth.species_set(1, 3, 200_000)
    check(eng, [t for _, _, t in items], [0, 0, 0], 31, 5001)


@pytest.mark.parametrize("nseq", (51, 52))
def test_bins_at_the_stripe_width(eng, nseq):
    """10 groups of nseq texts: nseq + 2 x 10 + 1 = 72 / 73 bins.  Texts of a group share most of their k-mers."""
    rng = random.Random(7 + nseq)
    roots = [random_dna(rng, 6_000) for _ in range(10)]
    seqs, group_of = [], []
    for i in range(nseq):
        g = i % 10
        r = roots[g]
        cut = 200 + 37 * (i // 10)
        seqs.append((r[cut:] + random_dna(rng, 300) + roots[(g + 1) % 10][:cut // 2]).encode())   # some k-mers cross the groups
        group_of.append(g)
    check(eng, seqs, group_of, 31, 16)
