"""k_skm_union (khoice_amd/csrc/kh_skm.hip): the paths of its read-out.

Both tables of the kernel share one index space (entry i of the second table is entry T + i of every plane), a field
of `made` is a valid bit and that joint index, and the read-out exchanges zero into both mask planes at it without
asking which table it is.  A mask is evaluated with its FIRST group outside the loop: the group's bin is counted, and
if no lane of the wave has a bit outside its first group's mask the wave leaves (one uniform test); otherwise the
lanes strip the first group and run the loop for the rest.  The group table holds a group's first bin as a byte offset.

What can go wrong: a mask left behind at an index >= T (it lands in the next slot's bins, so every workgroup walks at
least three slots here), the index of the main table's last entries or the second table's first ones, a wave in which
ONE lane has a second group, a first set bit in the high half of the mask, a group across bits 31 / 32, a bin offset
scaled for another stripe width, and the three places the read-out stands in (deferred, in place for multi-subset
slots, behind the loop).  Every case: against the C restatement bit for bit, a second call that must equal the first,
and the fast form must have answered.  The last cases run the shared read-out of the other super-k-mer kernels
(k_skm2_union at k = 41, k_skm_cross) on the same inputs."""
import functools

import numpy as np
import pytest

from tests import util
from tests.test_gpu_exp3_skm import check as exp3_check
from tests.test_gpu_exp3_skm import small_species, species_answer
from tests.test_gpu_skm2_hashsets import handover_case
from tests.test_gpu_skm_hashsets import deep_case, random_genomes, with_background
from tests.test_gpu_skm_union_chain import run_checked, union_grid
from tests.test_gpu_skm_union_overlap import FAST, MULTI, UNION_CAP, per_kmer
from tests.test_gpu_skm_union_roundtrips import SIX, mixed_groups, several_slots

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from khoice_amd import build as kbuild
    from khoice_amd import engine as E
    kbuild.build_library()
    e = E.Engine(0)
    yield e
    e.close()


@pytest.fixture
def skm_env(monkeypatch):
    monkeypatch.setenv("KHOICE_SKM_DEBUG", "1")
    return monkeypatch


# ---- 1. both ends of the joint index
@pytest.mark.parametrize("k", [20, 24, 31, 32])
def test_both_ends_of_the_joint_index(eng, capfd, skm_env, k):
    """The deep-tier families of test_gpu_skm_hashsets in slot 0, inside the union's region.  k = 20 and 31: homes
    4056 .. 4095, the main table's last entries, wrapping; k = 32: homes 0 .. 23 with the poly-A key at home 0; k = 24
    also the family of one hash, whose keys fill their chain of the second table (joint indices T .. T + T2 - 1) and go
    back to the main table.  Three slots per workgroup: a mask that the read-out did not take shows in the next slot."""
    seqs, group_of = with_background(deep_case(k), 1200 + k)
    skm_env.setenv("KHOICE_SKM_SLACK", "50")               # regions of the union's 1024 records
    want = several_slots(eng, skm_env, seqs, 3)
    nslots, did, err = run_checked(eng, capfd, seqs, group_of, k)
    assert nslots >= want, err
    assert did == FAST, (did, err)


# ---- 2. the uniform exit, both ways in one call
@functools.lru_cache(maxsize=None)
def one_shared_piece():
    """Six groups of two unrelated genomes of 20 kb: every k-mer sits in one group, and every wave leaves at the
    uniform test — but for ONE piece of 40 bases of genome 0 (group 0) that stands in genome 7 (group 3) as well: its
    40 - k + 1 k-mers (none at k = 41: there the piece only makes its neighbours' records differ) have a second group,
    in a handful of waves, one or two lanes each."""
    seqs, _ = random_genomes(12, 20_000, 1212, related=False)
    g = bytearray(seqs[7])
    g[9_000:9_040] = seqs[0][5_000:5_040]
    seqs[7] = bytes(g)
    return seqs, [j // 2 for j in range(12)]


@pytest.mark.parametrize("k", [31, 41])
def test_one_lane_with_a_second_group(eng, capfd, skm_env, k):
    seqs, group_of = one_shared_piece()
    want = several_slots(eng, skm_env, seqs, 3)
    nslots, did, err = run_checked(eng, capfd, seqs, group_of, k)
    assert nslots >= want, err
    assert did == FAST, (did, err)


@pytest.mark.parametrize("k", [31, 41])
@pytest.mark.parametrize("cs", [2, 3])
@pytest.mark.parametrize("sshift", [2, 1, 0])
def test_one_two_and_all_groups_in_the_same_slots(eng, capfd, skm_env, sshift, cs, k):
    """Sequence shared by all groups, by two groups and by one group in the same slots (`mixed_groups` of the
    round-trip tests, with its group counts): waves that leave at the uniform test and waves that run the loop for
    one, for two and for every group stand side by side, at every stripe width of the bins, and both clamps pass."""
    seqs, group_of = mixed_groups(SIX[sshift])
    nbins = len(seqs) + 2 * (max(group_of) + 1) + 1
    assert (2 if nbins <= 72 else 1 if nbins <= 144 else 0) == sshift
    want = several_slots(eng, skm_env, seqs, 3)
    nslots, did, err = run_checked(eng, capfd, seqs, group_of, k, cs=cs, hist_len=64)
    assert nslots >= want, err
    assert did == FAST, (did, err)


# ---- 3. the halves of the mask
HALVES = {"36_and_4": [0] * 36 + [1] * 4,                  # group 0 across bits 31 / 32, group 1 wholly in 36 .. 39
          "30_4_6": [0] * 30 + [1] * 4 + [2] * 6}          # group 1 is operands 30 .. 33, group 2 wholly in 34 .. 39


@pytest.mark.parametrize("k", [31, 41])
@pytest.mark.parametrize("groups", sorted(HALVES))
def test_first_group_in_the_high_half(eng, capfd, skm_env, groups, k):
    """40 related genomes of 20 kb.  A k-mer of the last group alone has its first set bit in the high half of the
    mask with the low half zero; the group across bits 31 / 32 is counted from both halves and stripped from both.
    Genome 35 is genome 3 again (the same content in the other half), genome 1 is genome 0 again."""
    seqs, _ = random_genomes(40, 20_000, 1313, related=True)
    seqs[1] = seqs[0]
    seqs[35] = seqs[3]
    want = several_slots(eng, skm_env, seqs, 3)
    nslots, did, err = run_checked(eng, capfd, seqs, HALVES[groups], k)
    assert nslots >= want, err
    assert did == FAST, (did, err)


# ---- 4. the bodies in any order
def test_multi_subset_slot_among_lean_ones(eng, capfd, skm_env):
    """Three unrelated genomes at k = 32 with a mean near the table size (the case of the overlap test, other
    sequence, two groups): multi-subset slots read out in place, lean ones behind the next slot's first barrier, the
    last one of a walk behind the loop — all through the same code, and the masks are zero whoever comes next."""
    k = 32
    rng = np.random.default_rng(1414)
    seqs = [util.random_dna_np(rng, 720_000) for _ in range(3)]
    mean = min(3950, int((UNION_CAP - 112) / (per_kmer(k) * 1.7)) - 20)
    skm_env.setenv("KHOICE_SKM_MEAN", str(mean))
    nslots, did, err = run_checked(eng, capfd, seqs, [0, 1, 1], k)
    assert nslots == -(-sum(len(s) - k + 1 for s in seqs) // mean) and nslots > union_grid(eng), err
    found = MULTI.findall(err)
    assert len(found) == 1 and 0 < int(found[0]) < nslots, err
    assert did == FAST, (did, err)


def test_handed_on_slot_among_lean_ones(eng, capfd, skm_env):
    """Slot 0 makes one chunk more than the union numbers and goes to k_skm_big (which reads out through the shared
    struct, with a group table of its own); the workgroup that met it reads out its previous slot before and goes on
    to lean slots behind it."""
    _, _, (s0, group_of) = handover_case(31, 1)
    bg, _ = random_genomes(len(s0), 10_000, 1415, related=True)
    seqs = [b + b"N" + s for b, s in zip(bg, s0)]
    skm_env.setenv("KHOICE_SKM_SLACK", "50")               # regions of the union's 1024 records
    want = several_slots(eng, skm_env, seqs, 3)
    nslots, did, err = run_checked(eng, capfd, seqs, group_of, 31)
    assert nslots >= want, err
    assert did["retries"] == 0 and did["skm_union"] == 1 and did["union_tagged"] == 0, (did, err)
    assert did["big_slots"] > 0 and did["skm_big"] == 1, (did, err)


# ---- 5. the shared read-out of the other kernels: k_skm_cross
def test_cross_read_out(eng, monkeypatch):
    """One kh_exp3_run call at k = 31 through k_skm_cross, against the oracle of tests/test_gpu_exp3_skm.py."""
    monkeypatch.setenv("KHOICE_EXP3_SKM", "1")
    seqs, group_of, pivots = small_species()
    exp3_check(eng, seqs, group_of, pivots, 31, want=species_answer(31))
