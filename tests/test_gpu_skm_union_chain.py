"""The per-slot chain of k_skm_union (khoice_amd/csrc/kh_skm.hip) over SEVERAL slots of one persistent workgroup.

The kernel leaves its mask planes zero by reading every mask with an exchange that stores zero instead of clearing
them per slot.  That only matters from a workgroup's second slot on, and the other small tests have fewer slots than
workgroups: here KHOICE_SKM_MEAN makes the slots small enough that every workgroup walks several, with chunk counts on both sides of a pass boundary, with a slot that is handed to k_skm_big in between, and
with genomes repeated inside a group (repeat counters, mask bits already set).  Everything against the C restatement."""
import numpy as np
import pytest

from khoice_amd import synth
from tests import util
from tests.test_gpu_skm2_hashsets import handover_case
from tests.test_gpu_skm_hashsets import deep_case, random_genomes, with_background

pytestmark = pytest.mark.gpu

KERNELS, COUNTERS = util.UNION_KERNELS, util.UNION_COUNTERS
UNION_NT = 1024            # threads of k_skm_union = chunks of one pass
NSLOTS = util.SKM_NSLOTS


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


def union_grid(eng):
    return 2 * eng.stats()["cus"]          # kh_skm_union_per_cu() workgroups per CU, persistent


run_checked = util.run_checked


def mean_for(seqs, nslots):
    """KHOICE_SKM_MEAN (k-mer positions per slot) that gives at least nslots slots."""
    return max(64, sum(len(s) for s in seqs) // (nslots + nslots // 8))


@pytest.mark.parametrize("k", [31, 21])
def test_several_slots_per_workgroup(eng, capfd, skm_env, k):
    items = synth.species_set(2, 3, 200_000)
    seqs = [t for _, _, t in items]
    group_of = [s - 1 for s, _, _ in items]
    grid = union_grid(eng)
    skm_env.setenv("KHOICE_SKM_MEAN", str(mean_for(seqs, 3 * grid)))
    nslots, did, err = run_checked(eng, capfd, seqs, group_of, k)
    assert nslots >= 3 * grid, err
    assert did["skm_union"] == 1 and did["union_tagged"] == 0 and did["retries"] == 0, did


@pytest.mark.parametrize("passes", [1, 2])
def test_chunks_around_a_pass_boundary(eng, capfd, skm_env, passes):
    """Unrelated genomes (nothing merges), the mean slot at about `passes` x 1024 chunks: slots of one pass more and
    one pass fewer occur in the same call.  (k = 31: records of 8.5 k-mers on average make 4.7 chunks of two, 0.55
    chunks per k-mer position.)"""
    rng = np.random.default_rng(77)
    seqs = [util.random_dna_np(rng, 60_000) for _ in range(4)]
    mean = int(passes * UNION_NT / 0.55)
    skm_env.setenv("KHOICE_SKM_MEAN", str(mean))
    nslots, did, err = run_checked(eng, capfd, seqs, [0, 0, 1, 1], 31)
    assert nslots >= 4 * 60_000 // mean - 1, err
    assert did["skm_union"] == 1 and did["union_tagged"] == 0 and did["retries"] == 0, did


@pytest.mark.parametrize("case", ["region", "chunks"])
def test_handed_on_slot_between_ordinary_slots(eng, capfd, skm_env, case):
    """Slot 0 goes to k_skm_big — its records exceed the region (`region`: the deep-tier families of
    test_gpu_skm_hashsets), or they fit and make more chunks than the union numbers (`chunks`: the hand-over case of
    test_gpu_skm2_hashsets) — while the same workgroup goes on to ordinary slots of related background sequence."""
    if case == "region":
        seqs, group_of = with_background(deep_case(31), 51)
    else:
        _, _, (s0, group_of) = handover_case(31, 1)
        bg, _ = random_genomes(len(s0), 10_000, 52, related=True)
        seqs = [b + b"N" + s for b, s in zip(bg, s0)]
        skm_env.setenv("KHOICE_SKM_SLACK", "50")       # regions of the union's 1024 records
    grid = union_grid(eng)
    skm_env.setenv("KHOICE_SKM_MEAN", str(mean_for(seqs, grid + grid // 2)))
    nslots, did, err = run_checked(eng, capfd, seqs, group_of, 31)
    assert nslots > grid, err
    assert did["retries"] == 0 and did["skm_union"] == 1 and did["union_tagged"] == 0, (did, err)
    assert did["big_slots"] > 0 and did["skm_big"] == 1, (did, err)


def test_genome_repeated_inside_a_group(eng, capfd, skm_env):
    """Related genomes, one of them twice in its group and once more in the other group: identical records of one genome
    tag merge with a bit already set, and k-mers meet masks that hold their bit."""
    items = synth.species_set(2, 3, 120_000)
    seqs = [t for _, _, t in items]
    group_of = [s - 1 for s, _, _ in items]
    seqs += [seqs[0], seqs[0][:70_000] + b"N" + seqs[4][10_000:90_000], seqs[0]]
    group_of += [0, 0, 1]
    grid = union_grid(eng)
    skm_env.setenv("KHOICE_SKM_MEAN", str(mean_for(seqs, 2 * grid)))
    nslots, did, err = run_checked(eng, capfd, seqs, group_of, 31)
    assert nslots >= 2 * grid, err
    assert did["skm_union"] == 1 and did["union_tagged"] == 0 and did["retries"] == 0, did
