"""How the persistent unions (k_skm_union, k_skm2_union) come by their slots: SkmSlotFeed, khoice_amd/csrc/kh_skm_device.h.

A workgroup walks the first share of its rounds strided (blockIdx.x + j x grid: STATIC_PCT per cent of nslots / grid
rounds, at least three) and then takes claims of B consecutive slots from one device counter that skm_prepare zeroes
with the workspace.  It always holds the slot it works on, the next one
and the one after: a claim is drawn a slot before it is needed and slots at or beyond nslots count as empty.  The edges
are therefore where nslots ends relative to the grid, to the static rounds and to a claim.  KHOICE_SKM_MEAN steers
nslots (= ceil(k-mer positions / mean)) into every such range and the [skm] debug line proves that it landed there.
Everything against the C restatement, every call twice on one engine (the counter is zero again at every call)."""
import functools
import os
import re

import pytest

from khoice_amd import synth
from oracle import c_oracle as CO
from tests import util
from tests.test_gpu_skm2_hashsets import handover_case
from tests.test_gpu_skm_hashsets import deep_case, random_genomes, with_background
from tests.test_gpu_skm_union_chain import mean_for, run_checked, union_grid

pytestmark = pytest.mark.gpu

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "khoice_amd", "csrc", "kh_skm_device.h")


def knob(name):
    with open(SRC) as fh:
        return int(re.search(r"^#define %s (\d+)" % name, fh.read(), re.M).group(1))


B = knob("KH_TUNE_SKM_CLAIM")                          # slots per claim, as shipped
STATIC_PCT = knob("KH_TUNE_SKM_CLAIM_STATIC_PCT")      # share of the rounds that is walked strided


def static_rounds(nslots, grid):
    """skm_first_claimed() / grid: the strided rounds of a call."""
    return max(3, (nslots // grid) * STATIC_PCT // 100)


def rounds_with_claims(claimed):
    """The fewest full rounds (nslots // grid) of which at least `claimed` are not strided."""
    r = 3 + claimed
    while r - max(3, r * STATIC_PCT // 100) < claimed:
        r += 1
    return r


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


@functools.lru_cache(maxsize=None)
def species(length):
    """2 species x 3 genomes, cut to `length` bases each."""
    items = synth.species_set(2, 3, max(length, 1_000))
    return [t[:length] for _, _, t in items], [s - 1 for s, _, _ in items]


def grid_of(eng, k):
    """Workgroups of the persistent union: two per CU with one-word keys, three with two-word keys."""
    return union_grid(eng) if k <= 32 else 3 * eng.stats()["cus"]


fitted = util.fitted


# name -> (genome length, nslots as a function of the grid)
EDGES = {
    "one_slot": (70, lambda g: 1),                                                     # (a mean of at most 256 is taken as it is)
    "fewer_slots_than_workgroups": (50_000, lambda g: g - 3),
    "second_round_not_full": (50_000, lambda g: g + max(1, B - 1)),                    # grid < nslots < grid + B
    "static_rounds_exactly": (100_000, lambda g: 3 * g),                               # nothing left to claim
    "first_claims_cut_by_the_end": (100_000, lambda g: 3 * g + max(1, B - 1)),         # look-ahead full, claims partly empty
    "one_claim_each_and_one_slot": (200_000, lambda g: rounds_with_claims(B) * g + 1),
    "several_claims_each": (200_000, lambda g: rounds_with_claims(3 * B) * g + 1),     # no multiple of B: the end cuts the last claim
    "strided_share_above_three_rounds": (200_000, lambda g: -(-400 // STATIC_PCT) * g + 5),
}


@pytest.mark.parametrize("k", [31, 41])
@pytest.mark.parametrize("edge", list(EDGES))
def test_slot_counts_around_the_claim_walk(eng, capfd, skm_env, edge, k):
    length, count = EDGES[edge]
    grid = grid_of(eng, k)
    want = count(grid)
    (seqs, group_of) = species(length)
    seqs, mean = fitted(seqs, k, want)
    skm_env.setenv("KHOICE_SKM_MEAN", str(mean))
    nslots, did, err = run_checked(eng, capfd, seqs, group_of, k)
    print(edge, k, "grid", grid, "B", B, "strided rounds", static_rounds(nslots, grid), "nslots", nslots)
    assert nslots == want, err
    if edge in ("static_rounds_exactly", "first_claims_cut_by_the_end"):
        assert static_rounds(nslots, grid) == 3, err
    if edge == "strided_share_above_three_rounds":
        assert static_rounds(nslots, grid) == 4, err
    if edge == "several_claims_each":
        assert nslots >= 3 * B * grid and (B == 1 or nslots % B), err
        assert nslots - static_rounds(nslots, grid) * grid > 3 * B * grid, err
    assert did["skm_union"] == 1 and did["union_tagged"] == 0 and did["retries"] == 0, did


@pytest.mark.parametrize("case", ["region", "chunks"])
def test_handed_on_slot_in_the_middle_of_a_claim(eng, capfd, skm_env, case):
    """The inputs of test_handed_on_slot_between_ordinary_slots with enough slots that the claims have begun: the slots
    that go to k_skm_big (records beyond the region; more chunks than the union numbers) come to their workgroups by
    claim or strided, with ordinary slots of related background around them."""
    if case == "region":
        seqs, group_of = with_background(deep_case(31), 51)
    else:
        _, _, (s0, group_of) = handover_case(31, 1)
        bg, _ = random_genomes(len(s0), 10_000, 52, related=True)
        seqs = [b + b"N" + s for b, s in zip(bg, s0)]
        skm_env.setenv("KHOICE_SKM_SLACK", "50")
    grid = union_grid(eng)
    skm_env.setenv("KHOICE_SKM_MEAN", str(mean_for(seqs, rounds_with_claims(2 * B) * grid)))
    nslots, did, err = run_checked(eng, capfd, seqs, group_of, 31)
    assert nslots - static_rounds(nslots, grid) * grid >= 2 * B * grid, err
    assert did["retries"] == 0 and did["skm_union"] == 1 and did["union_tagged"] == 0, (did, err)
    assert did["big_slots"] > 0 and did["skm_big"] == 1, (did, err)


@pytest.mark.parametrize("k", [31, 41])
@pytest.mark.parametrize("pattern", [0x41, 0xFF], ids=lambda p: f"p{p:02X}")
def test_claims_on_poisoned_pool_memory(eng, capfd, skm_env, pattern, k):
    """The claim counter's line is zeroed by the call, not inherited: fresh and recycled blocks hold the pattern."""
    seqs, group_of = species(100_000)
    grid = grid_of(eng, k)
    skm_env.setenv("KHOICE_SKM_MEAN", str(mean_for(seqs, rounds_with_claims(2 * B) * grid)))
    eng.trim()
    skm_env.setenv("KHOICE_DEBUG_POISON", str(pattern))
    before = eng.stats()["poisoned_bytes"]
    nslots, did, err = run_checked(eng, capfd, seqs, group_of, k)
    assert eng.stats()["poisoned_bytes"] > before
    assert nslots - static_rounds(nslots, grid) * grid >= 2 * B * grid, err
    assert did["skm_union"] == 1 and did["union_tagged"] == 0 and did["retries"] == 0, did


def test_by_group_pass_over_a_second_workspace(eng, capfd, monkeypatch):
    """70 genomes in two groups: the genomes go through the union in batches of at most 64, the groups in a pass of
    their own over another workspace, each with its own zeroed counter."""
    seqs, _ = random_genomes(70, 20_000, 653, related=True)
    group_of = [0] * 35 + [1] * 35
    grid = union_grid(eng)
    monkeypatch.setenv("KHOICE_SKM_MEAN", str(mean_for(seqs, rounds_with_claims(2 * B) * grid)))
    want = CO.exp1(seqs, group_of, 31, cs=5000, hist_len=5001)
    kernels, counters = ("skm_union", "union_tagged"), ("retries",)
    got, did = util.exp1_run_stats(eng, seqs, group_of, 31, 5000, 5001, kernels, counters)
    util.exp1_same(got, want)
    again, did2 = util.exp1_run_stats(eng, seqs, group_of, 31, 5000, 5001, kernels, counters)
    util.exp1_same(again, want)
    assert did == did2 and did["skm_union"] >= 2 and did["union_tagged"] == 0 and did["retries"] == 0, did
