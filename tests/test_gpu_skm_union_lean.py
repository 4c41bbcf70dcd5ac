"""The two bodies of k_skm_union (khoice_amd/csrc/kh_skm.hip) behind a slot's third barrier, and k as its template parameter.

A slot whose merged k-mers fit the 4096-entry table (R = 1) takes the lean body, a slot with more takes the multi body
(R = ceil(N / 4096) subsets of its keys, one after the other on the same planes); ctl[7], printed as `multi-subset
slots` in the [skm] debug line, counts the latter.  The kernel is instantiated for k = 17 .. 32.  Here: every
instantiated k on the lean path; lean and multi slots in one call and in one workgroup's walk, with repeats inside a
genome; a multi slot as the last one of a walk and with the claim draws around it; the pass by group.  Everything
against the C restatement, every call twice on one engine."""
import functools
import math
import re

import numpy as np
import pytest

from khoice_amd import synth
from oracle import c_oracle as CO
from tests import util
from tests.test_gpu_skm_hashsets import minimizer_len, random_genomes, two_round_case, with_background
from tests.test_gpu_skm_union_chain import mean_for, run_checked, union_grid
from tests.test_gpu_skm_union_claims import fitted

pytestmark = pytest.mark.gpu

SKM_T = 4096                # entries of the union's main table: a slot with more merged k-mers is a multi one
UNION_CAP = 1024            # kh_skm_union_max_cap2(): records of a slot
MULTI = re.compile(r"\[skm\] k=\d+ .* overfull slots \d+ multi-subset slots (\d+)")
KS = list(range(17, 33))    # the instantiated k


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


def multi_slots(err):
    found = MULTI.findall(err)
    assert len(found) == 1, err
    return int(found[0])


# ---- the planner's rule for a slot's records (skm_plan, kh_engine.cpp), for genomes in groups of one
def per_kmer(k):
    return 2.0 / (k - minimizer_len(k) + 2) + 1.0 / 48.0       # records per k-mer position: 2 / (w + 1) + 1 / 48


def accepted_mean(k, mean):
    """The slot mean skm_plan works with when KHOICE_SKM_MEAN asks for `mean`: cut until mean x records per k-mer x
    slack + 112 fits the union's 1024 records."""
    clump = 0.5 * (k - minimizer_len(k) + 2)
    for _ in range(8):
        slack = max(1.7, 1.0 + 5.0 * math.sqrt(clump / mean))
        c2 = mean * per_kmer(k) * slack + 96 + 16
        if c2 <= UNION_CAP or mean <= 256:
            break
        mean = max(256, int(mean * UNION_CAP / c2 * 0.98))
    return mean


def largest_mean(k):
    """The largest slot mean the planner takes as asked."""
    return int((UNION_CAP - 112) / (per_kmer(k) * 1.7))


SMALLEST_K_ABOVE_T = min(k for k in KS if accepted_mean(k, SKM_T + 1) > SKM_T)


def test_planner_rule_on_the_cpu():
    """Which k can have a slot mean above the table size at all: only the widest window (k = 32, w = 18)."""
    assert [k for k in KS if accepted_mean(k, SKM_T + 1) > SKM_T] == [32]
    assert largest_mean(31) < SKM_T < largest_mean(32)
    assert accepted_mean(31, largest_mean(31)) == largest_mean(31)


@functools.lru_cache(maxsize=None)
def species():
    items = synth.species_set(2, 3, 30_000)
    return [t for _, _, t in items], [s - 1 for s, _, _ in items]


@pytest.mark.parametrize("k", KS)
def test_every_instantiated_k_on_the_lean_path(eng, capfd, skm_env, k):
    seqs, group_of = species()
    nslots, did, err = run_checked(eng, capfd, seqs, group_of, k)
    assert did == dict(skm_union=1, skm_big=0, union_tagged=0, retries=0, big_slots=0), (did, err)
    assert multi_slots(err) == 0, err


def mean_below_table(k):
    """KHOICE_SKM_MEAN a little below 4096 that the planner takes as it is."""
    return min(3950, largest_mean(k) - 20)


@functools.lru_cache(maxsize=None)
def unrelated(length, repeat):
    """Three unrelated random genomes; repeat: the second holds a segment of 4 kbp twice."""
    rng = np.random.default_rng(3100 + length % 977)
    seqs = [util.random_dna_np(rng, length) for _ in range(3)]
    if repeat:
        s = seqs[1]
        seqs[1] = s[:length // 2] + s[5_000:9_000] + s[length // 2:]
    return seqs


# 60 kbp: a few dozen slots, lean and multi ones side by side in one launch.  720 kbp: more slots than the union has
# workgroups (two per CU), so the first workgroups walk two slots on the same LDS planes, of either kind in either order.
@pytest.mark.parametrize("repeat", [False, True], ids=["plain", "repeat"])
@pytest.mark.parametrize("length", [60_000, 720_000])
@pytest.mark.parametrize("k", sorted({31, SMALLEST_K_ABOVE_T}))
def test_lean_and_multi_slots_interleaved(eng, capfd, skm_env, k, length, repeat):
    seqs = unrelated(length, repeat)
    mean = mean_below_table(k)
    assert accepted_mean(k, mean) == mean
    skm_env.setenv("KHOICE_SKM_MEAN", str(mean))
    nslots, did, err = run_checked(eng, capfd, seqs, [0, 1, 2], k)
    positions = sum(len(s) - k + 1 for s in seqs)
    assert nslots == -(-positions // mean), err               # the planner took the mean as asked (for k = 32 also above 4096: see the CPU test)
    nm = multi_slots(err)
    print("k", k, "length", length, "nslots", nslots, "multi-subset slots", nm)
    assert 0 < nm < nslots, err
    if length == 60_000:
        assert nslots <= 64, err
    else:
        assert nslots > union_grid(eng), err
    assert did == dict(skm_union=1, skm_big=0, union_tagged=0, retries=0, big_slots=0), (did, err)


def test_planner_accepts_a_mean_above_the_table(eng, capfd, skm_env):
    """At SMALLEST_K_ABOVE_T a mean above 4096 is taken as it is (every slot is then a multi one, more or less); one k
    below, the same request is cut."""
    k = SMALLEST_K_ABOVE_T
    seqs = unrelated(60_000, False)
    mean = SKM_T + 100
    assert accepted_mean(k, mean) == mean and accepted_mean(k - 1, mean) < SKM_T
    skm_env.setenv("KHOICE_SKM_MEAN", str(mean))
    nslots, did, err = run_checked(eng, capfd, seqs, [0, 1, 2], k)
    assert nslots == -(-sum(len(s) - k + 1 for s in seqs) // mean), err
    assert multi_slots(err) > nslots // 2, err
    assert did == dict(skm_union=1, skm_big=0, union_tagged=0, retries=0, big_slots=0), (did, err)
    nslots1, did1, err1 = run_checked(eng, capfd, seqs, [0, 1, 2], k - 1)
    assert nslots1 == -(-sum(len(s) - k + 2 for s in seqs) // accepted_mean(k - 1, mean)), err1


@pytest.mark.parametrize("case", ["alone", "background"])
def test_multi_slot_then_empty_slots_and_the_end(eng, capfd, skm_env, case):
    """Slot 0 is taken in two subsets (the R = 2 input of test_gpu_skm_hashsets: every key holds the minimizer A^16).
    `alone`: nothing else, fewer slots than workgroups: the multi slot is the last of its workgroup's walk, every other
    workgroup has an empty slot and the end.  `background`: 4 x grid + 1 slots over a related background, three strided
    rounds: workgroup 0 draws its first claim in the multi slot (at subset 0), the next ones in empty slots or lean ones;
    a claim lost or drawn twice leaves slots out or counts them twice."""
    _, _, (seqs, group_of) = two_round_case()
    grid = union_grid(eng)
    # (a slack that the planner clamps to regions of the union's 1024 records: the mean slot holds 2 records / 27)
    skm_env.setenv("KHOICE_SKM_SLACK", "600" if case == "alone" else "50")
    if case == "alone":
        skm_env.setenv("KHOICE_SKM_MEAN", "128")
    else:
        seqs, group_of = with_background((seqs, group_of), 53)
        seqs, mean = fitted(list(seqs), 31, 4 * grid + 1)
        skm_env.setenv("KHOICE_SKM_MEAN", str(mean))
    nslots, did, err = run_checked(eng, capfd, seqs, group_of, 31)
    if case == "alone":
        assert 1 < nslots < grid, err
    else:
        assert nslots == 4 * grid + 1, err
    d = util.skm_line(err)
    assert d["cap"] == UNION_CAP and d["overfull"] == 0 and d["errors"] == 0, d
    assert multi_slots(err) >= 1, err
    assert did == dict(skm_union=1, skm_big=0, union_tagged=0, retries=0, big_slots=0), (did, err)


@pytest.mark.parametrize("k", [31, 17])
def test_pass_by_group(eng, capfd, skm_env, k):
    """66 genomes in two groups: batches of at most 64 genomes, then the groups through the same kernel with seg_tag."""
    seqs, _ = random_genomes(66, 20_000, 661, related=True)
    group_of = [0] * 33 + [1] * 33
    want = CO.exp1(seqs, group_of, k, cs=5000, hist_len=5001)
    kernels, counters = ("skm_union", "skm_big", "union_tagged"), ("retries",)
    got, did = util.exp1_run_stats(eng, seqs, group_of, k, 5000, 5001, kernels, counters)
    util.exp1_same(got, want)
    again, did2 = util.exp1_run_stats(eng, seqs, group_of, k, 5000, 5001, kernels, counters)
    capfd.readouterr()
    util.exp1_same(again, want)
    assert did == did2 and did["skm_union"] >= 2 and did["union_tagged"] == 0 and did["retries"] == 0, did
