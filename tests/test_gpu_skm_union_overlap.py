"""k_skm_union (khoice_amd/csrc/kh_skm.hip) with a lean slot's read-out moved behind the NEXT slot's first barrier:
the read-out of slot s and the merge of identical records of slot s + 1 share one barrier interval of a persistent
workgroup's walk.

What can go wrong is what one slot leaves for the next: `made` carried across the staging, a read-out that is skipped
or done twice (empty slots, multi-subset slots and slots handed to k_skm_big in between, the walk's last slot), masks
that are not zero when the next insertion begins, repeats counted by the merge and by the read-out in one interval.
KHOICE_SKM_MEAN makes the slots small enough that every workgroup walks several.  Every case: against the C
restatement bit for bit, a second call that must equal the first, and the fast form must have answered.

Inside the interval a wave with both jobs merges first, at the raised priority of the merge."""
import functools
import re

import numpy as np
import pytest

from khoice_amd import synth
from oracle import c_oracle as CO
from tests import util
from tests.test_gpu_skm2_hashsets import handover_case
from tests.test_gpu_skm_hashsets import deep_case, minimizer_len, random_genomes, with_background
from tests.test_gpu_skm_union_chain import mean_for, run_checked, union_grid

pytestmark = pytest.mark.gpu

SKM_T = 4096                # entries of the union's main table: a slot with more merged k-mers is a multi-subset one
UNION_CAP = 1024            # records of a slot: one per thread
MULTI = re.compile(r"\[skm\] k=\d+ .* overfull slots \d+ multi-subset slots (\d+)")
FAST = dict(skm_union=1, skm_big=0, union_tagged=0, retries=0, big_slots=0)


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
def species():
    """2 species x 3 genomes x 200 kb: the genomes of a species share most records, so the merge has work."""
    items = synth.species_set(2, 3, 200_000)
    return [t for _, _, t in items], [s - 1 for s, _, _ in items]


# ---- 1. several slots per workgroup, records that merge: the template's edges, the headline, the runtime-k kernel
@pytest.mark.parametrize("k", [17, 21, 31, 32, 16])
def test_several_slots_per_workgroup(eng, capfd, skm_env, k):
    seqs, group_of = species()
    grid = union_grid(eng)
    if k == 16:
        skm_env.setenv("KHOICE_SKM_MIN_K", "15")          # the instantiation that takes k from the job
    skm_env.setenv("KHOICE_SKM_MEAN", str(mean_for(seqs, 4 * grid)))
    nslots, did, err = run_checked(eng, capfd, seqs, group_of, k)
    assert nslots >= 4 * grid, err
    assert did == FAST, (did, err)


# ---- 2. empty and tiny slots between full ones
def test_empty_and_tiny_slots_between_full_ones(eng, capfd, skm_env):
    """64 k-mer positions per slot on average: a few records in most slots, none in some (R0 = 0: nothing to merge,
    no insertion, nothing left for the next slot to read out) — in every workgroup's walk, dozens of times."""
    seqs, group_of = species()
    skm_env.setenv("KHOICE_SKM_MEAN", "64")
    nslots, did, err = run_checked(eng, capfd, seqs, group_of, 31)
    assert nslots >= 16 * union_grid(eng), err
    assert did == FAST, (did, err)


# ---- 3. fewer slots than workgroups, and one slot in all
@pytest.mark.parametrize("mean", [64, 2000], ids=["few_slots", "one_slot"])
def test_fewer_slots_than_workgroups(eng, capfd, skm_env, mean):
    """One genome of 2 kb.  A workgroup with a slot runs it and the read-out behind the loop; every other one runs
    nothing but the end."""
    rng = np.random.default_rng(2001)
    seqs = [util.random_dna_np(rng, 2_000)]
    skm_env.setenv("KHOICE_SKM_MEAN", str(mean))
    nslots, did, err = run_checked(eng, capfd, seqs, [0], 31)
    if mean == 64:
        assert 1 < nslots < union_grid(eng), err
    else:
        assert nslots == 1, err
    assert did == FAST, (did, err)


# ---- 4. multi-subset slots among lean ones
def per_kmer(k):
    return 2.0 / (k - minimizer_len(k) + 2) + 1.0 / 48.0       # the planner's records per k-mer position


def test_multi_subset_slots_among_lean_ones(eng, capfd, skm_env):
    """Three unrelated genomes (nothing merges), k = 32 (the one k at which the planner takes a mean near 4096 as
    asked): slots with N on both sides of the table size in one call, more slots than workgroups.  A multi-subset slot
    keeps its read-outs, leaves nothing behind, and the staging of its successor waits for its last subset."""
    k = 32
    rng = np.random.default_rng(3204)
    seqs = [util.random_dna_np(rng, 720_000) for _ in range(3)]
    mean = min(3950, int((UNION_CAP - 112) / (per_kmer(k) * 1.7)) - 20)
    skm_env.setenv("KHOICE_SKM_MEAN", str(mean))
    nslots, did, err = run_checked(eng, capfd, seqs, [0, 1, 2], k)
    assert nslots == -(-sum(len(s) - k + 1 for s in seqs) // mean) and nslots > union_grid(eng), err
    found = MULTI.findall(err)
    assert len(found) == 1 and 0 < int(found[0]) < nslots, err
    assert did == FAST, (did, err)


# ---- 5. a slot handed to k_skm_big between ordinary slots, for both reasons
@pytest.mark.parametrize("case", ["region", "chunks"])
def test_handed_on_slot_between_ordinary_slots(eng, capfd, skm_env, case):
    """`region`: slot 0 holds more records than its region (listed before anything is merged; it counts as empty).
    `chunks`: its records fit and make more chunks than the union numbers; ten records stand twice in their genome, so
    the merge has counted repeats that are taken back behind barrier 2 — while the read-out of the previous slot adds
    to the same counters."""
    if case == "region":
        seqs, group_of = with_background(deep_case(31), 51)
    else:
        _, _, (s0, group_of) = handover_case(31, 1)
        bg, _ = random_genomes(len(s0), 10_000, 52, related=True)
        seqs = [b + b"N" + s for b, s in zip(bg, s0)]
        skm_env.setenv("KHOICE_SKM_SLACK", "50")           # regions of the union's 1024 records
    grid = union_grid(eng)
    skm_env.setenv("KHOICE_SKM_MEAN", str(mean_for(seqs, 2 * grid)))
    nslots, did, err = run_checked(eng, capfd, seqs, group_of, 31)
    assert nslots >= 2 * grid, err
    assert did["retries"] == 0 and did["skm_union"] == 1 and did["union_tagged"] == 0, (did, err)
    assert did["big_slots"] > 0 and did["skm_big"] == 1, (did, err)


# ---- 6. every wave holds records and chunks
@functools.lru_cache(maxsize=None)
def full_slot_case():
    """k = 17 (minimizers of 12 bases, windows of 6).  920 distinct records xxxx A^12 xxxx (x in CGT): 20 bases, four
    k-mers that all hold A^12, the smallest minimizer there is: one slot with 920 records in two chunks each (1840
    chunks, two passes; 3680 k-mers: a lean slot) and a few dozen of the background's.  Eight genomes in two groups
    over a related background."""
    m = minimizer_len(17)
    assert m == 12
    rng = np.random.default_rng(1706)
    flanks = set()
    while len(flanks) < 920:
        flanks.add(bytes(b"CGT"[i] for i in rng.integers(0, 3, size=8)))
    recs = [[] for _ in range(8)]
    for j, f in enumerate(sorted(flanks)):
        recs[j % 8].append(f[:4] + b"A" * m + f[4:])
    return [b"N".join(r) for r in recs], [g // 4 for g in range(8)]


def test_every_wave_holds_records_and_chunks(eng, capfd, skm_env):
    seqs, group_of = with_background(full_slot_case(), 54)
    grid = union_grid(eng)
    skm_env.setenv("KHOICE_SKM_SLACK", "50")               # regions of the union's 1024 records
    skm_env.setenv("KHOICE_SKM_MEAN", str(mean_for(seqs, grid + grid // 2)))
    nslots, did, err = run_checked(eng, capfd, seqs, group_of, 17)
    d = util.skm_line(err)
    print("fullest slot", d["slot_max"], "records of", d["cap"])
    assert nslots > grid, err
    assert d["cap"] == UNION_CAP and 900 <= d["slot_max"] <= UNION_CAP and d["overfull"] == 0 and d["errors"] == 0, (d, err)
    assert did == FAST, (did, err)


# ---- 7. both mask halves and repeats
def test_both_mask_halves_and_repeats(eng, capfd, skm_env):
    """40 related genomes of 20 kb in two groups of 20 (tags 32 .. 39: the high half of the mask).  Genome 1 is genome 0
    again, in the same group: identical records of one half, bits that are set already.  Genome 35 is genome 3 again:
    the same content in the other half, which must not merge."""
    seqs, _ = random_genomes(40, 20_000, 4007, related=True)
    seqs[1] = seqs[0]
    seqs[35] = seqs[3]
    group_of = [g // 20 for g in range(40)]
    grid = union_grid(eng)
    skm_env.setenv("KHOICE_SKM_MEAN", str(mean_for(seqs, 2 * grid)))
    nslots, did, err = run_checked(eng, capfd, seqs, group_of, 31)
    assert nslots >= 2 * grid, err
    assert did == FAST, (did, err)
