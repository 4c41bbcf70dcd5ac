"""The probe tail of k_skm_union's lean body (khoice_amd/csrc/kh_skm.hip): what happens to the keys that lose probe
round 1 of a pass — further rounds at full width, then one key per lane through the second table and on in the main
one — while the waves that merge the next slot's records run at a raised priority.

Here: losers that share their key across lanes and waves, a crowded table (the second table full, keys on in the main
table), ordinary load, repeats inside a genome among the losers, keys of the high mask half, and a multi-subset slot
(the other body) among lean ones.  Every call twice on one engine against the C restatement (oracle.c_oracle.exp1):
the union alone does the work, without an error bit, and takes the same number of multi-subset slots both times."""
import re

import numpy as np
import pytest

from khoice_amd import synth
from oracle import c_oracle as CO
from tests import util
from tests.test_gpu_skm_hashsets import random_genomes, two_round_case, with_background
from tests.test_gpu_skm_union_chain import eng, skm_env  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

KERNELS = ("skm_union", "skm_big", "union_tagged")
COUNTERS = ("retries",)
MULTI = re.compile(r"\[skm\] k=\d+ .* overfull slots \d+ multi-subset slots (\d+)")
UNION_T = 4096             # entries of the union's main table


def run_checked(eng, capfd, seqs, group_of, k, cs=5000, hist_len=5001):
    """Two calls against the oracle; on both: the union alone did the work, no error bit.  -> multi-subset slots of
    the first."""
    want = CO.exp1(seqs, group_of, k, cs=cs, hist_len=hist_len)
    seen = []
    for _ in range(2):
        capfd.readouterr()
        got, did = util.exp1_run_stats(eng, seqs, group_of, k, cs, hist_len, KERNELS, COUNTERS)
        err = capfd.readouterr().err
        util.exp1_same(got, want)
        assert did == dict(skm_union=1, skm_big=0, union_tagged=0, retries=0), (did, err)
        assert util.skm_line(err)["errors"] == 0, err
        found = MULTI.findall(err)
        assert len(found) == 1, err
        seen.append(int(found[0]))
    print("k", k, "multi-subset slots, both calls:", seen)
    assert seen[0] == seen[1], seen
    return seen[0]


_CACHE = {}


def unrelated():
    """Three unrelated genomes of 60 kbp in two groups: nothing merges, a slot's table fills to what the mean says."""
    if "u" not in _CACHE:
        rng = np.random.default_rng(4242)
        _CACHE["u"] = [util.random_dna_np(rng, 60_000) for _ in range(3)]
    return list(_CACHE["u"]), [0, 0, 1]


@pytest.mark.parametrize("k", [17, 24, 31, 32])
def test_losers_on_a_small_set(eng, capfd, skm_env, k):
    """Related genomes whose records differ here and there: non-identical records share k-mers, so several lanes and
    waves lose round 1 with the same key at once."""
    items = synth.species_set(2, 3, 30_000)
    run_checked(eng, capfd, [t for _, _, t in items], [s - 1 for s, _, _ in items], k)


def test_crowded_table(eng, capfd, skm_env):
    """A mean just below the table's size: most keys of the later passes lose round 1 (waves with more than 64
    losers), the second table is crowded and keys go on in the main table; some slots take two subsets."""
    seqs, group_of = unrelated()
    skm_env.setenv("KHOICE_SKM_MEAN", str(UNION_T - 96))
    run_checked(eng, capfd, seqs, group_of, 31)


def test_ordinary_load(eng, capfd, skm_env):
    seqs, group_of = unrelated()
    run_checked(eng, capfd, seqs, group_of, 31)


def test_repeats_among_losers(eng, capfd, skm_env):
    """A 4 kbp segment pasted twice into one genome: its k-mers meet masks that hold their genome's bit already, many
    of them as losers of round 1 — whichever lane places such a key counts the repeat (distinct_per_seq is instances -
    repeats)."""
    seqs, group_of = unrelated()
    seg = seqs[1][20_000:24_000]
    seqs[1] = seqs[1] + b"N" + seg + b"N" + seg
    run_checked(eng, capfd, seqs, group_of, 31)


def test_high_mask_half(eng, capfd, skm_env):
    """Forty related genomes of 8 kbp in groups of five: tags >= 32 put keys of the high mask half among the losers."""
    seqs, _ = random_genomes(40, 8_000, 77, related=True)
    run_checked(eng, capfd, seqs, [g // 5 for g in range(40)], 31)


def test_lean_next_to_multi(eng, capfd, skm_env):
    """One slot taken in two subsets (the multi body, unchanged) among lean slots of related background: both bodies
    work on the same planes in one walk."""
    skm_env.setenv("KHOICE_SKM_SLACK", "50")       # regions of the union's 1024 records
    skm_env.setenv("KHOICE_SKM_MEAN", "1000")      # little background in the family's slot: its records fit the region
    seqs, group_of = with_background(two_round_case()[2], 53)
    multi = run_checked(eng, capfd, seqs, group_of, 31)
    assert multi >= 1
