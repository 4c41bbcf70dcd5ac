"""k_skm_union (khoice_amd/csrc/kh_skm.hip): the two jobs between a slot's barriers 1 and 2, the merge of identical
records and the previous slot's read-out, at the edges that a rewrite of either for fewer dependent LDS round trips
can break.

The MERGE compares a record with the one it met in one 16-byte read and one branch (the four words XORed, the last
one under SkmRec1's content rule), and a copy adds its genome's bit to the surviving record's mask once, behind the
loop; whether the bit was set already (a repeat inside one genome) is looked at behind the chunk numbering.  The
READ-OUT evaluates the entries a thread created one after the other; a form that takes all of them at once (exchanges
issued together, common group rounds) was measured with these cases and rejected for its time, and the cases stay.

What can go wrong: a compare that overlooks one of the four words, the mask of the last word (the tag's five low bits
are ignored, its sixth and n are not), a repeat that is not counted or counted twice, the counters of a slot handed to
k_skm_big; in the read-out an entry whose group rounds end before its neighbour's, a clamp applied to the wrong entry,
a mask that is not zero when the next slot inserts, a field without an entry that disturbs a live one.
KHOICE_SKM_MEAN makes the slots small enough that every workgroup walks several: what a slot leaves behind shows in
the next.  Every case: against the C restatement bit for bit, a second call that must equal the first, and the fast
form must have answered."""
import functools

import numpy as np
import pytest

from tests import util
from tests.test_gpu_skm2_hashsets import handover_case
from tests.test_gpu_skm_hashsets import deep_case, random_genomes, with_background
from tests.test_gpu_skm_union_chain import mean_for, run_checked, union_grid
from tests.test_gpu_skm_union_overlap import FAST, MULTI, UNION_CAP, per_kmer

pytestmark = pytest.mark.gpu

ALPHA = np.frombuffer(b"ACGT", dtype=np.uint8)


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


def several_slots(eng, skm_env, seqs, per_wg=3):
    grid = union_grid(eng)
    skm_env.setenv("KHOICE_SKM_MEAN", str(mean_for(seqs, per_wg * grid)))
    return per_wg * grid


# ---- 1. the compare, word by word
@functools.lru_cache(maxsize=None)
def one_word_apart():
    """An ancestor of 200 kb and four variants, 1 Mbp in all.  Variants 1 - 3: one substitution every 97 / 101 / 103
    bases from another start each — a record is at most 64 bases, so nearly every changed record differs from the
    ancestor's in one base, i.e. in exactly one of its four 32-bit words, and over two thousand substitutions per
    variant at strides prime to every record length fall into all four.  Variant 4: an N every 89 bases, which cuts the
    run there: records with the ancestor's leading bases and another n (the last word's top bits alone differ).
    Two groups, the ancestor's holds a plain copy: most records do merge."""
    rng = np.random.default_rng(1101)
    anc = rng.integers(0, 4, size=200_000)
    out = [ALPHA[anc].tobytes()]
    for start, stride in ((5, 97), (40, 101), (77, 103)):
        g = anc.copy()
        at = np.arange(start, g.size, stride)
        g[at] = (g[at] + rng.integers(1, 4, size=at.size)) % 4
        out.append(ALPHA[g].tobytes())
    cut = bytearray(out[0])
    cut[60::89] = b"N" * len(cut[60::89])
    out.append(bytes(cut))
    return out, [0, 0, 1, 1, 0]


@pytest.mark.parametrize("k", [17, 31, 32, 16])
def test_records_one_word_apart(eng, capfd, skm_env, k):
    seqs, group_of = one_word_apart()
    if k == 16:
        skm_env.setenv("KHOICE_SKM_MIN_K", "15")          # the instantiation that takes k from the job
    want = several_slots(eng, skm_env, seqs)
    nslots, did, err = run_checked(eng, capfd, seqs, group_of, k)
    assert nslots >= want, err
    assert did == FAST, (did, err)


# ---- 2. both mask halves
def test_copies_in_one_half_and_across_halves(eng, capfd, skm_env):
    """40 related genomes of 20 kb, 36 of them in one group (operands 0 .. 35: both halves of its mask), 4 in another.
    Genome 35 is genome 3 again: the same content in the other half, which must not merge, and both count.  Genome 1
    is genome 0 again and genome 34 is genome 33 again: copies inside the low and inside the high half, which merge."""
    seqs, _ = random_genomes(40, 20_000, 2202, related=True)
    seqs[1] = seqs[0]
    seqs[35] = seqs[3]
    seqs[34] = seqs[33]
    group_of = [0] * 36 + [1] * 4
    want = several_slots(eng, skm_env, seqs, 2)
    nslots, did, err = run_checked(eng, capfd, seqs, group_of, 31)
    assert nslots >= want, err
    assert did == FAST, (did, err)


# ---- 3. repeats inside one genome
@functools.lru_cache(maxsize=None)
def repeats_case():
    """Six related genomes of 40 kb in two groups; every genome holds pieces of about 300 bases twice (one piece every
    4 kb, written again 1500 bases on), genome 4 holds one of them three times.  The second copy's records meet the
    first's in the merge with their genome's bit set already."""
    rng = np.random.default_rng(3303)
    base, _ = random_genomes(6, 40_000, 3304, related=True)
    out = []
    for j, s in enumerate(base):
        g = bytearray(s)
        for at in range(1000 + 137 * j, len(g) - 4000, 4000):
            n = 280 + int(rng.integers(0, 40))
            g[at + 1500:at + 1500 + n] = g[at:at + n]
        if j == 4:
            g[3200:3500] = g[1000 + 137 * 4:1300 + 137 * 4]
        out.append(bytes(g))
    return out, [0, 0, 0, 1, 1, 1]


@pytest.mark.parametrize("k", [31, 21])
def test_pieces_twice_in_one_genome(eng, capfd, skm_env, k):
    seqs, group_of = repeats_case()
    want = several_slots(eng, skm_env, seqs, 2)
    nslots, did, err = run_checked(eng, capfd, seqs, group_of, k)
    assert nslots >= want, err
    assert did == FAST, (did, err)


def test_repeats_counted_then_slot_handed_on(eng, capfd, skm_env):
    """Slot 0's records fit and make one chunk more than the union numbers; ten of them stand twice in their genome.
    The merge has counted those repeats (now behind its loop) when barrier 2 finds the slot too large: the hand-over
    path takes them back by the zero a counting record stored in its own rmask word.  Around it: ordinary slots of a
    background that holds repeats too, so the same counters are added to from the merge and the read-out."""
    _, _, (s0, group_of) = handover_case(31, 1)
    bg, _ = random_genomes(len(s0), 10_000, 3305, related=True)
    seqs = [b + b"N" + b[2000:2300] + b"N" + s for b, s in zip(bg, s0)]
    skm_env.setenv("KHOICE_SKM_SLACK", "50")               # regions of the union's 1024 records
    want = several_slots(eng, skm_env, seqs, 2)
    nslots, did, err = run_checked(eng, capfd, seqs, group_of, 31)
    assert nslots >= want, err
    assert did["retries"] == 0 and did["skm_union"] == 1 and did["union_tagged"] == 0, (did, err)
    assert did["big_slots"] > 0 and did["skm_big"] == 1, (did, err)


# ---- 4. group rounds that differ between the two entries of a thread
@functools.lru_cache(maxsize=None)
def mixed_groups(sizes):
    """One genome per entry of `sizes` summed, groups of those sizes.  Every genome: a block all genomes share (its
    k-mers sit in every group: as many rounds as groups, the across-group bin clamped at cs), a block shared by the
    genomes of groups 0 and 1 (two rounds), a block shared inside its group (one round, the count clamped at cs where
    the group is larger) and private sequence (one round, count 1) — cut into pieces of 1500 bases and interleaved, and
    all four kinds fall into every slot, so the two entries of a thread mostly need different numbers of rounds."""
    rng = np.random.default_rng(4400 + len(sizes))
    ngen = sum(sizes)
    per = min(15_000, 990_000 // ngen) // 4 // 1500 * 1500
    everyone = util.random_dna_np(rng, per)
    pair = util.random_dna_np(rng, per)
    seqs, group_of = [], []
    for g, n in enumerate(sizes):
        own = util.random_dna_np(rng, per)
        for _ in range(n):
            parts = [everyone, pair if g < 2 else util.random_dna_np(rng, per), own, util.random_dna_np(rng, per)]
            seqs.append(b"N".join(p[i:i + 1500] for i in range(0, per, 1500) for p in parts))
            group_of.append(g)
    return seqs, group_of


SIX = {2: (2, 2, 2, 2, 2, 2),                      # 25 bins: four stripes per bin (sshift 2)
       1: (12, 10, 10, 10, 10, 10),                # 75 bins: two stripes (sshift 1)
       0: (2,) * 12 + (1,) * 36}                   # 48 groups, 60 genomes: 157 bins, one stripe (sshift 0)


@pytest.mark.parametrize("cs", [2, 3])
@pytest.mark.parametrize("sshift", [2, 1, 0])
def test_entries_with_different_group_rounds(eng, capfd, skm_env, sshift, cs):
    """Six groups (sshift 0 takes more bins than six groups of at most 64 genomes have: 48 groups there).  cs = 2 and 3:
    the count inside a group and the number of groups both pass the clamp."""
    seqs, group_of = mixed_groups(SIX[sshift])
    nbins = len(seqs) + 2 * (max(group_of) + 1) + 1
    assert (2 if nbins <= 72 else 1 if nbins <= 144 else 0) == sshift
    want = several_slots(eng, skm_env, seqs, 2)
    nslots, did, err = run_checked(eng, capfd, seqs, group_of, 31, cs=cs, hist_len=64)
    assert nslots >= want, err
    assert did == FAST, (did, err)


# ---- 5. every kind of created entry
def test_entries_in_the_second_table(eng, capfd, skm_env):
    """The deep-tier families of test_gpu_skm_hashsets in slot 0, inside the union's region: entries created one key
    per lane, in the second table and in the main one behind it, read out through the same fields."""
    seqs, group_of = with_background(deep_case(31), 5501)
    skm_env.setenv("KHOICE_SKM_SLACK", "50")               # regions of the union's 1024 records
    want = several_slots(eng, skm_env, seqs, 2)
    nslots, did, err = run_checked(eng, capfd, seqs, group_of, 31)
    assert nslots >= want, err
    assert did == FAST, (did, err)


def test_three_passes_and_multi_subset_slots(eng, capfd, skm_env):
    """Three unrelated genomes at k = 32 with a mean near the table size: slots of two and three passes of chunks
    (the fields of passes 1 and 2 are set), multi-subset slots — which read out in place, through the same code —
    between lean ones whose read-out waits for the next slot, and a last slot of every walk that reads out behind
    the loop.  (2.2 Mbp, the size of the overlap test's case: slots of 4096 k-mers, and more of them than workgroups.)"""
    k = 32
    rng = np.random.default_rng(5502)
    seqs = [util.random_dna_np(rng, 720_000) for _ in range(3)]
    mean = min(3950, int((UNION_CAP - 112) / (per_kmer(k) * 1.7)) - 20)
    skm_env.setenv("KHOICE_SKM_MEAN", str(mean))
    nslots, did, err = run_checked(eng, capfd, seqs, [0, 0, 1], k)
    assert nslots == -(-sum(len(s) - k + 1 for s in seqs) // mean) and nslots > union_grid(eng), err
    found = MULTI.findall(err)
    assert len(found) == 1 and 0 < int(found[0]) < nslots, err
    assert did == FAST, (did, err)
