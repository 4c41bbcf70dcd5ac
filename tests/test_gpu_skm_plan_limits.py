"""The super-k-mer plan (skm_plan, khoice_amd/csrc/kh_engine.cpp) at the limits of its geometry, where the LDS layouts
of k_skm_regroup, skm_flush and the unions are fullest, and the side lists (SkmRun::spill_cap records, SkmRun::big_cap
listed slots) at and beyond what they keep.

1. Slot counts at the two partition levels.  KHOICE_SKM_MEAN=64 (the smallest the plan accepts) and texts of exactly
   64 x nslots k-mer positions put nslots where S (slots per coarse bucket) steps from 1 to 2, where it reaches
   MAX_FINE - 1 and MAX_FINE, where the last coarse bucket holds fewer slots than the others (nfine < S) and where the
   fine-slot field of a record is full — with one-word keys (256 x 512 slots, k = 17 and 31) and with two-word keys
   (512 x 1024 slots, k = 33, 41, 63) — and one step beyond: more positions than MAX_COARSE x MAX_FINE slots of 64
   take, where the plan keeps that many slots and cuts the regions' slack instead.
2. The side lists.  Two unrelated texts A and B, each 32 times in a group of its own (device pointers to ONE copy of
   each: read in place, nothing packed).  A text is random bases followed by one random block several times over, so
   every minimizer run of the block arrives 32 x (copies of the block) times in its slot, more than the slot's region
   holds: the block's length sets how many slots overflow, its copies by how many records.  KHOICE_SKM_SLACK=2 and
   about 131 072 slots keep every other slot and every coarse bucket far below its region.  (KHOICE_SKM_SLACK below 1,
   the way of the small overflow tests, cuts the coarse regions by the same factor: measured at 0.01 on 38 M
   positions, every call ended with a capacity error of the scatter and a retry whatever the mean.)  Below the
   capacities k_skm_big (k_skm_cross in its listed launch for experiment type 3) takes thousands of listed slots;
   above one of them SkmRun::settle declines, one retry is counted, the lost attempt's statistics are rolled back and
   the key-array form (the set form) answers.  The expected answer is that of the two-text call in closed form
   (closed_form_exp1, closed_form_exp3), proved on the CPU against the oracles on all 64 operands at a small length.

Every GPU case: kh_exp1_run against oracle.c_oracle.exp1 bit for bit, the call twice with equal results and
statistics, the answering form from the launch counts, the geometry from the [skm] line.

Not covered: the one-word nb1 = 512 branch of skm_plan (more than 256 x 512 slots and a slack cut below 1.4) needs
s2 = (1024 - 112) / (positions x records per k-mer / 131072) < 1.4, at least 279 M positions at k = 17: out of
reach of a test that takes seconds.  The scatter over 512 coarse buckets of one-word records is what
tests/test_gpu_skm_exchange.py runs (test_compact_path_one_word_coarse_boundary, test_plan_near_its_cap).

The unmarked tests restate the geometry, prove the closed forms and check that the case list holds every edge."""
import functools
import os
import re

import numpy as np
import pytest

from oracle import c_oracle as CO
from tests import test_gpu_exp3 as X3          # the oracle of experiment type 3
from tests import util

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "khoice_amd", "csrc")


def constant(fname, name):
    with open(os.path.join(CSRC, fname)) as fh:
        m = re.search(r"\b%s = ([^,;]+)[,;]" % name, fh.read())
    return int(eval(m.group(1).replace("u", ""), {}))      # "256", "1u << 20", "16384u"


MAX_COARSE = {1: constant("kh_launch.h", "KH_SKM_MAX_COARSE"), 2: constant("kh_launch.h", "KH_SKM2_MAX_COARSE")}
MAX_FINE = {1: constant("kh_launch.h", "KH_SKM_MAX_FINE"), 2: constant("kh_launch.h", "KH_SKM2_MAX_FINE")}
SPILL_CAP = constant("kh_engine.cpp", "spill_cap")
BIG_CAP = constant("kh_engine.cpp", "big_cap")
LIM = {w: MAX_COARSE[w] * MAX_FINE[w] for w in (1, 2)}
MEAN = 64                                       # KHOICE_SKM_MEAN of section 1
FAST = dict(skm_union=1, union_tagged=0, retries=0)


def geometry(k, positions, mean=MEAN):
    """skm_plan restated for callers without a table: (nslots, S, nb1, slots of the last coarse bucket).  More slots
    than the two levels number: the slack cut keeps MAX_COARSE x MAX_FINE (its conditions hold far beyond the sizes
    used here; the GPU tests read from the line that it was taken)."""
    w = util.words(k)
    nslots = min(max(1, -(-positions // mean)), LIM[w])
    S = max(1, -(-nslots // MAX_COARSE[w]))
    nb1 = -(-nslots // S)
    return nslots, S, nb1, nslots - (nb1 - 1) * S


# ---------------------------------------------------------------- 1. the cases: (k, nslots, extra positions) -> claims
# name: (k, k-mer positions, {what the [skm] line must show})
def slot_cases():
    cases = {}

    def add(name, k, nslots, positions=None, **claims):
        cases[f"{name}-k{k}"] = (k, MEAN * nslots if positions is None else positions, dict(nslots=nslots, **claims))

    for k in (17, 31):
        add("S1_last", k, 255, S=1, nb1=255)
        add("S1_full", k, 256, S=1, nb1=256)
        add("S2_first", k, 257, S=2, nb1=129)
        add("S511_full", k, 130_816, S=511, nb1=256)
        add("S512_last_257", k, 130_817, S=512, nb1=256)
        add("S512_last_511", k, 131_071, S=512, nb1=256)
        add("S512_full", k, 131_072, S=512, nb1=256)
        add("clipped_by_one_slot", k, 131_072, MEAN * 131_072 + 64, S=512, nb1=256)
    add("clipped_half_again", 17, 131_072, MEAN * 131_072 * 3 // 2 + 37, S=512, nb1=256)
    for k in (33, 41, 63):
        add("S1_last", k, 511, S=1, nb1=511)
        add("S1_full", k, 512, S=1, nb1=512)
        add("S2_first", k, 513, S=2, nb1=257)
    add("S1023_last_512", 41, 523_265, S=1023, nb1=512)
    add("S1024_last_513", 41, 523_777, S=1024, nb1=512)
    add("S1024_full", 41, 524_288, S=1024, nb1=512)
    add("clipped", 41, 524_288, MEAN * 524_288 + 5 * 64 + 1, S=1024, nb1=512)
    return cases


SLOT_CASES = slot_cases()
LARGEST = max(p for _, p, _ in SLOT_CASES.values())


@functools.lru_cache(maxsize=1)
def ancestors():
    """Four related texts of the largest case's size, as code arrays: group 0 = (X, X with 2 % substitutions),
    group 1 = (Y = X with 6 %, Y with 2 %): k-mers shared inside a group and across the groups at every k."""
    rng = np.random.default_rng(6401)
    n = LARGEST // 4 + 128
    x = rng.integers(0, 4, n, dtype=np.uint8)

    def mutated(a, rate):
        g = a.copy()
        hit = np.flatnonzero(rng.random(n) < rate)
        g[hit] = (g[hit] + rng.integers(1, 4, hit.shape[0], dtype=np.uint8)) & 3
        return g
    y = mutated(x, 0.06)
    return [x, mutated(x, 0.02), y, mutated(y, 0.02)]


def genomes(k, positions):
    """2 groups x 2 related genomes (host bytes) with exactly `positions` k-mer positions in all."""
    each, rest = divmod(positions, 4)
    lens = [each + k - 1] * 3 + [each + rest + k - 1]
    alpha = np.frombuffer(b"ACGT", dtype=np.uint8)
    return [alpha[a[:n]].tobytes() for a, n in zip(ancestors(), lens)], [0, 0, 1, 1]


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
    for name in ("KHOICE_SKM_MEAN", "KHOICE_SKM_SLACK", "KHOICE_EXP3_SKM"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("KHOICE_SKM_DEBUG", "1")
    return monkeypatch


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SLOT_CASES))
def test_slot_counts_at_the_partition_limits(eng, capfd, skm_env, name):
    k, positions, claims = SLOT_CASES[name]
    seqs, group_of = genomes(k, positions)
    if positions == MEAN * claims["nslots"]:
        seqs, mean = util.fitted(seqs, k, claims["nslots"])
        assert mean == MEAN
    assert sum(len(s) - k + 1 for s in seqs) == positions
    skm_env.setenv("KHOICE_SKM_MEAN", str(MEAN))
    nslots, did, err = util.run_checked(eng, capfd, seqs, group_of, k)
    line = util.skm_line(err)
    print(name, {f: line[f] for f in ("positions", "nb1", "S", "nslots", "cap", "slot_max", "spilled", "overfull")}, did)
    assert line["positions"] == positions and nslots == line["nslots"], err
    for f, v in claims.items():
        assert line[f] == v, (f, line)
    assert line["nslots"] - (line["nb1"] - 1) * line["S"] == geometry(k, positions)[3], line
    assert line["errors"] == 0, line
    for f, v in FAST.items():
        assert did[f] == v, (f, did, err)
    if positions > MEAN * LIM[util.words(k)]:      # the slack cut: what a region no longer holds goes to k_skm_big
        assert did["big_slots"] == line["overfull"], (did, line)
    else:
        assert did["big_slots"] == 0 and did["skm_big"] == 0 and line["overfull"] == 0, (did, line)


# ---------------------------------------------------------------- 2. the side lists
# (k, side of the capacities) -> (unique bases, bases of the repeated block, its copies): see side_texts
# (31, above) lists more slots than big_cap, (41, above) fewer, with more records beside their regions than spill_cap
SIDE = {(31, "below"): (200_000, 37_000, 6), (31, "above"): (100_000, 130_000, 9),
        (41, "below"): (200_000, 50_000, 6), (41, "above"): (200_000, 50_000, 14)}
SIDE_W = {31: 16, 41: 27}                       # m-mers per k-mer (the [skm] line's w)
SIDE_SLOTS = 131_072                            # slots the mean aims at: every slot far below a region without the block
COPIES = 32
SLACK = "2"
MARGIN = 1.25
SIDE_PAIRS = [(5000, 5001), (7, 20)]            # (cs, hist_len): nothing clamps / cs clamps the 32, the histogram's end too
SIDE_COUNTERS = ("retries", "big_slots", "builds", "bases", "kmers", "distinct", "text_packed")


@functools.lru_cache(maxsize=None)
def side_texts(unique, period, reps, seed=977):
    """Two unrelated texts: `unique` random bases, then a random block of `period` bases `reps` times over.  Every
    minimizer run of the block arrives reps x COPIES times in its slot: `period` sets how many slots overflow, `reps`
    by how many records."""
    rng = np.random.default_rng(seed)
    return tuple(util.random_dna_np(rng, unique) + util.random_dna_np(rng, period) * reps for _ in range(2))


def side_mean(k, texts, copies=COPIES):
    return -(-copies * sum(len(t) - k + 1 for t in texts) // SIDE_SLOTS)


def side_region(k, texts, copies=COPIES):
    """cap2 of skm_plan under KHOICE_SKM_SLACK: records of a slot's region."""
    positions = copies * sum(len(t) - k + 1 for t in texts)
    nslots = -(-positions // side_mean(k, texts, copies))
    recs = positions * (2.0 / (SIDE_W[k] + 1) + 1.0 / 48.0)
    return (int(recs / nslots * float(SLACK)) + 96 + 15) & ~15


def ocsum_bin(genomes_holding, cs, hist_len):
    """Bin of a pivot k-mer (counter 1) met in a -cs{cs} union of `genomes_holding` plain sets: intersect -ocsum."""
    return min(min(1 + min(genomes_holding, cs), cs), hist_len - 1)


def closed_form_exp1(base, copies, cs, hist_len):
    """kh_exp1_run of (A x copies | B x copies) from base = the answer for (A | B) at the same cs and hist_len: every
    distinct k-mer of a text is in all `copies` genomes of its group; the groups hold what the two texts hold."""
    want = {"within_hist": np.zeros_like(base["within_hist"]), "across_hist": base["across_hist"].copy(),
            "distinct_per_seq": np.repeat(base["distinct_per_seq"], copies)}
    for g in range(2):
        assert base["within_hist"][g].sum() == base["within_hist"][g][1] == base["distinct_per_seq"][g]
        want["within_hist"][g][min(min(copies, cs), hist_len - 1)] = base["distinct_per_seq"][g]
    return want


def closed_form_exp3(base, copies, cs, hist_len):
    """kh_exp3_run of (A x copies | B x copies) with the pivots A and B from the same exp-1 base: a pivot meets all its
    k-mers in its own text's group and the k-mers both texts hold (across_hist[2]) in the other, in `copies` genomes."""
    d, both = base["distinct_per_seq"], base["across_hist"][min(2, hist_len - 1)]
    want = {"inter_hist": np.zeros((2, 2, hist_len), dtype=np.uint64),
            "distinct_per_seq": np.repeat(d, copies), "distinct_per_pivot": d.copy()}
    for p in range(2):
        for g in range(2):
            want["inter_hist"][p, g, ocsum_bin(copies, cs, hist_len)] = d[p] if p == g else both
    return want


@functools.lru_cache(maxsize=None)
def side_base(k, key, cs, hist_len):
    return CO.exp1(list(side_texts(*SIDE[key])), [0, 1], k, cs=cs, hist_len=hist_len)


class DeviceTexts:
    """A and B once each in device memory, at 16-byte aligned addresses: (pointer, length) tuples read in place."""

    def __init__(self, texts):
        import torch
        self.keep = [torch.from_numpy(np.frombuffer(t, dtype=np.uint8).copy()).to("cuda:0") for t in texts]
        torch.cuda.synchronize()
        assert all(t.data_ptr() % 16 == 0 for t in self.keep)
        self.a, self.b = ((t.data_ptr(), len(x)) for t, x in zip(self.keep, texts))

    def operands(self, copies):
        return [self.a] * copies + [self.b] * copies, [0] * copies + [1] * copies


def side_run(eng, capfd, seqs, group_of, k, cs, hist_len):
    capfd.readouterr()
    got, did = util.exp1_run_stats(eng, seqs, group_of, k, cs, hist_len, util.UNION_KERNELS, SIDE_COUNTERS)
    return got, did, capfd.readouterr().err


def side_env(skm_env, k, texts):
    skm_env.setenv("KHOICE_SKM_MEAN", str(side_mean(k, texts)))
    skm_env.setenv("KHOICE_SKM_SLACK", SLACK)


def side_case(eng, capfd, skm_env, key):
    """The 64-operand call at every pair of SIDE_PAIRS, twice each, against the closed form -> [(line, did)]."""
    k, texts = key[0], side_texts(*SIDE[key])
    length = len(texts[0])
    dev = DeviceTexts(texts)
    seqs, group_of = dev.operands(COPIES)
    side_env(skm_env, k, texts)
    out = []
    for cs, hist_len in SIDE_PAIRS:
        base = side_base(k, key, cs, hist_len)
        want = closed_form_exp1(base, COPIES, cs, hist_len)
        got, did, err = side_run(eng, capfd, seqs, group_of, k, cs, hist_len)
        line = util.skm_line(err)
        assert line["w"] == SIDE_W[k] and line["cap"] == side_region(k, texts), line
        print(key, (cs, hist_len), {f: line[f] for f in ("nb1", "S", "nslots", "coarse_max", "cap1", "cap", "slot_max", "errors", "spilled", "overfull")}, did)
        util.exp1_same(got, want)
        again, did2, _ = side_run(eng, capfd, seqs, group_of, k, cs, hist_len)
        util.exp1_same(again, want)
        assert did2 == did, (did, did2)
        # the statistics move by the oracle's totals once, whichever form answered; texts read in place
        assert did["builds"] == 2 * COPIES and did["bases"] == 2 * COPIES * length and did["text_packed"] == 0, did
        assert did["kmers"] == 2 * COPIES * (length - k + 1), did
        assert did["distinct"] == COPIES * int(base["distinct_per_seq"].sum()), did
        assert line["errors"] == 0 and line["coarse_max"] <= line["cap1"], line      # nothing but the side lists declines
        out.append((line, did))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 41])
def test_side_lists_below_their_capacities(eng, capfd, skm_env, k):
    for line, did in side_case(eng, capfd, skm_env, (k, "below")):
        assert 0.25 * BIG_CAP <= line["overfull"] <= 0.9 * BIG_CAP and line["spilled"] <= SPILL_CAP, line
        assert line["slot_max"] > line["cap"], line
        assert did["retries"] == 0 and did["skm_union"] == 1 and did["union_tagged"] == 0, did
        assert did["skm_big"] == 1 and did["big_slots"] == line["overfull"], (did, line)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 41])
def test_side_lists_above_a_capacity(eng, capfd, skm_env, k):
    for line, did in side_case(eng, capfd, skm_env, (k, "above")):
        assert line["overfull"] >= MARGIN * BIG_CAP or line["spilled"] >= MARGIN * SPILL_CAP, line     # (a condition on the input)
        assert did["retries"] == 1 and did["skm_union"] == 1 and did["skm_big"] == 0 and did["big_slots"] == 0, did
        assert did["union_tagged"] >= 1, did                                                          # the key arrays answered
    # an ordinary call on the same engine: the fast form, nothing left behind by the declined attempts
    skm_env.delenv("KHOICE_SKM_MEAN")
    skm_env.delenv("KHOICE_SKM_SLACK")
    seqs, group_of = genomes(k, 4 * 30_000)
    _, did, err = util.run_checked(eng, capfd, seqs, group_of, k)
    assert util.skm_line(err)["errors"] == 0 and did["big_slots"] == 0, (did, err)
    for f, v in FAST.items():
        assert did[f] == v, (f, did, err)


X3_KERNELS = ("skm_cross", "skm_union", "skm_big", "union_tagged", "setop")
X3_COUNTERS = ("retries", "big_slots", "builds", "bases", "text_packed")


@pytest.mark.gpu
@pytest.mark.parametrize("above", [False, True], ids=["below", "above"])
def test_exp3_side_lists(eng, capfd, skm_env, above):
    """kh_exp3_run (KHOICE_EXP3_SKM=1) on the same records: A x 31 | B x 31 and the pivots A and B are the 64 texts of
    the exp-1 case with other tags, so the exp-1 call's [skm] line (kh_exp3_run prints none) tells how full the side
    lists get."""
    k = 31
    key = (k, "above" if above else "below")
    texts = side_texts(*SIDE[key])
    length = len(texts[0])
    dev = DeviceTexts(texts)
    side_env(skm_env, k, texts)
    seqs, group_of = dev.operands(COPIES)
    _, _, err = side_run(eng, capfd, seqs, group_of, k, 5000, 5001)
    line = util.skm_line(err)
    if above:
        assert line["overfull"] >= MARGIN * BIG_CAP or line["spilled"] >= MARGIN * SPILL_CAP, line
    else:
        assert 0.25 * BIG_CAP <= line["overfull"] <= 0.9 * BIG_CAP and line["spilled"] <= SPILL_CAP, line
    skm_env.setenv("KHOICE_EXP3_SKM", "1")
    seqs, group_of = dev.operands(COPIES - 1)
    pivots = [dev.a, dev.b]
    for cs, hist_len in SIDE_PAIRS:
        want = closed_form_exp3(side_base(k, key, cs, hist_len), COPIES - 1, cs, hist_len)
        runs = []
        for _ in range(2):
            eng.profile(True)
            st0 = eng.stats()
            got = eng.exp3_run(seqs, group_of, pivots, k, cs=cs, hist_len=hist_len)
            st1 = eng.stats()
            eng.profile(False)
            did = {n: st1["kernels"][n]["launches"] - st0["kernels"][n]["launches"] for n in X3_KERNELS}
            did.update({n: st1[n] - st0[n] for n in X3_COUNTERS})
            for f in X3.FIELDS:
                assert got[f].shape == want[f].shape and (got[f] == want[f]).all(), (f, cs, hist_len, did)
            runs.append(did)
        did = runs[0]
        print("exp3", above, (cs, hist_len), did, {f: line[f] for f in ("nslots", "cap", "spilled", "overfull")})
        assert runs[1] == did, runs
        assert did["builds"] == 2 * COPIES and did["bases"] == 2 * COPIES * length and did["text_packed"] == 0, did
        assert did["skm_union"] == 0 and did["skm_big"] == 0 and did["union_tagged"] == 0, did
        if above:       # the direct launch lists, settle declines, the set form answers
            assert did["retries"] == 1 and did["skm_cross"] == 1 and did["big_slots"] == 0 and did["setop"] > 0, did
        else:           # the listed launch of k_skm_cross takes every overfull slot
            assert did["retries"] == 0 and did["skm_cross"] == 2 and did["setop"] == 0, did
            assert did["big_slots"] == line["overfull"], (did, line)


# ---------------------------------------------------------------- 3. on the CPU
def test_constants_read_from_the_sources():
    assert MAX_COARSE == {1: 256, 2: 512} and MAX_FINE == {1: 512, 2: 1024}
    assert SPILL_CAP == 1 << 20 and BIG_CAP == 16384
    with open(os.path.join(CSRC, "kh_skm_rec.h")) as fh:
        fine_bits = [int(b) for b in re.findall(r"using SkmRec\d = SkmRecFmt<\d, \d+, (\d+)>", fh.read())]
    assert [1 << b for b in fine_bits] == [MAX_FINE[1], MAX_FINE[2]]     # a full fine field at S = MAX_FINE


@pytest.mark.parametrize("name", list(SLOT_CASES))
def test_claimed_geometry(name):
    k, positions, claims = SLOT_CASES[name]
    nslots, S, nb1, _ = geometry(k, positions)
    assert (nslots, S, nb1) == (claims["nslots"], claims["S"], claims["nb1"])
    lens = [positions // 4 + k - 1] * 3 + [positions // 4 + positions % 4 + k - 1]
    assert sum(n - k + 1 for n in lens) == positions and max(lens) <= LARGEST // 4 + 128


def test_case_list_holds_every_edge():
    """(S, slots of the last bucket) of every edge the module is there for, at both key widths."""
    seen = {w: set() for w in (1, 2)}
    clipped = {w: 0 for w in (1, 2)}
    for k, positions, _ in SLOT_CASES.values():
        w = util.words(k)
        nslots, S, nb1, last = geometry(k, positions)
        seen[w].add((S, last))
        clipped[w] += positions > MEAN * LIM[w]
        assert nslots <= LIM[w] and nb1 <= MAX_COARSE[w] and S <= MAX_FINE[w] and 1 <= last <= S
    for w in (1, 2):
        F = MAX_FINE[w]
        must = {(1, 1), (2, 1), (F, F // 2 + 1), (F, F)}        # S = 1 -> 2; MAX_FINE with a partial last bucket, and full
        assert must <= seen[w], (w, must - seen[w])
        assert clipped[w] >= 1
    assert {(511, 511), (512, 511)} <= seen[1] and (1023, 512) in seen[2]      # MAX_FINE - 1; a last bucket one slot short
    assert {k for k, _, _ in SLOT_CASES.values()} == {17, 31, 33, 41, 63}
    assert geometry(17, MEAN * 255)[1:3] == (1, 255) and geometry(17, MEAN * 257)[1:3] == (2, 129)
    assert set(SIDE) == {(k, side) for k in (31, 41) for side in ("below", "above")} and 2 * COPIES == 64
    for (k, _), (unique, period, reps) in SIDE.items():     # a slot with one run of the block overflows its region
        assert COPIES * reps > side_region(k, side_texts(unique, period, reps)), (k, reps)


@pytest.mark.parametrize("k", [31, 41])
@pytest.mark.parametrize("cs,hist_len", [(5000, 5001), (5000, 20), (7, 5001), (7, 20), (40, 33)])
def test_closed_form_exp1(k, cs, hist_len):
    a, b = side_texts(2_000, 250, 4, seed=5)
    b = b[:1500] + a[1000:2500]                      # the texts share k-mers: across_hist[2] > 0
    base = CO.exp1([a, b], [0, 1], k, cs=cs, hist_len=hist_len)
    assert base["across_hist"][min(2, hist_len - 1)] > 0
    full = CO.exp1([a] * COPIES + [b] * COPIES, [0] * COPIES + [1] * COPIES, k, cs=cs, hist_len=hist_len)
    util.exp1_same(closed_form_exp1(base, COPIES, cs, hist_len), full)


@pytest.mark.parametrize("cs,hist_len", [(5000, 5001), (7, 20), (40, 33), (5000, 20)])
def test_closed_form_exp3(cs, hist_len):
    k, n = 31, COPIES - 1
    a, b = side_texts(400, 100, 2, seed=6)
    b = b[:300] + a[200:500]
    base = CO.exp1([a, b], [0, 1], k, cs=cs, hist_len=hist_len)
    assert base["across_hist"][2] > 0
    full = X3.oracle([a] * n + [b] * n, [0] * n + [1] * n, [a, b], k, cs, hist_len)
    want = closed_form_exp3(base, n, cs, hist_len)
    for f in X3.FIELDS:
        assert want[f].shape == full[f].shape and (want[f] == full[f]).all(), f
