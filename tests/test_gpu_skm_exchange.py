"""The records exchange of steps 7-8 (khoice_amd/dist.py: across_records_exchange) rank by rank on one GPU:
kh_skm_exchange_plan, kh_skm_pack (k_skm_pack, k_skm_pack_compact) and kh_skm_phased_histogram (k_skm_phased).

Pack is a pure function of one rank's genomes and the agreed geometry, the phased union one of the pieces, so one
process plays every rank: it packs each rank into buffers laid out as dist.py lays them out, hands every owner the
pieces the all-to-all would deliver — only the prefix [:part_n[j]] of a foreign part travels, copied into a fresh
tensor, while the rest of the source part holds a poison pattern — and sums the owners' histograms.  The sum must be
the C oracle's across-group histogram over all ranks' genomes (a rank's groups are its own: global group = the rank's
group offset + the local tag).

Every pack output is also checked on the host against the contract the stand-in of tests/test_dist_gloo.py assumes:
the per-slot ranges tile each part's prefix exactly, masks and record fields are in range, identical records are
merged, and the records decode (base j at bits 2j, tag at 117-122, n at 123-127 — the decoding of
insert_chunk in k_skm_phased) to exactly the oracle's distinct (k-mer, local group) pairs, each k-mer in one global
slot on every rank."""
import numpy as np
import pytest
import torch

from khoice_amd import synth
from khoice_amd.engine import KhoiceError
from oracle import c_oracle as CO

pytestmark = pytest.mark.gpu

KH_E_ARG, KH_E_CAPACITY = -1, -6
POISON_REC = -0x0123456789ABCDEF      # as a record: n = 31 and every tag bit set
POISON_MASK = -1
POISON_TABLE = 0x7F7F7F7F
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def eng():
    from khoice_amd import build as kbuild
    from khoice_amd import engine as E
    kbuild.build_library()
    torch.cuda.init()
    e = E.Engine(0)
    yield e
    e.close()


# ---------------------------------------------------------------------------------------------------- inputs
def species_rank(first_species, groups, genomes, length):
    """One rank: `groups` species from first_species on, `genomes` genomes of each, tag = local group."""
    seqs, tags = [], []
    for g in range(groups):
        anc = synth.ancestor(first_species + g, length)
        for j in range(genomes):
            seqs.append(synth.clean_text(synth.genome_records(first_species + g, j, length, anc)))
            tags.append(g)
    return seqs, tags


def positions(seqs, k):
    return sum(max(0, len(s) - k + 1) for s in seqs)


# ---------------------------------------------------------------------------------------------------- decoding
def _revpairs(x):
    """Reverse the 32 two-bit groups of uint64 x."""
    x = ((x >> np.uint64(2)) & np.uint64(0x3333333333333333)) | ((x & np.uint64(0x3333333333333333)) << np.uint64(2))
    x = ((x >> np.uint64(4)) & np.uint64(0x0F0F0F0F0F0F0F0F)) | ((x & np.uint64(0x0F0F0F0F0F0F0F0F)) << np.uint64(4))
    return x.byteswap()


def decode(rec, k):
    """rec int64[n, 2] -> (canonical k-mer codes uint64[m], the index of the record each came from int64[m])."""
    lo, hi = rec[:, 0].view(np.uint64), rec[:, 1].view(np.uint64)
    n = (hi >> np.uint64(59)).astype(np.int64)
    mask = np.uint64((1 << (2 * k)) - 1)
    codes, owner = [], []
    for j in range(int(n.max()) if n.size else 0):
        sel = np.nonzero(n > j)[0]
        l, h = lo[sel], hi[sel]
        x = (l >> np.uint64(2 * j)) | (h << np.uint64(64 - 2 * j)) if j else l
        x &= mask
        fw = _revpairs(x) >> np.uint64(64 - 2 * k)
        rc = ~x & mask
        codes.append(np.minimum(fw, rc))
        owner.append(sel)
    if not codes:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.int64)
    return np.concatenate(codes), np.concatenate(owner)


def test_decode_follows_insert_chunk():
    """The host decoder on a hand-built record: bases j at bits 2j, k-mer j canonical = min(forward, reverse
    complement) with the first base most significant."""
    k, seq = 17, "ACGTTGCAAGGCTTACGATCCA"          # 22 bases: n = 6 k-mers
    v = 0
    for j, b in enumerate(seq):
        v |= "ACGT".index(b) << (2 * j)
    v |= (len(seq) - k + 1) << 123 | 5 << 117
    rec = np.array([[v & M64, v >> 64]], dtype=np.uint64).view(np.int64)
    got, owner = decode(rec, k)
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    want = []
    for j in range(len(seq) - k + 1):
        km = seq[j:j + k]
        rc = "".join(comp[c] for c in reversed(km))
        want.append(min(int("".join("0123"["ACGT".index(c)] for c in s), 4) for s in (km, rc)))
    assert sorted(got.tolist()) == sorted(want) and (owner == 0).all()


# ---------------------------------------------------------------------------------------------------- one simulated job
class Job:
    """R ranks packed on device 0 with the geometry they agreed on (dist.across_records_exchange).  feed[r]: the form in
    which rank r's texts are handed to the pack ((device pointer, length) pairs; default: the host bytes of `ranks`)."""

    def __init__(self, eng, ranks, k, positions_max=None, fan_max=None, feed=None):
        self.eng, self.ranks, self.k, self.R = eng, ranks, k, len(ranks)
        pmax = max(positions(s, k) for s, _ in ranks)
        self.positions_max = max(pmax, positions_max or 0)
        self.fan_max = fan_max or max([int(np.bincount(t).max()) for _, t in ranks if len(t)] + [1])
        self.nslots, self.spp, self.cap = eng.skm_exchange_plan(k, self.positions_max, self.fan_max, self.R)
        R, cap, spp, dev = self.R, self.cap, self.spp, torch.device("cuda", 0)
        self.rec, self.msk, self.cnt, self.off, self.part_n = [], [], [], [], []
        for r, (seqs, tags) in enumerate(ranks):
            rec = torch.full((R, cap, 2), POISON_REC, dtype=torch.int64, device=dev)
            msk = torch.full((R, cap), POISON_MASK, dtype=torch.int32, device=dev)
            cnt = torch.full((R, spp), POISON_TABLE, dtype=torch.int32, device=dev)
            off = torch.full((R, spp), POISON_TABLE, dtype=torch.int32, device=dev)
            torch.cuda.synchronize(dev)
            pn = eng.skm_pack(feed[r] if feed else seqs, tags, k, self.nslots, R, cap, rec.data_ptr(), msk.data_ptr(),
                              cnt.data_ptr(), off.data_ptr())
            self.rec.append(rec), self.msk.append(msk), self.cnt.append(cnt), self.off.append(off)
            self.part_n.append([int(x) for x in pn])

    def pieces(self, owner, sources=None):
        """What owner j holds after the all-to-all: its own part in place, of every other source a fresh contiguous copy
        of exactly the part's used prefix and of its per-slot tables."""
        out, keep = [], []
        for r in (range(self.R) if sources is None else sources):
            if r == owner:
                t = (self.rec[r][owner], self.msk[r][owner], self.cnt[r][owner], self.off[r][owner])
            else:
                n = self.part_n[r][owner]
                rec = torch.full((n + 64, 2), POISON_REC, dtype=torch.int64, device=self.rec[r].device)
                msk = torch.full((n + 64,), POISON_MASK, dtype=torch.int32, device=self.rec[r].device)
                rec[:n] = self.rec[r][owner, :n]
                msk[:n] = self.msk[r][owner, :n]
                t = (rec, msk, self.cnt[r][owner].clone(), self.off[r][owner].clone())
            keep.append(t)
            out.append(tuple(x.data_ptr() for x in t))
        torch.cuda.synchronize()
        return out, keep

    def owner_hist(self, owner, cs=5000, hist_len=5001, sources=None):
        pcs, keep = self.pieces(owner, sources)
        h = self.eng.skm_phased_histogram(self.k, pcs, self.spp, cs, hist_len)
        del keep
        return h

    def hist(self, cs=5000, hist_len=5001, sources_of=None):
        return sum(self.owner_hist(j, cs, hist_len, sources_of(j) if sources_of else None) for j in range(self.R))

    def oracle_hist(self, cs=5000, hist_len=5001, sources=None):
        """The C oracle over the ranks listed in `sources` (a rank listed twice: its groups twice, as new groups)."""
        seqs, groups, first = [], [], 0
        for r in (range(self.R) if sources is None else sources):
            s, t = self.ranks[r]
            seqs += s
            groups += [first + g for g in t]
            first += (max(t) + 1) if len(t) else 0
        if not seqs:
            return np.zeros(hist_len, dtype=np.uint64)
        return CO.exp1(seqs, groups, self.k, cs=cs, hist_len=hist_len, nthreads=16)["across_hist"]

    # ------------------------------------------------------------------------------------------- the pack contract
    def check_structure(self):
        k, R, spp, nslots = self.k, self.R, self.spp, self.nslots
        nmax = min(31, 55 - k)
        slot_of_kmer = []
        for r, (seqs, tags) in enumerate(self.ranks):
            ntags = (max(tags) + 1) if len(tags) else 0
            cnt = self.cnt[r].cpu().numpy().astype(np.int64)
            off = self.off[r].cpu().numpy().astype(np.int64)
            tail = nslots - (R - 1) * spp          # slots of the last part
            assert (cnt[R - 1, tail:] == 0).all() and (off[R - 1, tail:] == 0).all(), "entries past nslots"
            recs, masks, gslots = [], [], []
            for p in range(R):
                n = self.part_n[r][p]
                assert n == int(cnt[p].sum()) and n <= self.cap, (r, p, n, int(cnt[p].sum()), self.cap)
                used = np.nonzero(cnt[p] > 0)[0]
                order = used[np.argsort(off[p, used], kind="stable")]
                ends = off[p, order] + cnt[p, order]
                # [off, off + cnt) of the used slots tile [0, part_n) exactly: no gap, no overlap
                assert (off[p, order][1:] == ends[:-1]).all() and (n == 0 or (off[p, order[0]] == 0 and ends[-1] == n)), \
                    (r, p, "slot ranges do not tile the part")
                rec = self.rec[r][p, :n].cpu().numpy()
                msk = self.msk[r][p, :n].cpu().numpy().view(np.uint32)
                gs = np.empty(n, dtype=np.int64)
                for s in used:
                    gs[off[p, s]:off[p, s] + cnt[p, s]] = p * spp + s
                recs.append(rec), masks.append(msk), gslots.append(gs)
            rec, msk, gs = np.concatenate(recs), np.concatenate(masks), np.concatenate(gslots)
            hi = rec[:, 1].view(np.uint64)
            nf = (hi >> np.uint64(59)).astype(np.int64)
            tag = ((hi >> np.uint64(53)) & np.uint64(63)).astype(np.int64)
            assert ((nf >= 1) & (nf <= nmax)).all(), (r, "record length field")
            assert (tag < ntags).all(), (r, "tag field")
            assert (msk != 0).all() and (msk.astype(np.uint64) >> np.uint64(ntags) == 0).all(), (r, "mask bits")
            assert ((msk >> tag.astype(np.uint32)) & 1 == 1).all(), (r, "mask without the record's own tag")
            # merge contract: one record per content and slot, whatever its tag
            body = hi & ~np.uint64(63 << 53)
            order = np.lexsort((rec[:, 0].view(np.uint64), body, gs))
            same = (gs[order][1:] == gs[order][:-1]) & (body[order][1:] == body[order][:-1]) & \
                   (rec[order, 0][1:] == rec[order, 0][:-1])
            assert not same.any(), (r, "identical records left unmerged")
            # the (k-mer, tag) pairs the masks expand to = the oracle's distinct (k-mer, local group) pairs
            km, at = decode(rec, k)
            for t in range(ntags):
                sel = ((msk[at] >> np.uint32(t)) & 1) == 1
                want = np.unique(np.concatenate([CO.count(s, k).arrays()[0][:, 0]
                                                 for s, g in zip(seqs, tags) if g == t] + [np.zeros(0, np.uint64)]))
                got = np.unique(km[sel])
                assert got.size == want.size and (got == want).all(), (r, t, got.size, want.size)
            if ntags == 0:
                assert km.size == 0
            slot_of_kmer.append((km, gs[at]))
        # across ranks: every canonical k-mer lies in one global slot
        km = np.concatenate([a for a, _ in slot_of_kmer] + [np.zeros(0, np.uint64)])
        gs = np.concatenate([b for _, b in slot_of_kmer] + [np.zeros(0, np.int64)])
        order = np.lexsort((gs, km))
        same = km[order][1:] == km[order][:-1]
        assert (gs[order][1:][same] == gs[order][:-1][same]).all(), "a k-mer filed under two slots"


def run(eng, ranks, k, check=True, **kw):
    job = Job(eng, ranks, k, **kw)
    if check:
        job.check_structure()
    got, want = job.hist(), job.oracle_hist()
    assert (got == want).all(), (k, job.R, np.nonzero(got != want)[0][:8])
    return job, got


# ---------------------------------------------------------------------------------------------------- the matrix
@pytest.mark.parametrize("R", [1, 2, 3, 8])
@pytest.mark.parametrize("k", [17, 18, 20, 21, 24, 25, 27, 31, 32])
def test_exchange_matches_oracle(eng, k, R):
    """Every minimizer length (12 for k = 17..24, 13 for 25..27, 15 / 16 above) and both window families, on 1, 2, 3
    and 8 ranks of different species (the shared rRNA-like block makes k-mers of several groups)."""
    ranks = [species_rank(1 + 3 * r, 2 + r % 2, 2, 12_000) for r in range(R)]
    job, got = run(eng, ranks, k)
    assert got[2:].sum() > 0
    if R == 1:
        seqs, tags = ranks[0]
        assert (eng.exp1_run(seqs, tags, k)["across_hist"] == got).all()


@pytest.mark.parametrize("k", [31, 21])
def test_compact_path_realistic(eng, k):
    """Two ranks of 11 Mbp: slots_per_part >= 2048, so every pack runs k_skm_pack through 64 sub-range cursors and
    k_skm_pack_compact moves the parts together; the parts are full, not a few records in a large geometry."""
    ranks = [species_rank(1 + 2 * r, 2, 5, 1_100_000) for r in range(2)]
    job, _ = run(eng, ranks, k)
    assert job.spp >= 2048, job.spp
    assert min(job.part_n[r][p] for r in range(2) for p in range(2)) > 100_000


def _positions_for(eng, k, R, want_nslots):
    """A positions_max whose plan gives about want_nslots slots (the plan's mean is found from one call)."""
    probe = 100_000_000
    ns, _, _ = eng.skm_exchange_plan(k, probe, 2, R)
    return int(probe / (ns - 1) * (want_nslots - 1))


@pytest.mark.parametrize("side", [-1, 1])
def test_compact_path_one_word_coarse_boundary(eng, side):
    """Small ranks under a large agreed positions_max: one plan a little below 256 x 512 slots (256 coarse buckets) and
    one a little above (512 coarse buckets), both through the compaction."""
    k, R, lim = 31, 2, 256 * 512
    pmax = _positions_for(eng, k, R, lim + side * 600)
    ranks = [species_rank(1 + 2 * r, 2, 2, 10_000) for r in range(R)]
    job, _ = run(eng, ranks, k, positions_max=pmax)
    assert (job.nslots <= lim) if side < 0 else (job.nslots > lim), job.nslots
    assert job.spp >= 2048


@pytest.mark.parametrize("frac", [1.0, 1.55, 1.7])
def test_plan_near_its_cap(eng, frac):
    """Around the largest positions_max the plan takes: from about 512 x 512 slots of the default mean on (frac = 1) the
    slot count stays at 512 x 512 and the slots grow until a region would pass 1024 records (between 1.55 and 1.7 at
    k = 31).  The plan either gives a geometry whose pack and union match the oracle, or refuses with KH_E_CAPACITY —
    never a wrong histogram."""
    k, R, lim = 31, 2, 512 * 512
    pmax = int(_positions_for(eng, k, R, lim) * frac)
    ranks = [species_rank(1 + 2 * r, 1, 2, 8_000) for r in range(R)]
    try:
        job, _ = run(eng, ranks, k, positions_max=pmax)
    except KhoiceError as e:
        assert e.code == KH_E_CAPACITY, e
        return
    assert job.nslots <= lim and job.spp >= 2048


@pytest.mark.parametrize("R", [1, 3, 8])
def test_pack_widths(eng, R):
    """k_skm_pack<NT> for NT = 256 / 512 / 1024, chosen by the slot region's capacity cap2 (KHOICE_SKM_DEBUG=1 prints it):
    at k = 31 with ranks of three groups of two 40 kbp genomes, one rank gives cap2 = 944 (NT = 1024), three ranks
    cap2 = 480 (NT = 512), eight ranks cap2 = 240 (NT = 256): the more ranks, the fewer positions per slot."""
    ranks = [species_rank(1 + 3 * r, 3, 2, 40_000) for r in range(R)]
    run(eng, ranks, 31)


def test_uneven_ranks(eng):
    """32 groups on one rank (tag 31 = mask bit 31), one group on another, a rank whose sequences are all shorter than
    k, one of only N, and one without sequences (nseq = 0): the last three send empty parts, and a piece of the empty
    rank leaves its owner's histogram as it is."""
    k = 27
    many = species_rank(1, 32, 1, 6_000)
    one = species_rank(40, 1, 3, 20_000)
    short = ([b"ACGTACGTAC", b"ACG", b"GATTACA\nGATTACA"], [0, 0, 1])
    all_n = ([b"N" * 5000, b"NNNN\nNNNN" * 100], [0, 0])
    empty = ([], [])
    job, _ = run(eng, [many, one, short, all_n, empty], k)
    assert all(sum(job.part_n[r]) == 0 for r in (2, 3, 4))
    assert all((job.cnt[r] == 0).all() and (job.off[r] == 0).all() for r in (2, 3, 4))
    for j in range(job.R):
        assert (job.owner_hist(j) == job.owner_hist(j, sources=[0, 1])).all()


def test_empty_rank_pack_direct(eng):
    """kh_skm_pack with nseq = 0: success, zero part_n and per-slot tables, no record written."""
    k, R = 31, 3
    nslots, spp, cap = eng.skm_exchange_plan(k, 50_000, 2, R)
    rec = torch.full((R, cap, 2), POISON_REC, dtype=torch.int64, device="cuda")
    msk = torch.full((R, cap), POISON_MASK, dtype=torch.int32, device="cuda")
    cnt = torch.full((R, spp), POISON_TABLE, dtype=torch.int32, device="cuda")
    off = torch.full((R, spp), POISON_TABLE, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    pn = eng.skm_pack([], [], k, nslots, R, cap, rec.data_ptr(), msk.data_ptr(), cnt.data_ptr(), off.data_ptr())
    assert (pn == 0).all() and (cnt == 0).all() and (off == 0).all()
    assert (rec == POISON_REC).all() and (msk == POISON_MASK).all()


def test_identical_genomes_on_every_rank(eng):
    """Every rank holds the same genomes, so every k-mer occurs in every phase of the union, with a group of 32 genomes
    on 8 ranks: the largest clump of copies a slot's region has to take (ADVICE low: regions sized from the table's
    mean, not from the exchange's positions per slot)."""
    k = 31
    big = species_rank(7, 1, 32, 20_000)
    small = species_rank(8, 1, 3, 20_000)
    rank = (big[0] + small[0], big[1] + [1] * len(small[1]))
    job, got = run(eng, [rank] * 8, k)
    assert got[8:].sum() > 0


# ---------------------------------------------------------------------------------------------------- the phased union
@pytest.fixture(scope="module")
def shared_job(eng):
    """Three ranks that share one species (counts up to 3 x its genomes' groups) besides their own."""
    ranks = []
    for r in range(3):
        s1, t1 = species_rank(50, 1, 2, 30_000)
        s2, t2 = species_rank(51 + r, 2, 2, 30_000)
        ranks.append((s1 + s2, t1 + [t + 1 for t in t2]))
    job = Job(eng, ranks, 31)
    job.check_structure()
    return job


@pytest.mark.parametrize("cs", [1, 2, 5000])
@pytest.mark.parametrize("hist_len", [2, 3, 64, 5001])
def test_phased_saturation_and_short_histograms(shared_job, cs, hist_len):
    """Counters saturate at cs, bins at hist_len - 1 (counts reach 3 here, above hist_len - 1 for 2 and 3 bins)."""
    want = shared_job.oracle_hist(cs, hist_len)
    assert (shared_job.hist(cs, hist_len) == want).all()
    if cs == 5000 and hist_len == 5001:
        assert want[3:].sum() > 0


def test_phased_piece_order(shared_job):
    """The same pieces in another order give the same histogram."""
    want = shared_job.hist()
    assert (shared_job.hist(sources_of=lambda j: [2, 0, 1]) == want).all()
    assert (shared_job.hist(sources_of=lambda j: [1, 2, 0][::-1]) == want).all()


@pytest.mark.parametrize("npieces", [33, 40])
def test_phased_many_pieces(shared_job, npieces):
    """More than 32 pieces: the unstaged path, a phase numbered at a time.  The three ranks' pieces repeat; each copy is
    a phase, so its tags are groups of their own."""
    src = [i % 3 for i in range(npieces)]
    got = shared_job.hist(sources_of=lambda j: src)
    assert (got == shared_job.oracle_hist(sources=src)).all()


def test_phased_owner_rounds(eng, monkeypatch):
    """Larger slots (KHOICE_SKM_EXCHANGE_MEAN): an owner's slot holds more k-mer instances than a table round takes and
    more chunks over all pieces than one numbering takes (4096): rounds of key subsets, numbered a phase at a time."""
    monkeypatch.setenv("KHOICE_SKM_EXCHANGE_MEAN", "2500")
    ranks = []
    for r in range(3):
        s1, t1 = species_rank(60, 1, 2, 60_000)
        s2, t2 = species_rank(61 + r, 1, 2, 60_000)
        ranks.append((s1 + s2, t1 + [1] * len(t2)))
    job, _ = run(eng, ranks, 31)
    assert job.positions_max / job.nslots > 2000


def test_hard_genomes(eng):
    """Skewed, repetitive genomes (synth.hard_species_set) on two ranks: the oracle's histogram, or KH_E_CAPACITY from an
    overfull slot (the exchange form has no side list: ADVICE medium) — never a wrong histogram.  Today kh_skm_pack
    raises KH_E_CAPACITY: the repeats send about 2300 records of a rank to the side list."""
    items = synth.hard_species_set(2, 3, 300_000)
    ranks = [([t for s, _, t in items if s == r + 1], [0] * 3) for r in range(2)]
    try:
        run(eng, ranks, 31)
    except KhoiceError as e:
        assert e.code == KH_E_CAPACITY, e


# ---------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors(eng):
    """Refused with KH_E_ARG before any launch; the device is fine afterwards."""
    seqs, tags = species_rank(1, 2, 1, 5_000)
    k = 31
    nslots, spp, cap = eng.skm_exchange_plan(k, 20_000, 1, 2)
    rec = torch.zeros((2, cap, 2), dtype=torch.int64, device="cuda")
    msk = torch.zeros((2, cap), dtype=torch.int32, device="cuda")
    cnt = torch.zeros((2, spp), dtype=torch.int32, device="cuda")
    off = torch.zeros((2, spp), dtype=torch.int32, device="cuda")
    ptrs = (rec.data_ptr(), msk.data_ptr(), cnt.data_ptr(), off.data_ptr())
    torch.cuda.synchronize()

    def refused(f):
        with pytest.raises(KhoiceError) as ei:
            f()
        assert ei.value.code == KH_E_ARG, ei.value

    for bad_k in (16, 33):
        refused(lambda: eng.skm_exchange_plan(bad_k, 20_000, 1, 2))
        refused(lambda: eng.skm_pack(seqs, tags, bad_k, nslots, 2, cap, *ptrs))
        refused(lambda: eng.skm_phased_histogram(bad_k, [(ptrs[0], ptrs[1], ptrs[2], ptrs[3])], spp, 5000, 64))
    refused(lambda: eng.skm_exchange_plan(k, 20_000, 1, 0))
    refused(lambda: eng.skm_pack(seqs, tags, k, nslots, 0, cap, *ptrs))
    refused(lambda: eng.skm_pack(seqs, [0, 32], k, nslots, 2, cap, *ptrs))            # tag 32
    refused(lambda: eng.skm_pack(seqs, [0, 2], k, nslots, 2, cap, *ptrs))             # tag 1 has no sequence
    piece = [(ptrs[0], ptrs[1], ptrs[2], ptrs[3])]
    refused(lambda: eng.skm_phased_histogram(k, piece, spp, 5000, 1))
    refused(lambda: eng.skm_phased_histogram(k, piece, spp, 0, 64))
    torch.cuda.synchronize()
    run(eng, [(seqs, tags), species_rank(5, 1, 2, 5_000)], k)
