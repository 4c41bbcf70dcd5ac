// khoice_amd — the super-k-mer form of the fused experiment-type-1 path (gfx950, wave64).
//
// What it replaces: steps 1-8 of workflow/rules/exp_type_1.smk:156-259 when only the histograms and the
// per-genome distinct counts are wanted (kh_exp1_run without group_sets / across_set).  The key-array
// form (kh_kernels.hip: passes A-C + k_union_hash) moves every k-mer through HBM as an 8-byte key three
// times.  KMC itself does not do that: it bins *super-k-mers* by a minimizer signature.  Same idea here,
// laid out for this machine:
//
//   k_skm_scatter   bases -> hash of every canonical m-mer -> sliding minimum over the w = k-m+1 m-mers of
//                   a k-mer (the minimizer) -> slot = f(minimizer).  A k-mer and its reverse complement
//                   have the same canonical m-mers, hence the same slot; consecutive k-mers mostly share
//                   their minimizer, so a run of n of them travels as ONE 16-byte record (n + k - 1 bases
//                   at two bits, genome tag, n; a run may go on into the next thread's positions): ~2 bytes
//                   per k-mer instead of 8.  2048 records are counting-sorted by coarse bucket in LDS and
//                   flushed as runs (one global atomic per run, cursors on separate memory channels).
//   k_skm_regroup   one workgroup per coarse bucket, 8192 records per round: the same LDS counting sort by
//                   fine slot (cursors in LDS: the workgroup owns its slots) -> every slot of the key space
//                   is one contiguous record range.
//   k_skm_union     one workgroup of 1024 threads per slot: records -> k-mers (balanced: a thread takes 4
//                   consecutive k-mer indices of the slot, whatever records they fall in) -> canonical key -> LDS hash
//                   set {key, genome mask} -> popcount per group / number of groups -> histogram bins.
//                   A repeated (key, genome) pair is seen when its mask bit is already set: distinct
//                   k-mers of a genome = its valid k-mer instances - those repeats.
//
// Nothing here is ordered and nothing needs to be: equal k-mers only have to meet, and they do because the
// slot is a function of the k-mer as a set of m-mers.  All integer work, no MFMA.
#include <hip/hip_runtime.h>

#include "kh_device.h"
#include "kh_launch.h"

// Diagnostic build only (-DKH_STAMPS): thread 0 of a workgroup stores the shader clock at phase boundaries.
#ifdef KH_STAMPS
__device__ u64* g_skm_stamps = nullptr;
void kh_debug_set_stamps_skm(u64* p) { (void)hipMemcpyToSymbol(HIP_SYMBOL(g_skm_stamps), &p, sizeof p); }
#define SKM_STAMP(idx)                                                                     \
    do {                                                                                   \
        __builtin_amdgcn_sched_barrier(0);                                                 \
        if (threadIdx.x == 0 && g_skm_stamps)                                              \
            g_skm_stamps[((u64)blockIdx.y * gridDim.x + blockIdx.x) * 16 + (idx)] = __builtin_amdgcn_s_memtime(); \
        __builtin_amdgcn_sched_barrier(0);                                                 \
    } while (0)
#else
#define SKM_STAMP(idx) do {} while (0)
#endif
// (-DKH_STAMPS_WG with -DKH_STAMPS: two stamps per workgroup, the beginning and the end of its walk, instead of the
// per-slot ones: when do the workgroups of the persistent union finish?  Word 1: the hardware id of the wave, word 2:
// the XCC; words 3 and 11: the constant-rate clock, which all XCCs share.)
#if defined(KH_STAMPS) && defined(KH_STAMPS_WG)
#define SKM_USTAMP(idx) do {} while (0)
#define SKM_WGSTAMP(idx)                                                                   \
    do {                                                                                   \
        __builtin_amdgcn_sched_barrier(0);                                                 \
        if (threadIdx.x == 0 && g_skm_stamps) {                                            \
            u64* const sp_ = g_skm_stamps + (u64)blockIdx.x * 16;                          \
            sp_[(idx)] = __builtin_amdgcn_s_memtime();                                     \
            sp_[(idx) + 3] = wall_clock64();                                               \
            if ((idx) == 0) {                                                              \
                sp_[1] = __builtin_amdgcn_s_getreg(4 | (31 << 11));                        \
                sp_[2] = __builtin_amdgcn_s_getreg(20 | (31 << 11));                       \
            }                                                                              \
        }                                                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                 \
    } while (0)
#elif defined(KH_STAMPS)
#define SKM_WGSTAMP(idx) do {} while (0)
#define SKM_USTAMP(idx)                                                                    \
    do {                                                                                   \
        __builtin_amdgcn_sched_barrier(0);                                                 \
        if (threadIdx.x == 0 && g_skm_stamps) g_skm_stamps[(u64)slot * 16 + (idx)] = __builtin_amdgcn_s_memtime(); \
        __builtin_amdgcn_sched_barrier(0);                                                 \
    } while (0)
// (words 12 and 13 of a slot: the workgroup that walked it and the slot's place in that walk, so that a reader can put
// a workgroup's slots behind each other: tools/union_stamps.py)
#define SKM_USTAMP_WALK(seq)                                                               \
    do {                                                                                   \
        if (threadIdx.x == 0 && g_skm_stamps) {                                            \
            g_skm_stamps[(u64)slot * 16 + 12] = blockIdx.x + 1u;                           \
            g_skm_stamps[(u64)slot * 16 + 13] = (seq);                                     \
        }                                                                                  \
    } while (0)
#else
#define SKM_USTAMP(idx) do {} while (0)
#define SKM_WGSTAMP(idx) do {} while (0)
#endif
#ifndef SKM_USTAMP_WALK
#define SKM_USTAMP_WALK(seq) do {} while (0)
#endif
#if defined(KH_STAMPS) && defined(KH_STAMPS_WG)   // (the scatter's workgroups likewise; its phase stamps share the words: off)
#undef SKM_STAMP
#define SKM_STAMP(idx) do {} while (0)
#endif

// ISA study only (-DKH_MARKS with --cuda-device-only -S): comments that delimit the sections of the union in the assembly
#ifdef KH_MARKS
#define SKM_MARK(name) asm volatile("; ===== MARK " name ::: "memory")
#else
#define SKM_MARK(name) do {} while (0)
#endif
#ifndef KH_TUNE_SKM_SCATTER_WAVES
#define KH_TUNE_SKM_SCATTER_WAVES 3   // waves per SIMD the scatter is compiled for (workgroups of 4 waves per CU)
#endif

#include "kh_skm_device.h"   // (after SKM_STAMP: the shared flush carries stamps)

static size_t kh_skm_scatter_lds_bytes(u32 nb1) {
    const u32 nbk = (nb1 + 3) & ~3u;
    return flush_lds_bytes<SKM_CAP>(nbk) + (size_t)SKM_CW * 4 + (((size_t)SKM_CW * 2 + 15) & ~(size_t)15) + 64 * 4 + 4 * 32 * 4 +
           (size_t)SKM_NT * 8 + 64;
}

// ------------------------------------------------------------------------------------------
// S1: bases -> records, partitioned by coarse bucket.  WW = m-mers per k-mer (k - m + 1), compile time:
// the sliding minimum is register arithmetic with constant indices.
// ------------------------------------------------------------------------------------------
template <int WW>
__global__ __launch_bounds__(SKM_NT, KH_TUNE_SKM_SCATTER_WAVES) void k_skm_scatter(const KhSkmJob jb) {
    extern __shared__ __attribute__((aligned(16))) u8 lds_raw[];
    const u32 nbk = (jb.nb1 + 3) & ~3u;
    const FlushLds L = flush_lds<SKM_CAP>(lds_raw, nbk);
    u8* p = lds_raw + flush_lds_bytes<SKM_CAP>(nbk);
    u32* code = reinterpret_cast<u32*>(p);                    p += (size_t)SKM_CW * 4;
    u16* bad16 = reinterpret_cast<u16*>(p);                   p += ((size_t)SKM_CW * 2 + 15) & ~(size_t)15;
    u32* tailh = reinterpret_cast<u32*>(p);                   p += 64 * 4;       // hashes of positions SUB .. SUB + 63
    u32* xch = reinterpret_cast<u32*>(p);                     p += 4 * 32 * 4;   // [wave][j]: hashes of the wave's first thread
    uint2* lrun = reinterpret_cast<uint2*>(p);                p += (size_t)SKM_NT * 8;   // [thread]: {cont, ext}, read by the record builders
    u32* misc = reinterpret_cast<u32*>(p);                    // [1] valid k-mers of the tile, [2] scratch, [4..] scan scratch

    const u32 tid = threadIdx.x, lane = lane_id(), wid = tid >> 6;
    const KhTile t = jb.tiles[blockIdx.x];
    const KhSeg sg = jb.segs[t.seg];
    const u32 rtag = jb.seg_tag ? jb.seg_tag[t.seg] : t.seg;   // the tag of the tile's records: the genome, or its group
    const int k = jb.k, m = jb.m;
    const u32 nslots = jb.nslots, S = jb.S, nmax = jb.nmax;
    const u64 smagic = ((1ull << 40) + S - 1) / S;   // slot / S == (slot * smagic) >> 40 for slot < 2^20
    const u32 mmask = m >= 16 ? 0xffffffffu : ((1u << (2 * m)) - 1u);
    const u64 tile_pos0 = (u64)t.tile_in_seg * jb.tile_pos;
    const int subtiles = (int)(jb.tile_pos / SKM_SUB);

    SKM_WGSTAMP(0);
    for (u32 i = tid; i < nbk; i += SKM_NT) L.bcnt[i] = 0;
    if (tid < 4) misc[tid] = 0;
    u32 staged = 0, tile_recs = 0;   // uniform

    SkmFetch pre;
    for (int sub = 0; sub < subtiles; ++sub) {
        const u64 p0 = tile_pos0 + (u64)sub * SKM_SUB;
        if (p0 >= sg.npos) break;   // uniform
        __syncthreads();
        const bool stamp = sub == 1;
        if (stamp) SKM_STAMP(0);
        skm_fetch(sg.seq, sg.len, p0, pre);   // (fetched one sub-tile ahead into registers: 0.656 ms against 0.624, three workgroups per CU hide the load as well)
        skm_store(pre, code, bad16);
        __syncthreads();
        if (stamp) SKM_STAMP(1);
        // ---- hashes of the m-mers starting at the thread's 32 positions
        u32 cw[3];   // bases p .. p + 47: the last of the thread's m-mers ends at base p + 31 + 15
#pragma unroll
        for (int i = 0; i < 3; ++i) cw[i] = code[2 * tid + i];
        u32 cur[SKM_PPT + WW - 1];
        {   // Both strands of the m-mer at a compile-time position j are one funnel shift each: the reverse complement
            // (base i at bits 2i, complemented) of the complemented words, the forward strand (first base on top) of the
            // words with their 2-bit groups reversed — what the 64 tail threads below do from LDS.
            u32 cv[3], rv[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) { cv[i] = ~cw[i]; rv[i] = revpairs32(cw[i]); }
            const u32 fsh = 32u - 2u * (u32)m;
#pragma unroll
            for (int j = 0; j < (int)SKM_PPT; ++j) {
                const int w = j >> 4, o = j & 15;
                const u32 f = (o ? __builtin_amdgcn_alignbit(rv[w], rv[w + 1], 32 - 2 * o) : rv[w]) >> fsh;
                const u32 r = __builtin_amdgcn_alignbit(cv[w + 1], cv[w], 2 * o) & mmask;
                cur[j] = mmer_hash(f < r ? f : r);
            }
        }
        if (WW > 1) {
            if (tid < 64) {   // positions SUB .. SUB + 63, straight from the packed window
                const u32 q = SKM_SUB + tid, wq = q >> 4, oq = q & 15u;
                const u32 x = __builtin_amdgcn_alignbit(code[wq + 1], code[wq], 2 * oq) & mmask;
                const u32 f = revpairs32(x) >> (32 - 2 * m);
                const u32 r = (~x) & mmask;
                tailh[tid] = mmer_hash(f < r ? f : r);
            }
            if (lane == 0) {
#pragma unroll
                for (int j = 0; j < WW - 1; ++j) xch[wid * 32 + j] = cur[j];
            }
            __syncthreads();
            // the first WW - 1 hashes of the next thread: next lane, or the next wave's first thread
            const u32* nx = wid + 1 < SKM_NT / 64 ? xch + (wid + 1) * 32 : tailh;
#pragma unroll
            for (int j = 0; j < WW - 1; ++j) {
                const u32 edge = lane == KH_WAVE - 1 ? nx[j] : 0u;
                cur[SKM_PPT + j] = next_lane(cur[j], edge);
            }
            window_min<WW>(cur);
        }
        if (stamp) SKM_STAMP(2);
        // ---- which of the 32 start positions have k valid bases
        u32 vm;
        {
            u64 bm = (u64)bad16[2 * tid] | ((u64)bad16[2 * tid + 1] << 16) | ((u64)bad16[2 * tid + 2] << 32) |
                     ((u64)bad16[2 * tid + 3] << 48);
            u32 cover = 1;
            while (2 * cover <= (u32)k) { bm |= bm >> cover; cover <<= 1; }
            bm |= bm >> ((u32)k - cover);
            vm = ~(u32)bm;
        }
        // ---- runs of valid positions with one minimizer become records
        // (the hash is a bijection: equal minimizer hashes = one minimizer = one slot; the slot itself is
        // worked out once per record, by the thread that builds it)
        u32 cont = 0;
#pragma unroll
        for (int j = 1; j < (int)SKM_PPT; ++j)
            if (cur[j] == cur[j - 1]) cont |= 1u << j;
        cont &= vm & (vm << 1);
        // A run may go on into the NEXT thread of the wave (not past the wave's 2048 positions, not over more than
        // one boundary, not beyond nmax k-mers): then its record belongs to the thread it starts in, and the next
        // thread's leading positions are not starts.  Down the wave: minimizer and length of my last run; back up:
        // how many of the next thread's positions join it.  (Records cut at every 32 positions held 6.8 k-mers
        // where the minimizer runs average 8.5.)
        const u32 tr = (vm >> 31) ? 1u + (u32)__builtin_clz(~cont | 1u) : 0u;            // my last run's k-mers (32: all of mine)
        const u32 lead = 1u + (u32)__builtin_ctz(~(cont >> 1));                            // positions 0 .. lead-1 continue position 0's run
        const u32 p_min = (u32)__builtin_amdgcn_update_dpp(0, (int)cur[SKM_PPT - 1], 0x138, 0xf, 0xf, false);   // wave_shr:1
        const u32 p_tr = (u32)__builtin_amdgcn_update_dpp(0, (int)tr, 0x138, 0xf, 0xf, false);
        const bool merge_in = lane != 0 && p_tr != 0 && (vm & 1u) && p_min == cur[0] && p_tr + lead <= nmax;
        const u32 ext = next_lane(merge_in ? lead : 0u, 0u);   // k-mers of the next thread that join my last run
        const u32 starts = (vm & ~cont) & ~(merge_in ? 1u : 0u);
        auto run_len = [&](u32 c, u32 e, u32 s) -> u32 {
            const u32 len = 1u + (u32)__builtin_ctzll(~((u64)c >> (s + 1)));
            return s + len == SKM_PPT ? len + e : len;
        };
        lrun[tid] = make_uint2(cont, ext);
        // One record per start, unless a run is longer than nmax k-mers, i.e. cont holds nmax consecutive ones.
        // (A run joined by the next thread is never cut: the join asks for tr + lead <= nmax.)  Such threads
        // ("split") count and describe their records one start at a time; they are rare (tandem repeats).
        bool split;
        {
            u32 y = cont, c = 1;
            while (2 * c <= nmax) { y &= y >> c; c <<= 1; }
            split = (y & (y >> (nmax - c))) != 0u;
        }
        const bool any_split = __ballot(split) != 0;   // uniform
        u32 nrec = (u32)__popc(starts);
        if (any_split && split) {
            nrec = 0;
            u32 st = starts;
            while (st) {
                const u32 s = (u32)__builtin_ctz(st);
                st &= st - 1;
                nrec += (run_len(cont, ext, s) + nmax - 1) / nmax;
            }
        }
        {   // valid k-mer instances of the tile
            const u32 tot = wave_scan_add((u32)__popc(vm));
            if (lane == KH_WAVE - 1 && tot) atomicAdd(&misc[1], tot);
        }
        if (stamp) SKM_STAMP(3);
        // ---- append to the staging array; a full array is flushed (a prefix of the threads fits).
        // Two steps: every thread writes one descriptor {thread, start, n or 0, minimizer} into the first 8 bytes of
        // the staging entry each of its records will occupy; then the wave's records (contiguous) are built by its
        // 64 lanes in turn, each from the sub-tile's code words in LDS, and overwrite their descriptors.  The
        // divergent per-thread loop over starts it replaces ran as often as the busiest lane of the wave.
        if (stamp) SKM_STAMP(4);
        uint2* const dsc = reinterpret_cast<uint2*>(L.stage);   // descriptor of staging entry i: dsc[2 * i]
        bool done = false, first_round = true;
        while (true) {
            const u32 mine = done ? 0u : nrec;
            const u32 incl = wave_scan_add(mine);
            if (lane == KH_WAVE - 1) misc[4 + wid] = incl;
            __syncthreads();
            u32 excl = incl - mine, total = 0;
            for (u32 q = 0; q < SKM_NT / 64; ++q) {
                const u32 v = misc[4 + q];
                excl += q < wid ? v : 0u;
                total += v;
            }
            if (first_round) { tile_recs += total; first_round = false; }
            const bool fits = staged + excl + mine <= SKM_CAP;
            const bool wrote = !done && fits;
            if (stamp) SKM_STAMP(9);
            if (wrote) {
                const u32 at = staged + excl;
                if (!split) {   // predicated compaction over the 32 positions: no run-time register index
                    u32 sv = starts, tb = tid << 5;
                    asm volatile("" : "+v"(sv), "+v"(tb));   // (keeps 32 ranks / 32 tags from being hoisted out of the loops as live registers)
#pragma unroll
                    for (int j = 0; j < (int)SKM_PPT; ++j)
                        if (sv & (1u << j))
                            dsc[2 * (at + (u32)__popc(sv & ((1u << j) - 1u)))] = make_uint2(tb | (u32)j, cur[j]);
                } else {
                    u32 sl[SKM_PPT];
#pragma unroll
                    for (int j = 0; j < (int)SKM_PPT; ++j) sl[j] = cur[j];
                    u32 a = at, st = starts;
                    while (st) {
                        const u32 s = (u32)__builtin_ctz(st);
                        st &= st - 1;
                        const u32 minv = pick32(sl, s);
                        for (u32 s2 = s, len = run_len(cont, ext, s); len; ) {
                            const u32 n = len < nmax ? len : nmax;
                            dsc[2 * a++] = make_uint2((n << 16) | (tid << 5) | s2, minv);
                            s2 += n;
                            len -= n;
                        }
                    }
                }
            }
            // The lanes that wrote are consecutive, and those before them in the wave wrote in an earlier round
            // (mine = 0 now): the wave's new records are staging entries base .. base + cnt - 1.
            const u64 wm = __ballot(wrote);
            if (wm) {   // uniform
                const u32 base = staged + (u32)__builtin_amdgcn_readlane((int)excl, 0);
                const u32 cnt = (u32)__builtin_amdgcn_readlane((int)incl, 63 - __builtin_clzll(wm));
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                for (u32 r = lane; r < cnt; r += KH_WAVE) {
                    const u32 at = base + r;
                    const uint2 d = dsc[2 * at];
                    const u32 src = (d.x >> 5) & (SKM_NT - 1), s = d.x & 31u;
                    const uint2 li = lrun[src];
                    const u32 n = (d.x >> 16) ? (d.x >> 16) : run_len(li.x, li.y, s);
                    const u32 slot = slot_of(d.y, nslots);
                    const u32 coarse = (u32)(((u64)slot * smagic) >> 40), fine = slot - coarse * S;
                    // bases src * 32 + s .. + n + k - 2 (at most 31 + 54 < 96: inside the thread's window)
                    const u32 bp = src * SKM_PPT + s, sh = 2 * (bp & 15u);
                    const u32* cq = code + (bp >> 4);
                    const u32 c0 = cq[0], c1 = cq[1], c2 = cq[2], c3 = cq[3], c4 = cq[4];
                    const int bits = 2 * ((int)n + k - 1);   // 2k .. 108
                    auto keep = [](u32 x, int b) -> u32 { return b >= 32 ? x : (b <= 0 ? 0u : x & ((1u << b) - 1u)); };
                    const u32 x0 = __builtin_amdgcn_alignbit(c1, c0, sh);
                    const u32 x1 = keep(__builtin_amdgcn_alignbit(c2, c1, sh), bits - 32);
                    const u32 x2 = keep(__builtin_amdgcn_alignbit(c3, c2, sh), bits - 64);
                    const u32 x3 = keep(__builtin_amdgcn_alignbit(c4, c3, sh), bits - 96) | SkmRec1::header(fine, rtag, n);
                    L.stage[at] = make_uint4(x0, x1, x2, x3);
                    L.sid[at] = (u16)coarse;
                    atomicAdd(&L.bcnt[coarse], 1u);
                }
            }
            if (wrote) done = true;
            // records appended in this round: those of the fitting prefix of threads
            if (stamp) SKM_STAMP(5);
            const u32 room = SKM_CAP - staged;
            if (total <= room) {   // all fitted: the common case
                staged += total;
                if (stamp) SKM_STAMP(6);
                __syncthreads();
                if (stamp) { SKM_STAMP(7); SKM_STAMP(8); }
                break;
            }
            // some threads did not fit: the prefix that did ends at the largest excl + mine <= room
            if (tid == 0) misc[2] = 0;
            __syncthreads();
            if (fits && mine) atomicMax(&misc[2], excl + mine);
            __syncthreads();
            const u32 part = misc[2];
            if (stamp) SKM_STAMP(10);
            skm_flush<SKM_NT, SKM_CAP, false>(L, staged + part, jb.nb1, jb.cur1, jb.reg1, jb.cap1, jb.ctl);
            if (stamp) SKM_STAMP(11);
            staged = 0;
        }
    }
    __syncthreads();
    if (staged) skm_flush<SKM_NT, SKM_CAP, false>(L, staged, jb.nb1, jb.cur1, jb.reg1, jb.cap1, jb.ctl);
    if (tid == 0 && misc[1]) atomicAdd(&jb.inst[t.seg], (unsigned long long)misc[1]);
    if (tid == 0 && tile_recs) atomicAdd(jb.ctl + KH_SKM_CTL_RECORDS, tile_recs);
#if defined(KH_STAMPS) && defined(KH_STAMPS_WG)
    __syncthreads();   // (the workgroup's end, not thread 0's)
#endif
    SKM_WGSTAMP(8);
}

// ------------------------------------------------------------------------------------------
// S2b: one slot per workgroup -> LDS hash set {canonical k-mer, genome mask} -> histogram bins.
//
// 1. Identical records are expanded ONCE.  A record is a content-defined piece of sequence (a run of k-mers with
//    one minimizer), so the genomes of a species hold the same records wherever they agree: the slot's records
//    (one per thread) meet in a small LDS hash set keyed by their bases; a record that finds its own content
//    already there ORs its genome bit into the first one's mask and retires (a copy inside the SAME genome: all
//    its k-mers are repeats).  Related genomes (the workload the reference is written for: groups of one species)
//    halve the k-mers that reach the big table; unrelated ones lose one LDS round trip.
// 2. Records -> k-mers: every surviving record is cut into chunks of 4 consecutive k-mers, a scan numbers the
//    chunks, a thread takes one chunk: first k-mer by a funnel shift + reversal of the 2-bit groups, the other
//    three by ROLLING both strands (32-bit halves: a funnel shift and a shift-or each); the keys of a thread share
//    one genome mask.
// 3. Insertion: rounds of 4 compare-and-swaps per thread.  A key gets KH_HASH_ROUNDS probes in the main table,
//    moves to a small second table with an independent hash, and from a full second table back to unbounded
//    probing of the main one; occupied entries stay occupied, so every copy of a key takes the same decisions as
//    the first.  (Measured and rejected: finishing the keys that lost round 1 one per lane in a loop — fewer
//    instructions, but a chain of ~20 dependent LDS round trips per wave: 2.63 ms against 2.30; and the same keys
//    packed into the wave's first lanes, all walking at once: see at the kernel.)
//    The waves that hold records run the merge of identical records at a raised priority.
// 4. Read-out: the thread whose compare-and-swap CREATED an entry remembers where; once all masks are final it
//    turns its own entries into histogram bins (popcount per group / number of groups).  Nobody scans the table,
//    no key is read again, waves without chunks have nothing to do.  The read is an exchange that stores zero: the
//    mask planes are clean for the next slot without being cleared (1.430 -> 1.407 ms).  A lean slot's read-out
//    waits for the next slot's first barrier and shares a barrier interval with that slot's merge of identical
//    records (the slot timeline at the kernel).
//
// Geometry <NT, T>: threads and table entries of a workgroup.  <1024, 4096>: 79 KB of LDS, two workgroups per CU.
// (<512, 2048> with four per CU and <640, 2560> with three were measured slower: DESIGN.md §3, §8.)
// ------------------------------------------------------------------------------------------
#ifndef KH_TUNE_SKM_UE
#define KH_TUNE_SKM_UE 2
#endif
constexpr u32 SKM_UE = KH_TUNE_SKM_UE;                // k-mers per chunk (2 or 4)
constexpr u32 SKM_OB = SKM_UE == 2 ? 4 : 3;           // bits of a chunk's number inside its record (n <= 31)
constexpr u32 SKM_PASSES = SKM_UE == 2 ? 3 : 2;       // chunks of a slot: at most SKM_PASSES per thread
template <u32 NT, u32 T> struct SkmUnionGeo {
    static constexpr u32 TABLE = T;                   // main table
    static constexpr u32 T2 = 128;                    // second table
    static constexpr u32 MAXREC = NT;                 // records of a slot (cap2 <= this): one per thread
    static constexpr u32 MAXCH = SKM_PASSES * NT;     // chunks of a slot (after the merge of identical records)
    static constexpr size_t LDS = (size_t)T * 16 + (size_t)T2 * 16 + 1024 + 128 + 256 + (size_t)SKM_HSTRIPE_WORDS * 4 +
                                  (size_t)MAXCH * 2 + (size_t)MAXREC * 4;
    static_assert(MAXREC * 16 <= T * 4, "records are staged in the first half of the key plane");
    static_assert(T2 <= NT && T % 4 == 0, "table planes are cleared 16 bytes at a time");
    static_assert((T & (T - 1u)) == 0u, "table indices wrap by a mask");
};
using SkmUnion = SkmUnionGeo<1024, 4096>;
static_assert(SkmUnion::TABLE == 4096, "the slot geometry and its measurements (skm_plan) are the 4096-entry table's");

__device__ __forceinline__ u32 key_hash2(u32 lo, u32 hi) { return (lo ^ hi) * 0x9E3779B1u; }

// ------------------------------------------------------------------------------------------
// Record -> canonical k-mers, one chunk of E consecutive k-mers (k_skm_big, k_skm_phased; k_skm_union keeps a twin of
// this in its own body, see there).  The first k-mer by a funnel shift + reversal of the 2-bit groups, the others by
// ROLLING both strands (32-bit halves: a funnel shift and a shift-or each).  f(e, cl, ch) gets the canonical key of
// every e < E as two halves, also of those behind the record's last k-mer: the caller knows how many it wants.
// ------------------------------------------------------------------------------------------
struct Skm1Consts {   // per launch: the 2k-bit mask and where the last base of a k-mer sits, as 32-bit halves (15 <= k <= 32)
    u32 kml, kmh;
    u32 fsh;          // right-aligns a reversed window
    u32 tsh;          // 2k - 2: 28 .. 62
    u32 tsh_sub;      // the same inside its word
    bool tsh_high;    // (uniform) the last base of a k-mer sits in the high word
    __device__ __forceinline__ explicit Skm1Consts(const int k)
        : kml((u32)kh_mask(2 * k)), kmh((u32)(kh_mask(2 * k) >> 32)), fsh(64u - 2u * (u32)k), tsh(2u * (u32)k - 2u),
          tsh_sub(tsh >= 32u ? tsh - 32u : tsh), tsh_high(tsh >= 32u) {}
};
template <int E, class F>
__device__ __forceinline__ void skm1_expand(const uint4 r0, const u32 first, const Skm1Consts& kc, F&& f) {
    const u64 clo = ((u64)r0.y << 32) | r0.x, chi = ((u64)r0.w << 32) | r0.z;
    const u32 sh = 2u * first;   // 0, 2E, .. <= 60
    const u64 lo = sh ? (clo >> sh) | (chi << (64u - sh)) : clo, hi = chi >> sh;
    const u32 xl = (u32)lo & kc.kml, xh = (u32)(lo >> 32) & kc.kmh;   // the first k-mer, base j at bits 2j
    const u64 fw = kh_revpairs64(((u64)xh << 32) | xl) >> kc.fsh;
    u32 fl = (u32)fw, fh = (u32)(fw >> 32), rl = ~xl & kc.kml, rh = ~xh & kc.kmh;
    const u32 t = (u32)((lo >> kc.tsh) | (hi << (64u - kc.tsh)));   // bits 2e: the last base of the chunk's k-mer e
    const u32 tc = ~t;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        if (e) {   // roll both strands by one base
            fh = __builtin_amdgcn_alignbit(fh, fl, 30) & kc.kmh;
            fl = ((fl << 2) | ((t >> (2 * e)) & 3u)) & kc.kml;
            rl = __builtin_amdgcn_alignbit(rh, rl, 2);
            rh >>= 2;
            if (kc.tsh_high) rh |= ((tc >> (2 * e)) & 3u) << kc.tsh_sub; else rl |= ((tc >> (2 * e)) & 3u) << kc.tsh_sub;
        }
        const bool fwd = fh < rh || (fh == rh && fl < rl);
        f((u32)e, fwd ? fl : rl, fwd ? fh : rh);
    }
}
// the claim of the probe walk for a one-word key: one 64-bit compare-and-swap
struct SkmClaim1 {
    unsigned long long* tkey;   // key plane of the main table
    u32 okey_off;               // the second table's, in entries behind it (one base pointer, an integer choice)
    unsigned long long empty, K;
    __device__ __forceinline__ u32 operator()(const bool second, const u32 S) const {
        const unsigned long long o2 = atomicCAS(tkey + (second ? okey_off : 0u) + S, empty, K);
        return o2 == empty ? SKM_FRESH : (o2 == K ? SKM_SAME_KEY : SKM_OTHER_KEY);
    }
};

// PERSISTENT: the grid is two workgroups per CU (what the LDS allows); a workgroup walks slots blockIdx.x,
// blockIdx.x + gridDim.x, ... for the first half of its rounds and takes the rest by claim from a device counter
// (SkmSlotFeed, kh_skm_device.h: the two workgroups of a CU do not run at the same speed; with equal shares the one
// dispatched first left at 0.75 of the kernel's time and the other finished alone, 13 % of the wave-slots stood
// empty).  While it works on one slot the record of the next one is already on its way to the
// thread's registers and the count of the one after to a scalar register: a workgroup that started with "load the
// count, then load the records" spent 2.5 of its 6 microseconds waiting for memory with nothing else to do.  The
// histogram bins and the repeat counters stay in LDS over all slots of the workgroup and are written once.
//
// A SLOT, barrier by barrier.  Two of its phases leave most of the workgroup idle on disjoint memory: in the merge of
// identical records only the waves that hold a record work (key plane, rmask, owner, scratch[0]; adds to dupc), in the
// read-out only the creators of entries (mask planes, gtab, hstripe; adds to dupc).  So a lean slot's insertion leaves
// `made` in registers and its read-out runs behind the NEXT slot's barrier 1, in one barrier interval with that slot's merge:
//   B4(s) | stage(s+1) + clear dd | B1 | { merge(s+1), then read-out(s) } | B2 | clear keys | B3 | expand + insert(s+1) | B4(s+1)
// A wave with both jobs merges first.  The first slot of a walk finds nothing to read out, the last slot's read-out runs
// alone behind the loop, an empty slot (R0 = 0: three barriers, no insertion) reads out its predecessor like any other
// and leaves nothing behind.  Union 1.227 -> 1.171 ms against the read-out directly behind barrier 4; 61 VGPRs against
// 60, no scratch either way.
//
// TWO BODIES behind the third barrier (`slot_body`).  A slot whose merged k-mers fit the table (N <= T, what the planner
// aims at: nearly every slot) takes the LEAN one: no subset loop, no subset filter per key, no clears and barriers
// between subsets, and none of the scalars those keep alive; its read-out is the deferred one above.  A slot with N > T
// takes the MULTI one: R = ceil(N / T) subsets of its keys, chosen by hash bits, inserted and read out one after the
// other on the same planes, every read-out directly behind its subset's barrier 4 (every subset needs its masks
// evaluated before the next one is inserted, the last one included: a multi slot leaves nothing behind).  Both are one
// piece of code with a compile-time flag; the masks-self-clean invariant (at the read-out) holds for either, so lean
// and multi slots may follow each other in any order in one workgroup's walk.  KH_SKM_CTL_MULTI counts the multi slots.
// KT: k at compile time (17 .. 32; the masks and shifts of the expansion are immediates), 0: k from the job (15, 16).
//
// ONE PRIORITY RAISE: the waves that hold records run the merge, from barrier 1 to barrier 2, at wave priority 1
// (s_setprio ignores EXEC, so the guard is a ballot and compiles to an s_cbranch).  Arbitration goes by priority, then
// by age: only the ~6 waves of 16 that hold records work in the merge, and in the younger workgroup of a CU they queued
// behind the bulk insertion of the older one.  Union 1.258 -> 1.226 ms; it holds against read-out waves too (1.180 ->
// 1.209 without it).
//
// LDS ROUND TRIPS BETWEEN BARRIERS 1 AND 2.  The merge loop makes two dependent round trips per iteration (the
// compare-and-swap on `dd`, one 16-byte read of the staged record, compared without a branch per word); a copy's OR
// into the survivor's mask is issued once behind the loop and waited for behind the chunk numbering.  With the compare
// as an `&&` chain (three dependent reads) and the OR waited for inside the loop it made five: union 1.170 -> 1.090 ms,
// B1->B2 7700 -> 7164 ticks per slot.  The read-out made four per pass with both fields set (the exchange pair, then
// the gtab read of the mask's lowest genome, per entry) and makes two: the gtab entry it starts from is that of the
// creator's OWN genome, known from `made`, fetched once per pass ahead of the exchanges (`eval_mask`).  That dependent
// read was what the read-out cost: halving the vector instructions of an entry (52 -> 25: one index space for both
// tables, the first group outside the loop, bin offsets in bytes) bought 0.008 ms of 1.088, a timing build that
// evaluated nothing 0.101; what taking the read off the chain bought: profiles/README.md, round 12.
//
// MEASURED AND REJECTED.  Each was a compile-time switch of this kernel up to the commit "k_skm_union: read out a slot
// during the next slot's merge interval", where the code can be found; every number: profiles/README.md, DESIGN.md §8.
//   - the keys that lose probe round 1 packed into the wave's first lanes by ds_permute, one key per lane through the
//     tiers: 129 -> 40 static vector instructions, but a chain of dependent LDS round trips: 1.258 -> 1.417 / 1.347 ms.
//   - priority also on the one-key-per-lane finish and on the wave that draws the claim: 1.223 / 1.227 against 1.226,
//     inside the noise rule; priority levels 1 and 3 time the same.
//   - a wave with both jobs reads out first, then merges: 1.180 ms against 1.171.
//   - chunks numbered from the last thread down (the record-holding waves get chunks last): 1.215 / 1.212 against
//     1.180 / 1.171; why was not looked into.
//   - the mask planes cleared per slot instead of zeroed by the read-out's exchange: 1.430 against 1.407 ms.
// Forms of the read-out tried when the merge loop was shortened (never committed; their code and every number:
// profiles/README.md, round 11), each on top of the merge as it is now, which alone times 1.090 ms:
//   - the read-out of all entries of a thread at once (the exchanges of both fields back to back, a field without an
//     entry exchanging zero for zero at a spare word; the gtab reads of both entries in common group rounds): two
//     round trips per pass instead of four, 3630 -> 3665 static vector instructions in the kernel and 370 more scalar
//     ones and waits: 1.122 ms, alone 1.195 against 1.170.
//   - the same with a branch per field (the compiler parts the two exchange pairs by a wait): 1.119 ms.
//   - only the exchanges together, the entries evaluated one after the other as before: 1.103 ms.
//   Why was not found.  What the common rounds do at run time and the counts above do not show: both entries' code
//   runs for as many rounds as the slower entry needs, and every field without an entry makes two exchanges.
#define KH_TUNE_SKM_UNION_COMPACT 0   // (read by no code: the previous commit's tests/test_gpu_skm_union_tail.py parses this line at import)
template <u32 NT, u32 T, int KT>
__global__ __launch_bounds__(NT, 8) void k_skm_union(const KhSkmJob jb, u32 cs, u32 first_claimed) {
    extern __shared__ __attribute__((aligned(16))) u8 lds_raw[];
    using G = SkmUnionGeo<NT, T>;
    constexpr u32 T2 = G::T2, NW = NT / 64;
    constexpr u32 T2SH = 25;   // 32 - log2(T2)
    constexpr int E = (int)SKM_UE;
    constexpr u64 EMPTY = ~0ull;   // never a canonical key: the reverse complement of the all-T k-mer is 0
    // Table planes: keys (8-byte stride), low and high halves of the genome masks (4-byte stride).  ONE INDEX SPACE for
    // both tables: entry i of the second table is entry T + i of each plane, so whoever knows an entry's joint index
    // (the read-out, from `made`) addresses its masks without asking which table it is in.
    // A word of `made`: two fields of 13 bits (0: no entry, else the entry's joint index + 1) and, above them, the
    // operand number of the genome whose record the thread's chunk of that pass came from.
    constexpr u32 MADE_FIELD_BITS = 13, MADE_FIELD = (1u << MADE_FIELD_BITS) - 1u, MADE_FIELDS = (1u << (2 * MADE_FIELD_BITS)) - 1u;
    constexpr u32 MADE_OWN_SHIFT = 2 * MADE_FIELD_BITS;
    static_assert(T + T2 <= MADE_FIELD, "a field of `made` holds a joint index + 1");
    static_assert(KH_TAG_MAX_OPS <= (1 << (32 - MADE_OWN_SHIFT)), "a word of `made` holds an operand number above its fields");
    u8* p = lds_raw;
    unsigned long long* tkey = reinterpret_cast<unsigned long long*>(p);   p += (size_t)(T + T2) * 8;
    u32* tmlo = reinterpret_cast<u32*>(p);                                 p += (size_t)(T + T2) * 4;
    u32* tmhi = reinterpret_cast<u32*>(p);                                 p += (size_t)(T + T2) * 4;
    unsigned long long* const okey = tkey + T;
    u32* const omlo = tmlo + T;
    u32* const omhi = tmhi + T;
    uint4* gtab = reinterpret_cast<uint4*>(p);                             p += 1024;   // per operand: its group's mask (two halves), first bin as a BYTE offset into hstripe
    u32* scratch = reinterpret_cast<u32*>(p);                              p += 128;
    u32* dupc = reinterpret_cast<u32*>(p);                                 p += 256;
    u32* hstripe = reinterpret_cast<u32*>(p);                              p += (size_t)SKM_HSTRIPE_WORDS * 4;
    u16* owner = reinterpret_cast<u16*>(p);                                p += (size_t)G::MAXCH * 2;   // chunk -> record << SKM_OB | chunk of the record
    u32* rmask = reinterpret_cast<u32*>(p);                                // [MAXREC] genomes (of one half of the mask) that hold the record
    // While identical records are merged the table is not in use yet (and its KEY plane is not read any more once a
    // slot's insertions are over): the records are staged in the first half of the key plane, the set of their
    // contents (record number + 1, 0: empty) is the second half.
    uint4* stage = reinterpret_cast<uint4*>(tkey);
    u32* dd = reinterpret_cast<u32*>(tkey) + T;
    const u32 tid0 = threadIdx.x;
    u32 tid = tid0, lane = lane_id();
    const u32 nbins = jb.nbins, cap2 = jb.cap2, nslots = jb.nslots;
    const int k = KT ? KT : jb.k;
    const u32 sshift = nbins <= 72u ? 2u : (nbins <= 144u ? 1u : 0u), smask = (1u << sshift) - 1u;
    // The keys of both tables are reset per slot (and per subset).  The mask planes are NOT: the read-out takes every
    // mask it evaluates by an exchange that stores zero (the invariant is stated there), so they are zero whenever an
    // insertion phase begins.
    auto clear_keys = [&]() {
        uint4* k4 = reinterpret_cast<uint4*>(tkey);
        for (u32 i = tid; i < T / 2; i += NT) k4[i] = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
        unsigned long long e0 = EMPTY;   // (opaque, as `emptyv` below)
        asm volatile("" : "+v"(e0));
        if (tid < T2) okey[tid] = e0;
    };
    // the record counts were written by the regroup kernel and do not change here: read through the constant address
    // space, i.e. by SCALAR loads (inside the slot loop the compiler cannot prove that for a plain global pointer)
    typedef const u32 __attribute__((address_space(4))) * ConstU32;
    const ConstU32 counts = (ConstU32)(unsigned long long)jb.cur2;
    // (a slot with more records than its region holds — the rest were spilled by the regroup — is not this kernel's:
    // it is listed for k_skm_big and counts as empty here)
    const u32 fit = cap2 < G::MAXREC ? cap2 : G::MAXREC;
    auto count_of = [&](u32 sl) -> u32 {
        const u32 n = sl < nslots ? counts[sl] : 0u;
        return n <= fit ? n : 0u;
    };
    SKM_MARK("init");
    // The read-out below is the twin of SkmReadout (kh_skm_device.h), kept in place: with the shared struct this kernel
    // had the same registers and 32 instructions fewer, and ran 1 % slower (1.431 -> 1.446 ms, three alternated runs
    // each, the parent's spread 0.003).  The BIN RULE is shared: a change of it has to be made in both; only the ORDER
    // in which a mask's groups are counted differs (here the creator's own group first, there from the lowest bit up),
    // and the group table here holds byte offsets.  The zeroing of the masks as they are read, the joint index of both
    // tables and the genome carried in `made` are this kernel's alone: the kernels built on SkmReadout clear their planes.
    // (the mask planes, once: the first slot's first barrier comes before any mask is touched)
    for (u32 i = tid; i < (T + T2) / 2; i += NT) reinterpret_cast<uint4*>(tmlo)[i] = make_uint4(0u, 0u, 0u, 0u);   // (both planes, both tables: they are adjacent)
    if (tid < (u32)KH_TAG_MAX_OPS) {
        const u32 g = jb.ginfo[tid], g0 = g & 0xffu, gn = (g >> 8) & 0xffu;
        const u64 gm = gn ? (gn >= 64u ? ~0ull : ((1ull << gn) - 1ull)) << g0 : 0ull;
        gtab[tid] = make_uint4((u32)gm, (u32)(gm >> 32), (g >> 16) << (sshift + 2u), 0u);
        dupc[tid] = 0;
    }
    if (tid < SKM_HSTRIPE_WORDS) hstripe[tid] = 0;
    if (tid == 0) { scratch[0] = 0; scratch[1] = ~0u; }   // ([1]: the claim that is handed over, SkmSlotFeed)
    // the 2k-bit mask and where the last base of a k-mer sits, as 32-bit halves (15 <= k <= 32)
    const u32 kml = (u32)kh_mask(2 * k), kmh = (u32)(kh_mask(2 * k) >> 32);
    const u32 fsh = 64u - 2u * (u32)k;          // right-aligns a reversed window
    const u32 tsh = 2u * (u32)k - 2u;           // 28 .. 62
    const bool tsh_high = tsh >= 32u;           // (uniform) the last base of a k-mer sits in the high word
    const u32 tsh_sub = tsh_high ? tsh - 32u : tsh;
    // one distinct k-mer: popcount of its mask per group -> the group's bin; number of groups -> across bin
    // (returns true when the k-mer sits in exactly one group — nearly all do: those are counted per wave)
    // THE CREATOR'S OWN GROUP stands outside the loop.  Whoever created an entry ORed the mask of its own record into
    // it, so the group of that record's genome (`own`, its operand number) is one of the mask's groups, and in which
    // order the groups of a mask are counted makes no difference to the bins.  Its table entry `g` does not depend on
    // the mask: the read-out fetches it together with the exchanges, one LDS round trip instead of two in a row.
    // Nearly every k-mer sits in one group, and then no lane of the wave has bits outside that group's mask: one
    // wave-uniform test, and the strip and the loop are not executed at all.  Otherwise the own group and the own bit
    // are stripped (a tag outside every group has an empty group mask: its bit goes here, as the lowest bit does in
    // the loop, which therefore ends) and the remaining groups are taken from the lowest bit up.
    auto eval_mask = [&](u32 mlo, u32 mhi, const uint4 g, const u32 own) -> bool {
        const u32 bsh = sshift + 2u;   // a bin's stripe in bytes
        u8* const hlane = reinterpret_cast<u8*>(hstripe) + ((lane & smask) << 2);   // the lane's word of every stripe
        auto count_group = [&](const uint4 gg) {
            u32 c = (u32)__popc(mlo & gg.x) + (u32)__popc(mhi & gg.y);
            c = c < cs ? c : cs;
            atomicAdd(reinterpret_cast<u32*>(hlane + (gg.z + (c << bsh))), 1u);
        };
        count_group(g);
        if (!__builtin_amdgcn_ballot_w64(((mlo & ~g.x) | (mhi & ~g.y)) != 0u)) return true;   // (uniform) no lane has a second group
        const u32 ob = 1u << (own & 31u);
        mlo &= ~(g.x | (own < 32u ? ob : 0u));
        mhi &= ~(g.y | (own < 32u ? 0u : ob));
        u32 ng = 1;
        while (mlo | mhi) {
            const uint4 g2 = gtab[mlo ? (u32)__builtin_ctz(mlo) : 32u + (u32)__builtin_ctz(mhi)];
            count_group(g2);
            const u32 keep_hi = mlo ? ~0u : mhi - 1u;   // (the lowest bit goes in any case: a tag outside every group cannot hang the loop)
            mlo &= ~g2.x & (mlo - 1u);
            mhi &= ~g2.y & keep_hi;
            ++ng;
        }
        if (ng == 1u) return true;
        atomicAdd(&hstripe[((jb.abase + (ng < cs ? ng : cs)) << sshift) + (lane & smask)], 1u);
        return false;
    };
    u32 st_full = 0, st_exp = 0;   // fullest slot seen, k-mer instances expanded (uniform)
    // ---- the read-out: every thread turns the entries it created (13-bit fields of `made`, per pass) into histogram bins.
    // Invariant (the masks clean themselves): every non-zero mask has exactly one creator; it is read once, here, behind
    // the barrier after the insertion, and the read stores zero — so both planes of both tables are zero when
    // the next insertion phase (next subset, next slot) begins; this holds word for word for the second table's
    // entries, joint indices T .. T + T2 - 1 of the same planes.  A mask is only ever ORed into behind a
    // compare-and-swap that found its key or created it, and whoever created it recorded the place in `made`:
    // in the probe rounds (`mk`) or one key per lane (`where`, either table).  A key dropped under
    // KH_ERR_CAPACITY touched no mask; a slot handed on inserts nothing (C = 0); with R > 1 each subset's
    // read-out zeroes what that subset created before the barrier that precedes the next one.
    // The read-out of a lean slot s runs between barriers 1 and 2 of slot s + 1: behind
    // B4(s), which ends the insertions of s, and before B3(s + 1), which the insertions of s + 1 follow.  In that
    // interval nobody else touches the mask planes, gtab or hstripe (the merge works on the key plane, rmask, owner and
    // scratch[0]); dupc is added to from both sides, and additions commute.
    auto read_out = [&](u32 (&made)[SKM_PASSES][E / 2]) __attribute__((always_inline)) {
        u32 ones = 0;   // keys that sit in exactly one group, of the whole wave (uniform: a scalar register)
#pragma unroll
        for (u32 pass = 0; pass < SKM_PASSES; ++pass) {
            u32 any = 0;
#pragma unroll
            for (int e = 0; e < E / 2; ++e) any |= made[pass][e] & MADE_FIELDS;
            if (!__builtin_amdgcn_ballot_w64(any != 0)) continue;
            const u32 own = made[pass][0] >> MADE_OWN_SHIFT;   // the genome of the pass's record (0 where the thread had none)
            const uint4 g = gtab[own];                         // (issued ahead of the exchanges, which it does not depend on)
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const u32 f = (made[pass][e >> 1] >> (MADE_FIELD_BITS * (e & 1))) & MADE_FIELD;
                bool one = false;
                if (f) {   // the joint index + 1: either table
                    const u32 mlo = atomicExch(tmlo + f - 1u, 0u);
                    const u32 mhi = atomicExch(tmhi + f - 1u, 0u);
                    // (opaque copies made behind the exchanges: left to itself the compiler works on `g` ahead of them, for
                    // both entries at once, and waits for it there: two round trips in a row again)
                    uint4 ge = g;
                    u32 owne = own;
                    asm volatile("" : "+v"(ge.x), "+v"(ge.y), "+v"(ge.z), "+v"(owne));
                    one = eval_mask(mlo, mhi, ge, owne);
                }
                ones += (u32)__builtin_popcountll(__builtin_amdgcn_ballot_w64(one));
            }
        }
        if (ones && lane == 0) atomicAdd(&hstripe[(jb.abase + 1u) << sshift], ones);
        SKM_MARK("readout_done");
    };
    // what a lean slot's insertion leaves for the read-out behind the next barrier 1 (all zero: nothing)
    // (zeroed here by a loop in place and again behind every deferred read-out: one shared lambda, or `= {}` here,
    // moves the register allocation of the whole kernel)
    u32 made_d[SKM_PASSES][E / 2];
#pragma unroll
    for (u32 ps = 0; ps < SKM_PASSES; ++ps)
#pragma unroll
        for (int e = 0; e < E / 2; ++e) made_d[ps][e] = 0u;
    auto read_out_deferred = [&]() __attribute__((always_inline)) {
        read_out(made_d);
#pragma unroll
        for (u32 ps = 0; ps < SKM_PASSES; ++ps)
#pragma unroll
            for (int e = 0; e < E / 2; ++e) made_d[ps][e] = 0u;
    };
    // ---- pipeline prologue: this slot's record, the next slot's count
    SkmSlotFeed feed(gridDim.x, nslots, first_claimed);
    u32 slot = blockIdx.x, slot_next = slot + gridDim.x;
    u32 nrec = count_of(slot);
    u32 nrec_next = count_of(slot_next);
    uint4 rr = tid < nrec ? (jb.reg2 + (u64)slot * cap2)[tid] : make_uint4(0, 0, 0, 0);
    SKM_WGSTAMP(0);
    [[maybe_unused]] u32 walk_seq = 0;   // (stamp build)
    while (slot < nslots) {
        // (the thread number through an opaque copy, per slot: the many LDS addresses formed from it are worked out
        // where they are used instead of being kept in registers — and spilled — across the whole loop)
        tid = tid0;
        asm volatile("" : "+v"(tid));
        lane = tid & (KH_WAVE - 1u);
        const uint4* __restrict__ reg = jb.reg2 + (u64)slot * cap2;
        if (!nrec && counts[slot] > fit) {   // uniform: an overfull slot
            if (tid0 == 0) {
                const u32 at = atomicAdd(jb.ctl + KH_SKM_CTL_LISTED, 1u);
                if (at < jb.big_cap) jb.big_list[at] = slot;
            }
        }
        // ---- stage this slot's records, one per thread (behind the previous slot's barrier 4: the key plane, rmask,
        // owner and scratch[0] had their last readers in its insertions; its read-out, wherever it runs, reads none of them)
        u32 nj = 0;   // k-mers of this thread's record while it is alive
        const u32 tg = SkmRec1::tag(rr.w);
        const u32 rx = rr.x, ry = rr.y, rz = rr.z, rw = rr.w;   // (this slot's record; `rr` is loaded again below)
        {
            u32 z = 0;   // (opaque: a zero kept in four registers across the loop was spilled)
            asm volatile("" : "+v"(z));
            for (u32 i = tid; i < T / 4; i += NT) reinterpret_cast<uint4*>(dd)[i] = make_uint4(z, z, z, z);
        }
        if (tid < nrec) {
            nj = SkmRec1::n(rr.w);
            stage[tid] = rr;
            rmask[tid] = 1u << (tg & 31u);
        }
        SKM_USTAMP(0);
        SKM_USTAMP_WALK(walk_seq++);
        __syncthreads();
        SKM_USTAMP(1);
        // the slot after the next one (a claim drawn during the previous slot has arrived in LDS) and its count:
        // a scalar load, two slots ahead
        const u32 slot_after = feed.take(scratch + 1);
        const u32 nrec_after = count_of(slot_after);
        const bool draw = feed.wants();   // (uniform)
        SKM_MARK("dedup");
        // ---- identical records meet: the first keeps its place, the others add their genome bit to its mask.  A
        // record that stays takes its chunks from a counter (chunks in the low half, k-mers in the high half) and
        // enters them into the chunk table at once: no block scan, no phase of its own.
        if (__builtin_amdgcn_ballot_w64(nj != 0)) {   // (waves without records go straight to the barrier)
            __builtin_amdgcn_s_setprio(1);   // (the one priority raise: see above the kernel)
            u32 h = rx * 0x9E3779B1u ^ ry * 0x85EBCA77u ^ rz * 0xC2B2AE3Du ^ SkmRec1::content_hash_word(rw) * 0x27D4EB2Fu;
            h ^= h >> 15;
            h *= 0x2C1B3C6Du;
            u32 hp = (u32)(((u64)h * T) >> 32);
            const u32 nch = (nj + (u32)E - 1u) / (u32)E;
            bool pend = nj != 0, won = false;
            u32 mold = ~0u;   // the record this one is a copy of (a record merges at most once: it leaves the loop)
            while (__builtin_amdgcn_ballot_w64(pend)) {
                if (pend) {
                    const u32 old = atomicCAS(&dd[hp], 0u, tid + 1u);
                    if (old == 0u) {   // the first record with this content
                        won = true;
                        pend = false;
                    } else {
                        uint4 o = stage[old - 1u];   // (one 16-byte read: the opaque copy keeps the compiler from splitting it by use)
                        asm volatile("" : "+v"(o.x), "+v"(o.y), "+v"(o.z), "+v"(o.w));
                        // the same bases, the same number of k-mers, a genome of the same half of the mask: no branch per word
                        if (((o.x ^ rx) | (o.y ^ ry) | (o.z ^ rz) | SkmRec1::content_diff(o.w, rw)) == 0u) {
                            mold = old - 1u;
                            pend = false;
                        } else {
                            hp = (hp + 1u) & (T - 1u);
                        }
                    }
                }
            }
            // A copy adds its genome's bit to the mask of the record that stays: issued once, behind the loop (inside it,
            // every iteration of the wave waited for the answer), and the answer is looked at behind the chunk
            // numbering.  The loop is two dependent LDS round trips per iteration: the compare-and-swap, the 16-byte read.
            const u32 bit = 1u << (tg & 31u);
            u32 was = 0;
            if (mold != ~0u) was = atomicOr(&rmask[mold], bit);
            // the wave's records take consecutive chunks in lane order (their loads in the expansion stay
            // coalesced); the wave's share comes from one returning LDS atomic
            const u32 mine = won ? (nch | (nj << 16)) : 0u;
            const u32 incl = wave_scan_add(mine);
            u32 wbase = 0;
            if (lane == KH_WAVE - 1 && incl) wbase = atomicAdd(&scratch[0], incl);
            wbase = (u32)__builtin_amdgcn_readlane((int)wbase, KH_WAVE - 1);
            if (won) {
                const u32 cstart = (wbase + incl - mine) & 0xffffu;
                if (cstart + nch <= G::MAXCH) {
#pragma unroll
                    for (u32 cc = 0; cc < (1u << SKM_OB); ++cc)
                        if (cc < nch) owner[cstart + cc] = (u16)((tid << SKM_OB) | cc);
                }
            }
            // The OR's answer, behind the chunk numbering.  Safe to look at this late: only winners are entered in `dd`,
            // so every OR goes to a winner's rmask word and nobody touches the word of a record that lost; the store
            // below has one reader, the hand-over path behind barrier 2.
            if (was & bit) {   // a second copy inside one genome: nj repeats
                atomicAdd(&dupc[tg], nj);
                rmask[tid] = 0u;   // (this record's own mask is unused: zero = "has counted repeats", should the slot be handed on below)
            }
            __builtin_amdgcn_s_setprio(0);
        }
        SKM_MARK("dedup_end");
        // ---- the previous slot's read-out (lean slots): in this barrier interval with the merge above, which a wave
        // with both jobs has done first
        read_out_deferred();
        SKM_USTAMP(7);
        SKM_USTAMP(2);
        __syncthreads();   // barrier 2: the staged records and the set of contents are dead, the previous slot's masks are read and zero: the table is made
        SKM_USTAMP(10);
        const u32 sc0 = scratch[0];   // chunks | k-mers << 16 of the merged records (reset behind the next barrier)
        if ((sc0 & 0xffffu) > G::MAXCH) {   // uniform, rare: the slot is handed to k_skm_big below; what the merge has counted is taken back
            if (tid < nrec && rmask[tid] == 0u) {
                const u32 w = stage[tid].w;
                atomicSub(&dupc[SkmRec1::tag(w)], SkmRec1::n(w));
            }
            __syncthreads();
        }
        // ---- the next slot's record sets out now, into the registers this slot's record has just left: it has the
        // expansion and the read-out to arrive
        rr = tid < nrec_next ? (jb.reg2 + (u64)slot_next * cap2)[tid] : make_uint4(0, 0, 0, 0);
        clear_keys();
        u32 C = sc0 & 0xffffu, N = sc0 >> 16;
        SKM_USTAMP(3);
        SKM_MARK("after_scan");
        st_full = N > st_full ? N : st_full;
        st_exp += N;
        if (C > G::MAXCH) {   // uniform: more chunks than are numbered here (long runs of one minimizer): k_skm_big takes the slot
            if (tid == 0) {
                if (jb.big_list) {
                    const u32 at = atomicAdd(jb.ctl + KH_SKM_CTL_LISTED, 1u);
                    if (at < jb.big_cap) jb.big_list[at] = slot;
                } else atomicOr(jb.ctl, KH_ERR_CAPACITY);
            }
            C = 0;
            N = 0;
        }
        __syncthreads();
        if (tid == 0) scratch[0] = 0;   // (everybody has read it; it is added to again behind the next slot's first barrier)
        SKM_MARK("owner_done");
        SKM_USTAMP(4);
        const u32 R0 = (N + T - 1) / T;   // key subsets handled one after the other (1 unless the slot is overfull)
        // ---- the slot behind the third barrier.  MULTI false: one subset, known at compile time (R is the literal 1:
        // the subset loop, the filter, the clears and the barrier between subsets fold away); true: R0 subsets.
        auto slot_body = [&](auto multi_) __attribute__((always_inline)) {
            constexpr bool MULTI = decltype(multi_)::value;
            const u32 R = MULTI ? R0 : 1u;
            // the thread's chunk in pass 0; in pass p: c0 + p * NT.  (Read here, before the subset loop: with `tid` read
            // inside the pass loop the multi body's chunk addresses are scheduled in another order.  A rotated numbering
            // of the waves — other SIMDs busy from slot to slot — changed nothing.)
            const u32 c0 = tid;
            for (u32 q = 0; q < R; ++q) {
                if (q) { clear_keys(); __syncthreads(); }
                unsigned long long emptyv = EMPTY;   // (opaque: made here, or the compiler keeps the constant in two VGPRs across the loop and spills it)
                asm volatile("" : "+v"(emptyv));
                // entries this thread created, per pass: two fields and the record's genome (the layout is at the table planes)
                u32 made[SKM_PASSES][E / 2];
#pragma unroll
                for (u32 ps = 0; ps < SKM_PASSES; ++ps)
#pragma unroll
                    for (int e = 0; e < E / 2; ++e) made[ps][e] = 0u;
#pragma unroll
                for (u32 pass = 0; pass < SKM_PASSES; ++pass) {
                    if (pass * NT >= C) break;   // uniform
                    const u32 c = pass * NT + c0;
                    u64 kreg[E];
                    u32 slot_[E], act = 0, bits = 0, half = 0, own = 0;
#pragma unroll
                    for (int e = 0; e < E; ++e) { kreg[e] = EMPTY; slot_[e] = 0; }
                    if (c < C) {
                        const u32 o = owner[c], ri = o >> SKM_OB, first = (o & ((1u << SKM_OB) - 1u)) * (u32)E;
                        // (an L2 hit: the records were read a moment ago.  Issued before the table clears instead, for the first
                        // pass, it made the kernel slower: 1.430 -> 1.486 ms, same registers, three alternated runs each)
                        const uint4 r0 = reg[ri];
                        bits = rmask[ri];
                        half = SkmRec1::half(r0.w);
                        own = SkmRec1::tag(r0.w);   // (its bit is in `bits`: the record that stays keeps its own)
                        const u32 left = SkmRec1::n(r0.w) - first;
                        const u32 cnt = left < (u32)E ? left : (u32)E;
                        // The twin of skm1_expand<E> above, kept in place: through the shared expander (hash, kreg, slot_ and act
                        // in a callback) registers, scratch and occupancy stay as they are, but the probe rounds behind it are
                        // structured with 7 % more instructions (s_and_saveexec / s_or / s_cbranch_execz / v_mov).  A change
                        // of the expansion has to be made in both.
                        const u64 clo = ((u64)r0.y << 32) | r0.x, chi = ((u64)r0.w << 32) | r0.z;
                        const u32 sh = 2u * first;   // 0, 2E, .. <= 60
                        const u64 lo = sh ? (clo >> sh) | (chi << (64u - sh)) : clo, hi = chi >> sh;
                        const u32 xl = (u32)lo & kml, xh = (u32)(lo >> 32) & kmh;   // the first k-mer, base j at bits 2j
                        const u64 fw = kh_revpairs64(((u64)xh << 32) | xl) >> fsh;
                        u32 fl = (u32)fw, fh = (u32)(fw >> 32), rl = ~xl & kml, rh = ~xh & kmh;
                        const u32 t = (u32)((lo >> tsh) | (hi << (64u - tsh)));   // bits 2e: the last base of the chunk's k-mer e
                        const u32 tc = ~t;
#pragma unroll
                        for (int e = 0; e < E; ++e) {
                            if (e) {   // roll both strands by one base
                                fh = __builtin_amdgcn_alignbit(fh, fl, 30) & kmh;
                                fl = ((fl << 2) | ((t >> (2 * e)) & 3u)) & kml;
                                rl = __builtin_amdgcn_alignbit(rh, rl, 2);
                                rh >>= 2;
                                if (tsh_high) rh |= ((tc >> (2 * e)) & 3u) << tsh_sub; else rl |= ((tc >> (2 * e)) & 3u) << tsh_sub;
                            }
                            const bool fwd = fh < rh || (fh == rh && fl < rl);
                            const u32 cl = fwd ? fl : rl, ch = fwd ? fh : rh;
                            const u32 h = key_hash2(cl, ch);
                            kreg[e] = ((u64)ch << 32) | cl;
                            slot_[e] = (u32)(((u64)h * T) >> 32);
                            if (R != 1 && (u32)e < cnt && (((h >> 4) & 0xffffu) * R) >> 16 == q) act |= 1u << e;
                        }
                        if (R == 1) act = (1u << cnt) - 1u;
                    }
                    SKM_MARK("expanded");
                    if (!__builtin_amdgcn_ballot_w64(act != 0)) continue;   // a wave without a chunk
                    u32* const mp = half ? tmhi : tmlo;
                    // ---- probe rounds, all of a thread's keys per round (one dependent LDS round trip per round)
                    u32 was[E];   // the mask half as it was: bits of this record's genomes set already = repeats inside those genomes
#pragma unroll
                    for (int e = 0; e < E; ++e) was[e] = 0u;
                    u32 mk = 0;   // keys whose compare-and-swap created the entry
                    // one probe round, all of a thread's keys
                    auto probe_round = [&]() __attribute__((always_inline)) {
                        unsigned long long old[E];
#pragma unroll
                        for (int e = 0; e < E; ++e)
                            old[e] = (act & (1u << e)) ? atomicCAS(&tkey[slot_[e]], emptyv, (unsigned long long)kreg[e]) : 0ull;
#pragma unroll
                        for (int e = 0; e < E; ++e) {
                            if (act & (1u << e)) {
                                const bool fresh = old[e] == emptyv;
                                if (fresh || old[e] == kreg[e]) {
                                    was[e] = atomicOr(mp + slot_[e], bits);   // looked at after the last round
                                    act &= ~(1u << e);
                                    if (fresh) mk |= 1u << e;
                                } else {
                                    slot_[e] = (slot_[e] + 1u) & (T - 1u);
                                }
                            }
                        }
                    };
                    u32 f16[E];   // where each key's entry is, if this thread created it
                    auto chain_home = [&](const u32 H) __attribute__((always_inline)) -> u32 { return ((H ^ (H >> 15)) * 0x85EBCA77u) >> T2SH; };
                    // One key per lane through the tiers, from entry S of the second table on; -> where the lane created an
                    // entry.  Level 1: second table, 2: main table, unbounded.  The lane counts the repeats it meets.
                    auto tier_walk = [&](const unsigned long long K, const u32 H, const u32 kbits, const u32 khalf,
                                         u32 S, bool mine) __attribute__((always_inline)) -> u32 {
                        u32 probes = 0;   // at the current level
                        u32* const kmp = khalf ? tmhi : tmlo;
                        u32 level = 1u, where = 0;
                        while (__builtin_amdgcn_ballot_w64(mine)) {
                            if (mine) {
                                unsigned long long* kp = level == 1 ? okey : tkey;
                                const unsigned long long o2 = atomicCAS(&kp[S], emptyv, K);
                                if (o2 == emptyv || o2 == K) {
                                    u32* mp2 = level == 1 ? (khalf ? omhi : omlo) : kmp;
                                    u32 d = atomicOr(mp2 + S, kbits) & kbits;
                                    while (d) { atomicAdd(&dupc[khalf * 32u + (u32)__builtin_ctz(d)], 1u); d &= d - 1u; }
                                    if (o2 == emptyv) where = (level == 1 ? T : 0u) + S + 1u;
                                    mine = false;
                                } else {
                                    ++probes;
                                    if (level == 1 && probes >= 8u) {   // a crowded second table: on in the main one
                                        level = 2; probes = 0;
                                        S = (u32)(((u64)H * T) >> 32) + (u32)KH_TUNE_SKM_FULL_ROUNDS;
                                        S = S & (T - 1u);
                                    } else if (level == 2 && probes >= T) {
                                        // The main table is full.  With R > 1 the key subsets are picked by hash bits, not by
                                        // count: a skewed slot (up to SKM_PASSES x NT chunks) can put more than T + T2
                                        // distinct keys into one subset.  The key is dropped here; the host sees the error,
                                        // counts a retry and hands the whole call to the key-array form.
                                        atomicOr(jb.ctl, KH_ERR_CAPACITY);
                                        mine = false;
                                    } else {
                                        S = level == 1 ? ((S + 1u) & (T2 - 1u)) : ((S + 1u) & (T - 1u));
                                    }
                                }
                            }
                        }
                        return where;
                    };
                    // the few keys still homeless: one per lane at a time, second table, then the main one again
                    auto serial_finish = [&]() __attribute__((always_inline)) {
                        while (__builtin_amdgcn_ballot_w64(act != 0)) {
                            const bool have_one = act != 0;
                            const u32 es = have_one ? (u32)__builtin_ctz(act) : 0u;
                            u64 K = 0;
#pragma unroll
                            for (int e = 0; e < E; ++e)
                                if (es == (u32)e) K = kreg[e];
                            const u32 H = key_hash2((u32)K, (u32)(K >> 32));
                            const u32 where = tier_walk((unsigned long long)K, H, bits, half, chain_home(H), have_one);
                            if (have_one) {
                                act &= ~(1u << es);
#pragma unroll
                                for (int e = 0; e < E; ++e)
                                    if (es == (u32)e) f16[e] = where;
                            }
                        }
                    };
                    for (u32 round = 0; round < (u32)KH_TUNE_SKM_FULL_ROUNDS && __builtin_amdgcn_ballot_w64(act != 0); ++round) probe_round();
                    SKM_USTAMP(9);
                    SKM_MARK("rounds_done");
#pragma unroll
                    for (int e = 0; e < E; ++e) f16[e] = (mk >> e) & 1u ? slot_[e] + 1u : 0u;
                    serial_finish();
                    SKM_MARK("serial_done");
#pragma unroll
                    for (int e = 0; e < E / 2; ++e) made[pass][e] = f16[2 * e] | (f16[2 * e + 1] << MADE_FIELD_BITS) | (own << MADE_OWN_SHIFT);
                    {   // repeats inside a genome: the bit was set before this instance came
                        u32 d = 0;
#pragma unroll
                        for (int e = 0; e < E; ++e) d |= was[e] & bits;
                        if (d) {
#pragma unroll
                            for (int e = 0; e < E; ++e) {
                                u32 de = was[e] & bits;
                                while (de) { atomicAdd(&dupc[half * 32u + (u32)__builtin_ctz(de)], 1u); de &= de - 1u; }
                            }
                        }
                    }
                }
                SKM_MARK("insert_done");
                SKM_USTAMP(5);
                // the next claim: one lane of the wave that runs out of chunks first (the last one); the barrier below and the
                // next slot's first one lie between this store and the threads that read it
                if (draw && q == 0 && tid0 == (NW - 1u) * KH_WAVE) feed.draw(jb.claim, scratch + 1);
                __syncthreads();   // barrier 4: the insertions are over, the KEY plane is dead, all masks are final
                SKM_USTAMP(6);
                if (!MULTI) {
                    // the read-out waits for the next slot's barrier 1 (`read_out`, above): what this thread created goes along
#pragma unroll
                    for (u32 ps = 0; ps < SKM_PASSES; ++ps)
#pragma unroll
                        for (int e = 0; e < E / 2; ++e) made_d[ps][e] = made[ps][e];
                } else {
                    read_out(made);
                    SKM_USTAMP(7);
                }
                if (q + 1 < R) __syncthreads();
            }
        };
        if (R0 == 1u) {
            slot_body(std::false_type{});
        } else if (__builtin_expect(R0 != 0u, 0)) {   // (uniform, cold)
            if (R0 > 1u && tid0 == 0) atomicAdd(jb.ctl + KH_SKM_CTL_MULTI, 1u);   // slots taken in more than one subset
            slot_body(std::true_type{});
        }
        SKM_USTAMP(8);
        if (draw && R0 == 0 && tid0 == (NW - 1u) * KH_WAVE) feed.draw(jb.claim, scratch + 1);   // (an empty slot: nothing was inserted)
        // ---- on to the next slot: its record has arrived in the meantime (it set out behind barrier 2 and had the
        // key clear, the insertion and barrier 4 to arrive; the next load is issued where `rr` is free again, behind the
        // next barrier 2).  No barrier here: what the next slot writes before its first barrier (staged records, the
        // set of contents: the KEY plane, whose last readers were the insertions that barrier 4 ended — with R > 1 the
        // last subset's barrier 4; this thread's record mask, read by those insertions too) is read by nobody in a
        // read-out, whether that ran in place (multi) or runs behind the next barrier 1 (lean).
        nrec = nrec_next;
        nrec_next = nrec_after;
        slot = slot_next;
        slot_next = slot_after;
    }
    read_out_deferred();   // the walk's last lean slot (a workgroup without slots: nothing)
    SKM_WGSTAMP(8);
    __syncthreads();
    tid = tid0;
    lane = tid & (KH_WAVE - 1u);
    unsigned long long* __restrict__ rep = jb.hist + (u64)(blockIdx.x % jb.reps) * nbins;
    for (u32 i = tid; i < nbins; i += NT) {
        u32 v = 0;
        for (u32 j = 0; j <= smask; ++j) v += hstripe[(i << sshift) + j];
        if (v) atomicAdd(&rep[i], (unsigned long long)v);
    }
    if (tid < (u32)KH_TAG_MAX_OPS && dupc[tid]) atomicAdd(&jb.dup[tid], (unsigned long long)dupc[tid]);
    if (tid == 0) {
        if (st_full > T) atomicMax(jb.ctl + KH_SKM_CTL_FULLEST, st_full);
        atomicAdd(jb.ctl + KH_SKM_CTL_EXPANDED, st_exp);   // k-mer instances that were expanded
    }
}

// ------------------------------------------------------------------------------------------
// Overfull slots: k_skm_big (kh_skm_device.h) with one-word keys
// ------------------------------------------------------------------------------------------
constexpr u32 SKM_BIG_T = 4096, SKM_BIG_T2 = 128;
struct SkmBig1 {
    using Rec = SkmRec1;
    using Consts = Skm1Consts;
    using Key = unsigned long long;
    static constexpr u32 T = SKM_BIG_T, T2 = SKM_BIG_T2, KEY_BYTES = 8, BATCH = 256, OB = SKM_OB;
    static constexpr int E = (int)SKM_UE;
    template <class F> static __device__ __forceinline__ void expand(const SkmRecord<1>& r, const u32 first, const Consts& kc, F&& f) {
        skm1_expand<E>(r.v[0], first, kc, [&](const u32 e, const u32 cl, const u32 ch) __attribute__((always_inline)) { f(e, ((u64)ch << 32) | cl); });
    }
    static __device__ __forceinline__ u32 hash(const Key K) { return key_hash2((u32)K, (u32)(K >> 32)); }
    static __device__ __forceinline__ SkmClaim1 claim(u8* kmain, const u32 okey_off, const Key K) {
        return SkmClaim1{reinterpret_cast<unsigned long long*>(kmain), okey_off, ~0ull, K};
    }
};
static_assert(skm_big_lds_bytes<SkmBig1>() == 94720, "k_skm_big<SkmBig1>: the walk's LDS with 288 stripe words and the side-list index");
static_assert(skm_cross_lds_bytes<SkmBig1>(false) == 81280 && skm_cross_lds_bytes<SkmBig1>(true) == 97664, "k_skm_cross<SkmBig1>: direct and listed launch");

// ------------------------------------------------------------------------------------------
// The exchange form (multi-GPU step 7-8): slots are a GLOBAL function of the minimizer, so ranks
// exchange RECORDS by slot range instead of key sets.
//
//   k_skm_pack     one workgroup per slot of this rank's records (tag = local group, < 32): identical records of a
//                  group are the same piece of sequence in several of its genomes — only one travels; identical
//                  records of different groups merge into one with a mask of groups.  The survivors go, with their
//                  32-bit masks, to the record array of the rank that owns the slot (one returning global atomic
//                  per slot); per slot: how many, and where.
//   k_skm_phased   persistent, one slot at a time: the pieces (one per source rank) are PHASES.  A phase expands
//                  its records and ORs their masks into the table's low mask plane; between phases every entry
//                  folds popcount(mask) into its counter (the high plane) and clears the mask: tags of different
//                  phases are different groups, so the counter ends as "in how many groups of all ranks".
// ------------------------------------------------------------------------------------------
// (NT threads = the most records a slot may hold: the host picks 256 / 512 / 1024 from the regions' capacity — a
// workgroup per slot costs ~5 us whatever it holds, and four or eight of the small ones fit a CU instead of two)
static size_t skm_pack_lds_bytes(u32 nt) { return (size_t)nt * 16 + (size_t)nt * 4 * 4 + (size_t)nt * 4 + 64; }

template <u32 NT>
__global__ __launch_bounds__(NT) void k_skm_pack(const KhSkmPackJob jb) {
    extern __shared__ __attribute__((aligned(16))) u8 lds_raw[];
    constexpr u32 T = 4 * NT, TSH = NT == 1024 ? 20u : (NT == 512 ? 21u : 22u);
    static_assert(NT == 1024 || NT == 512 || NT == 256, "table of 4 NT entries, a power of two");
    uint4* stage = reinterpret_cast<uint4*>(lds_raw);
    u32* dd = reinterpret_cast<u32*>(lds_raw + (size_t)NT * 16);
    u32* rmask = dd + T;
    u32* scratch = rmask + NT;
    const u32 tid = threadIdx.x, lane = lane_id();
    const u32 slot = blockIdx.x;
    u32 nrec = jb.cur2[slot];
    nrec = nrec < jb.cap2 ? nrec : jb.cap2;
    if (nrec > NT) {   // (the host sizes the slots so that this does not happen)
        if (tid == 0) atomicOr(jb.ctl, KH_ERR_CAPACITY);
        nrec = NT;
    }
    const uint4 rr = tid < nrec ? (jb.reg2 + (u64)slot * jb.cap2)[tid] : make_uint4(0, 0, 0, 0);
    reinterpret_cast<uint4*>(dd)[tid] = make_uint4(0u, 0u, 0u, 0u);
    if (tid == 0) { scratch[0] = 0; scratch[1] = 0; }
    const u32 tg = SkmRec1::tag(rr.w);
    u32 nj = 0;
    if (tid < nrec) {
        nj = SkmRec1::n(rr.w);
        stage[tid] = rr;
        rmask[tid] = 1u << (tg & 31u);
        if (tg >= 32u) atomicOr(jb.ctl, KH_ERR_ORDER);   // tags of the exchange form are below 32
    }
    __syncthreads();
    bool won = false;
    if (__builtin_amdgcn_ballot_w64(nj != 0)) {
        u32 h = rr.x * 0x9E3779B1u ^ rr.y * 0x85EBCA77u ^ rr.z * 0xC2B2AE3Du ^ SkmRec1::content_hash_word(rr.w) * 0x27D4EB2Fu;
        h ^= h >> 15;
        h *= 0x2C1B3C6Du;
        u32 hp = h >> TSH;
        bool pend = nj != 0;
        while (__builtin_amdgcn_ballot_w64(pend)) {
            if (pend) {
                const u32 old = atomicCAS(&dd[hp], 0u, tid + 1u);
                if (old == 0u) { won = true; pend = false; }
                else {
                    const uint4 o = stage[old - 1u];
                    if (o.x == rr.x && o.y == rr.y && o.z == rr.z && SkmRec1::same_content(o.w, rr.w)) {
                        const u32 bit = 1u << (tg & 31u);
                        const u32 was = atomicOr(&rmask[old - 1u], bit);
                        if ((was & bit) && jb.dup) atomicAdd(&jb.dup[tg & 31u], (unsigned long long)nj);   // a second copy under one tag
                        pend = false;
                    } else hp = (hp + 1u) & (T - 1u);
                }
            }
        }
    }
    // ---- the survivors, in thread order, to the array of the rank that owns the slot
    const u32 incl = wave_scan_add(won ? 1u : 0u);
    u32 wbase = 0;
    if (lane == KH_WAVE - 1 && incl) wbase = atomicAdd(&scratch[0], incl);
    wbase = (u32)__builtin_amdgcn_readlane((int)wbase, KH_WAVE - 1);
    __syncthreads();   // all masks are final, the slot's total is known
    const u32 nsurv = scratch[0];
    const u32 part = slot / jb.spp;
    if (tid == 0) {
        const u32 sub = slot % jb.nsub;
        const u64 subcap = jb.part_cap / jb.nsub;
        u32 base = nsurv ? atomicAdd(&jb.part_cursor[part * jb.nsub + sub], nsurv) : 0u;
        if ((u64)base + nsurv > subcap) { atomicOr(jb.ctl, KH_ERR_CAPACITY); base = 0; scratch[0] = 0; }
        base += (u32)(sub * subcap);
        scratch[1] = base;
        jb.slot_count[slot] = nsurv;
        jb.slot_off[slot] = base;
    }
    __syncthreads();
    if (won && scratch[0]) {
        const u64 at = (u64)scratch[1] + wbase + incl - 1u;
        if (at < jb.part_cap) {
            jb.out_rec[(u64)part * jb.part_cap + at] = rr;
            jb.out_mask[(u64)part * jb.part_cap + at] = rmask[tid];
        }
    }
}

// A part that was packed through 64 cursors (one returning atomic per slot on a single cursor is a queue: 78 K
// workgroups, 0.8 ms) is moved together: workgroup (sub-range, part) copies its records behind those of the sub-ranges
// before it and rewrites the offsets of its slots.
__global__ __launch_bounds__(256) void k_skm_pack_compact(const KhSkmCompactJob jb) {
    const u32 sub = blockIdx.x, part = blockIdx.y, tid = threadIdx.x;
    const u64 subcap = jb.part_cap / jb.nsub;
    // (a cursor that ran past its sub-range has counted a slot k_skm_pack refused — the host reports the overflow; the
    // clamp keeps the copy inside the part)
    auto used = [&](u32 q) { const u32 v = jb.cursors[part * jb.nsub + q]; return (u64)v < subcap ? v : (u32)subcap; };
    u32 before = 0, total = 0;
    for (u32 q = 0; q < jb.nsub; ++q) {   // uniform
        const u32 v = used(q);
        before += q < sub ? v : 0u;
        total += v;
    }
    const u32 n = used(sub);
    const u64 src = (u64)part * jb.part_cap + (u64)sub * subcap, dst = (u64)part * jb.part_cap + before;
    for (u32 i = tid + 256u * blockIdx.z; i < n; i += 256u * gridDim.z) {   // (z: slices of the copy)
        jb.out_rec[dst + i] = jb.tmp_rec[src + i];
        jb.out_mask[dst + i] = jb.tmp_mask[src + i];
    }
    if (blockIdx.z) return;
    const u32 s0 = part * jb.spp, s1 = s0 + jb.spp < jb.nslots ? s0 + jb.spp : jb.nslots;
    const u32 first = s0 + (sub + jb.nsub - s0 % jb.nsub) % jb.nsub;   // the part's first slot with slot % nsub == sub
    for (u32 slot = first + tid * jb.nsub; slot < s1; slot += 256u * jb.nsub)
        jb.slot_off[slot] = jb.slot_off[slot] - (u32)((u64)sub * subcap) + before;
    if (sub == 0 && tid == 0) jb.part_n[part] = total;
}

constexpr u32 SKM_PH_NT = 1024, SKM_PH_T = 4096, SKM_PH_T2 = 128, SKM_PH_MAXCH = 4096, SKM_PH_HBINS = 512;
// A phase holds a few dozen records and its time is the insertion's chain of LDS round trips (ablation: 64 % of the
// kernel): ONE k-mer per thread — twice the threads of the union's two-k-mer chunks, half the chain.
constexpr u32 SKM_PH_E = 1, SKM_PH_OB = 5;   // k-mers per chunk; a record has at most 1 << SKM_PH_OB chunks
constexpr u32 SKM_PH_ROUND = 3072;   // k-mer instances a round of the phased union takes (the table has 4096 entries)
constexpr u32 SKM_PH_STAGED = 32;    // pieces whose records of a slot are numbered in one go (more: a phase at a time)
size_t kh_skm_phased_lds_bytes() {
    return (size_t)SKM_PH_T * 16 + (size_t)SKM_PH_T2 * 16 + 128 + (size_t)SKM_PH_HBINS * 4 + (size_t)SKM_PH_MAXCH * 2 +
           (size_t)SKM_PH_NT * 2 + (size_t)SKM_PH_STAGED * (8 + 8 + 4 * 5) + 64;
}

// A slot's time is a chain of memory latencies, not work (a phase holds a few dozen records): the records of ALL
// pieces are numbered in one go — thread t takes record t of the concatenated pieces, one ordered block scan gives
// every phase its range of chunks — and the phases that follow only insert and fold (two barriers each).  The
// per-piece counts and offsets of the NEXT slot are loaded a slot ahead.  A slot with more than 1024 records or
// 3072 chunks over all pieces (or more than 32 pieces) is numbered a phase at a time instead.
__global__ __launch_bounds__(SKM_PH_NT, 8) void k_skm_phased(const KhSkmPhasedJob jb) {
    extern __shared__ __attribute__((aligned(16))) u8 lds_raw[];
    constexpr u32 NT = SKM_PH_NT, T = SKM_PH_T, T2 = SKM_PH_T2, NP = SKM_PH_STAGED;
    constexpr int E = (int)SKM_PH_E;
    constexpr u64 EMPTY = ~0ull;
    u8* p = lds_raw;
    unsigned long long* tkey = reinterpret_cast<unsigned long long*>(p);   p += (size_t)T * 8;
    u32* tmlo = reinterpret_cast<u32*>(p);                                 p += (size_t)T * 4;   // the running phase's mask
    u32* tcnt = reinterpret_cast<u32*>(p);                                 p += (size_t)T * 4;   // tags of the phases before it
    unsigned long long* okey = reinterpret_cast<unsigned long long*>(p);   p += (size_t)T2 * 8;
    u32* omlo = reinterpret_cast<u32*>(p);                                 p += (size_t)T2 * 4;
    u32* ocnt = reinterpret_cast<u32*>(p);                                 p += (size_t)T2 * 4;
    constexpr u32 OKEY_OFF = 2 * T, OMLO_OFF = 2 * T + 2 * T2;             // okey - tkey, omlo - tmlo (the probe walk addresses both tables from one base)
    u32* scratch = reinterpret_cast<u32*>(p);                              p += 128;   // [0] chunks of the phase, [1] entries made, [2] k-mers of the slot, [3] staged?, [8..23] wave totals
    u32* lhist = reinterpret_cast<u32*>(p);                                p += (size_t)SKM_PH_HBINS * 4;
    u16* owner = reinterpret_cast<u16*>(p);                                p += (size_t)SKM_PH_MAXCH * 2;
    u16* rloc = reinterpret_cast<u16*>(p);                                 p += (size_t)NT * 2;   // staged record t -> piece << 10 | record of the piece's slot
    const uint4** prec = reinterpret_cast<const uint4**>(p);               p += (size_t)NP * 8;   // the pieces' arrays (loaded once)
    const u32** pmsk = reinterpret_cast<const u32**>(p);                   p += (size_t)NP * 8;
    u32* pcnt = reinterpret_cast<u32*>(p);                                 p += (size_t)NP * 4;   // this slot: records per piece,
    u32* poff = reinterpret_cast<u32*>(p);                                 p += (size_t)NP * 4;   //   where they start,
    u32* cbeg = reinterpret_cast<u32*>(p);                                 p += (size_t)NP * 4;   //   the piece's chunks [cbeg, cend)
    u32* cend = reinterpret_cast<u32*>(p);                                 p += (size_t)NP * 4;
    u32* pflag = reinterpret_cast<u32*>(p);                                // dup_row << 1 | join_next
    const u32 tid0 = threadIdx.x;
    u32 tid = tid0, lane = lane_id();
    const Skm1Consts kc(jb.k);
    const u32 hbins = jb.hist_len < SKM_PH_HBINS ? jb.hist_len : SKM_PH_HBINS;   // counts below this: LDS; above: global atomics
    const bool want_dup = jb.dup != nullptr;
    const bool staged = jb.npieces <= NP;
    const u32 npieces = jb.npieces;
    typedef const u32 __attribute__((address_space(4))) * ConstU32;
    if (tid < SKM_PH_HBINS) lhist[tid] = 0;
    if (tid < 32) scratch[tid] = 0;
    const u32* my_count = nullptr;   // thread p < npieces: piece p's per-slot arrays
    const u32* my_off = nullptr;
    if (staged && tid < npieces) {
        const KhSkmPiece pc = jb.pieces[tid];
        prec[tid] = pc.rec;
        pmsk[tid] = pc.mask;
        pflag[tid] = (pc.dup_row << 1) | (pc.join_next & 1u);
        my_count = pc.count;
        my_off = pc.off;
    }
    u32 nxt_cnt = 0, nxt_off = 0;   // (thread p < npieces) piece p's records of the next slot
    if (my_count && blockIdx.x < jb.nslots) { nxt_cnt = my_count[blockIdx.x]; nxt_off = my_off[blockIdx.x]; }
    __syncthreads();
    unsigned long long emptyv = EMPTY;
    // ---- one chunk: E k-mers of record r0 from its k-mer `first` on, with the genomes / groups `bits`, enter the table
    auto insert_chunk = [&](const uint4 r0, const u32 bits, const u32 first, const u32 ph, const u32 R, const u32 q, u32& fresh_n) __attribute__((always_inline)) {
        const u32 cnt = SkmRec1::n(r0.w) - first;   // k-mers of the record from `first` on: the chunk holds min(cnt, E)
        skm1_expand<E>(r0, first, kc, [&](const u32 e, const u32 cl, const u32 ch) __attribute__((always_inline)) {
            if (e >= cnt) return;
            const unsigned long long K = ((u64)ch << 32) | cl;
            const u32 H = key_hash2(cl, ch);
            if (R != 1 && skm_round_of(H, R) != q) return;   // another round's key
            skm_probe_walk<T, T2>(H, jb.ctl, SkmClaim1{tkey, OKEY_OFF, emptyv, K}, [&](const bool second, const u32 S, const bool fresh) __attribute__((always_inline)) {
                u32* const mp = tmlo + (second ? OMLO_OFF : 0u) + S;
                if (want_dup) {   // uniform: bits set already = a second instance under that tag (rare: global counters)
                    u32 d = atomicOr(mp, bits) & bits;
                    while (d) { atomicAdd(&jb.dup[ph * 32u + (u32)__builtin_ctz(d)], 1ull); d &= d - 1u; }
                } else atomicOr(mp, bits);
                if (fresh) ++fresh_n;
            });
        });
    };
    // ---- behind a phase's insertions: its tags are counted, the mask plane is free for the next phase
    auto count_fresh = [&](const u32 fresh_n) {
        if (__builtin_amdgcn_ballot_w64(fresh_n != 0)) {
            const u32 tot = wave_scan_add(fresh_n);
            if (lane == KH_WAVE - 1) atomicAdd(&scratch[1], tot);
        }
    };
    auto fold_now = [&]() {
        __syncthreads();
        uint4 m4 = reinterpret_cast<uint4*>(tmlo)[tid];
        if (m4.x | m4.y | m4.z | m4.w) {
            uint4 c4 = reinterpret_cast<uint4*>(tcnt)[tid];
            c4.x += (u32)__popc(m4.x); c4.y += (u32)__popc(m4.y); c4.z += (u32)__popc(m4.z); c4.w += (u32)__popc(m4.w);
            reinterpret_cast<uint4*>(tcnt)[tid] = c4;
            reinterpret_cast<uint4*>(tmlo)[tid] = make_uint4(0u, 0u, 0u, 0u);
        }
        if (tid < T2) { const u32 m = omlo[tid]; if (m) { ocnt[tid] += (u32)__popc(m); omlo[tid] = 0u; } }
        if (tid == 0) {
            scratch[0] = 0;
            if (scratch[1] > T - T / 16) atomicOr(jb.ctl, KH_ERR_CAPACITY);   // nearly full: probing would crawl
        }
        __syncthreads();
    };
    for (u32 slot = blockIdx.x; slot < jb.nslots; slot += gridDim.x) {
        tid = tid0;
        asm volatile("" : "+v"(tid));   // (addresses formed from it are worked out where they are used)
        lane = tid & (KH_WAVE - 1u);
        asm volatile("" : "+v"(emptyv));
        // ---- the slot's records over all pieces, its k-mer instances (more than a table takes -> rounds of key subsets)
        bool all_staged = staged;   // uniform
        u32 my_nj = 0, my_nch = 0, my_cstart = 0, Ctot = 0;
        if (staged) {
            if (tid < npieces) {
                pcnt[tid] = nxt_cnt;
                poff[tid] = nxt_off;
                cbeg[tid] = 0;
                cend[tid] = 0;
                const u32 ns = slot + gridDim.x;
                nxt_cnt = 0;
                if (ns < jb.nslots) { nxt_cnt = my_count[ns]; nxt_off = my_off[ns]; }   // (arrives during this slot)
            }
            __syncthreads();
            u32 acc = 0, myph = NP, myidx = 0, mycnt = 0;
            for (u32 ph = 0; ph < npieces; ++ph) {
                const u32 cn = pcnt[ph];
                if (tid >= acc && tid - acc < cn) { myph = ph; myidx = tid - acc; mycnt = cn; }
                acc += cn;
            }
            if (acc > NT) {
                all_staged = false;
                if (tid == 0) atomicMax(jb.ctl + KH_SKM_XCTL_FULLEST, acc);
            } else {
                if (myph < NP) {
                    const u64 at = (u64)poff[myph] + myidx;
                    my_nj = SkmRec1::n(prec[myph][at].w);
                    const u32 touch = pmsk[myph][at];   // (the mask's cache line sets out now)
                    asm volatile("" ::"v"(touch));
                    rloc[tid] = (u16)((myph << 10) | myidx);
                }
                my_nch = (my_nj + (u32)E - 1u) / (u32)E;
                // ordered block scan of (chunks, instances): chunk numbers follow the record order, i.e. the phases
                const u32 both = my_nch | (my_nj << 16);
                const u32 incl = wave_scan_add(both);
                if (lane == KH_WAVE - 1) scratch[8 + (tid >> 6)] = incl;
                __syncthreads();
                u32 before = 0, total = 0;
#pragma unroll
                for (u32 w = 0; w < NT / KH_WAVE; ++w) {
                    const u32 v = scratch[8 + w];
                    if (w < (tid >> 6)) before += v;
                    total += v;
                }
                Ctot = total & 0xffffu;
                my_cstart = ((before + incl - both) & 0xffffu);
                if (tid == 0) scratch[2] = total >> 16;
                if (Ctot > SKM_PH_MAXCH) {
                    all_staged = false;
                } else if (myph < NP) {
#pragma unroll
                    for (u32 cc = 0; cc < (1u << SKM_PH_OB); ++cc)
                        if (cc < my_nch) owner[my_cstart + cc] = (u16)((tid << SKM_PH_OB) | cc);
                    if (myidx == 0) cbeg[myph] = my_cstart;
                    if (myidx + 1 == mycnt) cend[myph] = my_cstart + my_nch;
                }
            }
            if (!all_staged && tid == 0) scratch[2] = 0;
            __syncthreads();
        }
        if (!all_staged) {   // instances of the slot, a piece at a time
            u32 mine = 0;
            for (u32 ph = 0; ph < npieces; ++ph) {
                const KhSkmPiece pc = jb.pieces[ph];
                u32 nrec = ((ConstU32)(unsigned long long)pc.count)[slot];
                nrec = nrec < NT ? nrec : NT;
                if (tid < nrec) mine += SkmRec1::n((pc.rec + ((ConstU32)(unsigned long long)pc.off)[slot])[tid].w);
            }
            if (__builtin_amdgcn_ballot_w64(mine != 0)) {
                const u32 tot = wave_scan_add(mine);
                if (lane == KH_WAVE - 1) atomicAdd(&scratch[2], tot);
            }
            __syncthreads();
        }
        const u32 R = (((scratch[2] * jb.share_q8) >> 8) + SKM_PH_ROUND - 1u) / SKM_PH_ROUND;   // (an optimistic share_q8 that overfills a table is caught at the fold: the host runs the launch again with 256)
        for (u32 q = 0; q < R; ++q) {
            {   // a fresh table (the read-out before it is behind a barrier)
                uint4* k4 = reinterpret_cast<uint4*>(tkey);
#pragma unroll
                for (u32 e = 0; e < T / 2 / NT; ++e) k4[e * NT + tid] = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
                reinterpret_cast<uint4*>(tmlo)[tid] = make_uint4(0u, 0u, 0u, 0u);
                reinterpret_cast<uint4*>(tcnt)[tid] = make_uint4(0u, 0u, 0u, 0u);
                if (tid < T2) { okey[tid] = emptyv; omlo[tid] = 0u; ocnt[tid] = 0u; }
                if (tid == 0) { scratch[0] = 0; scratch[1] = 0; scratch[3] = 0; }
            }
            __syncthreads();
            // A phase = a piece and the pieces joined to it (join_next: the same tags — a sub-batch's side list): the fold
            // comes behind the last of them that holds records of this slot.
            bool open = false;   // uniform: insertions since the last fold
            if (all_staged) {
                for (u32 ph = 0; ph < npieces; ++ph) {
                    const u32 c0 = cbeg[ph], c1 = cend[ph], fl = pflag[ph];
                    if (c0 != c1) {   // uniform
                        const uint4* __restrict__ rec = prec[ph] + poff[ph];
                        const u32* __restrict__ msk = pmsk[ph] + poff[ph];
                        u32 fresh_n = 0;
                        for (u32 c = c0 + tid; c < c1; c += NT) {
                            const u32 o = owner[c], ri = rloc[o >> SKM_PH_OB] & 1023u;
                            insert_chunk(rec[ri], msk[ri], (o & ((1u << SKM_PH_OB) - 1u)) * (u32)E, fl >> 1, R, q, fresh_n);
                        }
                        count_fresh(fresh_n);
                        open = true;
                    }
                    if (open && !((fl & 1u) && ph + 1 < npieces)) { fold_now(); open = false; }
                }
            } else {
                constexpr u32 BATCH = SKM_PH_MAXCH >> SKM_PH_OB;   // records numbered at a time: their chunks fit the owner table
                u32 par = 0;
                for (u32 ph = 0; ph < npieces; ++ph) {
                    const KhSkmPiece pc = jb.pieces[ph];
                    u32 nrec = ((ConstU32)(unsigned long long)pc.count)[slot];
                    if (nrec > NT) {   // uniform
                        if (tid == 0) atomicOr(jb.ctl, KH_ERR_CAPACITY);
                        nrec = NT;
                    }
                    const u64 roff = ((ConstU32)(unsigned long long)pc.off)[slot];
                    const uint4* __restrict__ rec = pc.rec + roff;
                    const u32* __restrict__ msk = pc.mask + roff;
                    for (u32 b0 = 0; b0 < nrec; b0 += BATCH) {
                        // ---- number the chunks of the batch's records
                        const u32 nj = tid < BATCH && b0 + tid < nrec ? SkmRec1::n(rec[b0 + tid].w) : 0u;
                        const u32 nch = (nj + (u32)E - 1u) / (u32)E;
                        if (__builtin_amdgcn_ballot_w64(nch != 0)) {
                            const u32 incl = wave_scan_add(nch);
                            u32 wbase = 0;
                            if (lane == KH_WAVE - 1 && incl) wbase = atomicAdd(&scratch[par], incl);
                            wbase = (u32)__builtin_amdgcn_readlane((int)wbase, KH_WAVE - 1);
                            const u32 cstart = wbase + incl - nch;
#pragma unroll
                            for (u32 cc = 0; cc < (1u << SKM_PH_OB); ++cc)
                                if (cc < nch) owner[cstart + cc] = (u16)((tid << SKM_PH_OB) | cc);
                        }
                        __syncthreads();
                        const u32 C = scratch[par];   // (<= BATCH << SKM_PH_OB = SKM_PH_MAXCH)
                        par ^= 3u;                    // the batches' chunk counters alternate: [0] and [3]
                        if (tid == 0) scratch[par] = 0;   // (the next batch's: nobody reads it before the barrier below)
                        u32 fresh_n = 0;   // entries this thread created
                        for (u32 c = tid; c < C; c += NT) {
                            const u32 o = owner[c], ri = b0 + (o >> SKM_PH_OB);
                            insert_chunk(rec[ri], msk[ri], (o & ((1u << SKM_PH_OB) - 1u)) * (u32)E, pc.dup_row, R, q, fresh_n);
                        }
                        count_fresh(fresh_n);
                        open = true;
                        __syncthreads();   // the owner table is written again
                    }
                    if (open && !((pc.join_next & 1u) && ph + 1 < npieces)) { fold_now(); open = false; }
                }
            }
            // ---- every occupied entry is one distinct k-mer of the slot; its counter: in how many (phase, tag) pairs
            {
                const uint4 c4 = reinterpret_cast<uint4*>(tcnt)[tid];
                const u32 cv[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (cv[e]) {
                        u32 c = cv[e] < jb.cs ? cv[e] : jb.cs;
                        c = c < jb.hist_len - 1u ? c : jb.hist_len - 1u;
                        if (c < hbins) atomicAdd(&lhist[c], 1u);
                        else atomicAdd(&jb.hist[c], 1ull);
                    }
                }
                if (tid < T2 && ocnt[tid]) {
                    u32 c = ocnt[tid] < jb.cs ? ocnt[tid] : jb.cs;
                    c = c < jb.hist_len - 1u ? c : jb.hist_len - 1u;
                    if (c < hbins) atomicAdd(&lhist[c], 1u);
                    else atomicAdd(&jb.hist[c], 1ull);
                }
                if (tid == 0 && q + 1 == R) scratch[2] = 0;   // (everybody has worked R out, barriers ago)
            }
            __syncthreads();
        }
        if (!R) __syncthreads();   // (an empty slot: scratch[2] is written again only behind the next barrier anyway)
    }
    __syncthreads();
    if (tid0 < hbins && lhist[tid0]) atomicAdd(&jb.hist[tid0], (unsigned long long)lhist[tid0]);
}

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
template <int WW> static void launch_scatter_w(const KhSkmJob& job, u32 ntiles, size_t lds, hipStream_t st) {
    skm_allow_lds(k_skm_scatter<WW>, lds);
    hipLaunchKernelGGL(k_skm_scatter<WW>, dim3(ntiles), dim3(SKM_NT), lds, st, job);
}
static bool kh_skm_supports_w(u32 w) { return w >= (u32)SKM_WMIN && w <= (u32)SKM_WMAX; }
static void kh_launch_skm_scatter(const KhSkmJob& job, u32 ntiles, hipStream_t st) {
    if (!ntiles) return;
    const size_t lds = kh_skm_scatter_lds_bytes(job.nb1);
    switch (job.w) {
#define SKM_W(WW) case WW: launch_scatter_w<WW>(job, ntiles, lds, st); break;
        SKM_W(5) SKM_W(6) SKM_W(7) SKM_W(8) SKM_W(9) SKM_W(10) SKM_W(11) SKM_W(12) SKM_W(13) SKM_W(14) SKM_W(15) SKM_W(16)
        SKM_W(17) SKM_W(18)
#undef SKM_W
        default: break;   // the host asks kh_skm_supports_w first
    }
}
static void kh_launch_skm_regroup(const KhSkmJob& job, hipStream_t st) { skm_launch_regroup<SkmRec1>(job, st); }
template <int KT> static void launch_union_k(const KhSkmJob& job, u32 cs, u32 grid, hipStream_t st) {
    const size_t lds = SkmUnion::LDS;
    skm_allow_lds(k_skm_union<1024, 4096, KT>, lds);
    hipLaunchKernelGGL((k_skm_union<1024, 4096, KT>), dim3(grid), dim3(1024), lds, st, job, cs, skm_first_claimed(job.nslots, grid));
}
static void kh_launch_skm_union(const KhSkmJob& job, u32 cs, u32 grid, hipStream_t st) {
    switch (job.k) {
#define SKM_K(KK) case KK: launch_union_k<KK>(job, cs, grid, st); break;
        SKM_K(17) SKM_K(18) SKM_K(19) SKM_K(20) SKM_K(21) SKM_K(22) SKM_K(23) SKM_K(24)
        SKM_K(25) SKM_K(26) SKM_K(27) SKM_K(28) SKM_K(29) SKM_K(30) SKM_K(31) SKM_K(32)
#undef SKM_K
        default: launch_union_k<0>(job, cs, grid, st); break;   // any other k that reaches here (15, 16): k from the job
    }
}
// ------------------------------------------------------------------------------------------
// The workspace of a run (SkmRun, kh_engine.cpp) at both ends of the stream, as kernels: a copy engine between two
// kernels costs a hand-over of the queue each way (10 .. 17 us before k_skm_scatter, 10 us behind the union), a kernel
// that reads or writes the pinned staging itself costs none.
// k_skm_ws_init: ws[0, zero16) = 0, ws[zero16, zero16 + up16) = up[0, up16), in 16-byte words
// k_skm_ws_down: down[0, n8) = ws[0, n8), in 8-byte words
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_skm_ws_init(uint4* __restrict__ ws, const u32 zero16, const uint4* __restrict__ up, const u32 up16) {
    const u32 n = zero16 + up16, step = gridDim.x * 256u;
    for (u32 i = blockIdx.x * 256u + threadIdx.x; i < n; i += step)
        ws[i] = i < zero16 ? make_uint4(0u, 0u, 0u, 0u) : up[i - zero16];
}
__global__ __launch_bounds__(256) void k_skm_ws_down(unsigned long long* __restrict__ down, const unsigned long long* __restrict__ ws, const u32 n8) {
    for (u32 i = blockIdx.x * 256u + threadIdx.x; i < n8; i += gridDim.x * 256u) down[i] = ws[i];
}
void kh_launch_skm_ws_init(void* ws, size_t zero_bytes, const void* up, size_t up_bytes, hipStream_t st) {   // both multiples of 16
    const u32 zero16 = (u32)(zero_bytes / 16), up16 = (u32)(up_bytes / 16);
    if (!(zero16 + up16)) return;
    const u32 want = (zero16 + up16 + 255u) / 256u, grid = want < 1024u ? want : 1024u;
    hipLaunchKernelGGL(k_skm_ws_init, dim3(grid), dim3(256), 0, st, static_cast<uint4*>(ws), zero16, static_cast<const uint4*>(up), up16);
}
void kh_launch_skm_ws_down(void* down, const void* ws, size_t bytes, hipStream_t st) {   // a multiple of 8
    const u32 n8 = (u32)(bytes / 8);
    if (!n8) return;
    const u32 want = (n8 + 255u) / 256u, grid = want < 64u ? want : 64u;
    hipLaunchKernelGGL(k_skm_ws_down, dim3(grid), dim3(256), 0, st, static_cast<unsigned long long*>(down), static_cast<const unsigned long long*>(ws), n8);
}
void kh_launch_skm_pack(const KhSkmPackJob& job, hipStream_t st) {
    if (!job.nslots) return;
    if (job.cap2 <= 256) {
        hipLaunchKernelGGL(k_skm_pack<256>, dim3(job.nslots), dim3(256), skm_pack_lds_bytes(256), st, job);
    } else if (job.cap2 <= 512) {
        hipLaunchKernelGGL(k_skm_pack<512>, dim3(job.nslots), dim3(512), skm_pack_lds_bytes(512), st, job);
    } else {
        const size_t lds = skm_pack_lds_bytes(1024);
        skm_allow_lds(k_skm_pack<1024>, lds);
        hipLaunchKernelGGL(k_skm_pack<1024>, dim3(job.nslots), dim3(1024), lds, st, job);
    }
}
void kh_launch_skm_pack_compact(const KhSkmCompactJob& job, hipStream_t st) {
    if (!job.nparts || !job.nsub) return;
    const u32 z = job.nparts >= 16 ? 1u : 16u / job.nparts;   // about a thousand workgroups
    hipLaunchKernelGGL(k_skm_pack_compact, dim3(job.nsub, job.nparts, z), dim3(256), 0, st, job);
}
void kh_launch_skm_phased(const KhSkmPhasedJob& job, u32 grid, hipStream_t st) {
    if (!job.nslots || !grid) return;
    const size_t lds = kh_skm_phased_lds_bytes();
    skm_allow_lds(k_skm_phased, lds);
    hipLaunchKernelGGL(k_skm_phased, dim3(grid), dim3(SKM_PH_NT), lds, st, job);
}
// k_skm_cross (kh_skm_device.h) with one-word keys
constexpr bool SKM_CROSS1_VGPRS64 = true;   // resource report: 59 VGPRs, 78 SGPRs (54 more kept in VGPR lanes), no scratch, 8 waves per SIMD; 81280 bytes of LDS
// k_skm_cross with the type-2 read-out (SkmCrossOwn) and one-word keys
constexpr bool SKM_PIVOT1_VGPRS64 = true;   // resource report: 59 VGPRs, 78 SGPRs (54 more kept in VGPR lanes), no scratch, 8 waves per SIMD; 81280 bytes of LDS
const KhSkmWidth& kh_skm_width1() {
    static const KhSkmWidth wd = {
        (u32)sizeof(uint4) * SkmRec1::Q, KH_SKM_MAX_COARSE, KH_SKM_MAX_FINE, SkmUnion::MAXREC, SkmUnion::TABLE,
        2u /* two unions of 79 KB of LDS and 1024 threads fit a CU */, skm_cross_per_cu<SkmBig1>(SKM_CROSS1_VGPRS64),
        skm_cross_per_cu<SkmBig1>(SKM_PIVOT1_VGPRS64), skm_walk_round<SkmBig1>(),
        kh_skm_supports_w, kh_launch_skm_scatter, kh_launch_skm_regroup, kh_launch_skm_union, skm_launch_big<SkmBig1>,
        skm_launch_cross<SkmBig1>, skm_launch_pivot<SkmBig1>,
    };
    return wd;
}
