// khoice_amd — device helpers shared by the two super-k-mer kernel files (kh_skm.hip: one-word keys,
// kh_skm2.hip: two-word keys): minimizer hashing, sliding minimum, the LDS counting-sort flush, code-word prefetch,
// and the pieces both key widths are built from: the record formats (kh_skm_rec.h), the one-key probe walk, the
// read-out of genome masks into histogram bins, the regroup kernel, the walk of one slot and the two kernels built on
// it (k_skm_big: the overfull slots; k_skm_cross: experiment type 3).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "kh_device.h"
#include "kh_launch.h"
#include "kh_skm_rec.h"

#ifndef KH_TUNE_SKM_FULL_ROUNDS
#define KH_TUNE_SKM_FULL_ROUNDS 4   // probe rounds made by all keys of a thread together; the rest one key per lane (1 / 2 / 3 / 4 / 5 / 8 rounds: union 16.3 / 3.33 / 1.59 / 1.51 / 1.52 / 1.55 ms)
#endif

namespace {

constexpr u32 SKM_NT = 256;                    // threads of a scatter workgroup
constexpr u32 SKM_PPT = 32;                    // k-mer start positions per thread and sub-tile
constexpr u32 SKM_SUB = SKM_NT * SKM_PPT;      // 8192 positions per sub-tile
constexpr u32 SKM_CW = (SKM_SUB + KH_HALO) / 16;
constexpr u32 SKM_CAP = KH_SKM_STAGE;          // records staged in LDS per flush of the scatter
constexpr int SKM_WMIN = 5, SKM_WMAX = 18;     // m-mers per k-mer the scatter is instantiated for
constexpr u32 SKM_RG_NT = 1024;                // regroup: one workgroup per coarse bucket
static_assert(KH_SKM_MAX_FINE == 1u << SkmRec1::FINE_BITS && KH_SKM2_MAX_FINE == 1u << SkmRec2::FINE_BITS, "a fine slot index fills its field");

__device__ __forceinline__ u32 revpairs32(u32 x) {
    x = __builtin_bitreverse32(x);
    return ((x & 0x55555555u) << 1) | ((x >> 1) & 0x55555555u);
}
__device__ __forceinline__ u32 mmer_hash(u32 canon) {   // order of the m-mers: a bijection on 32 bits
    u32 h = canon * 0x9E3779B1u;   // (one multiply: quarter rate, and this runs once per base)
    h ^= h >> 15;
    return h;
}
__device__ __forceinline__ u32 slot_of(u32 minv, u32 nslots) {   // slot of a minimizer: independent of its rank
    u32 x = minv * 0xC2B2AE35u;
    x ^= x >> 16;
    x *= 0x27D4EB2Fu;
    x ^= x >> 15;
    return (u32)(((u64)x * (u64)nslots) >> 32);
}
// the value of the next lane (lane 63 keeps `old`): DPP wave_shl:1, no LDS round trip
__device__ __forceinline__ u32 next_lane(u32 v, u32 old) {
    return (u32)__builtin_amdgcn_update_dpp((int)old, (int)v, 0x130, 0xf, 0xf, false);
}
// v[s] for a run-time s < 32.  Per-lane register indexing does not exist; written as a tree of bit selects
// (v_bfi) so that the compiler does not turn it into a scratch array.
__device__ __forceinline__ u32 bsel(u32 m, u32 a, u32 b) { return (a & m) | (b & ~m); }   // m ? a : b, bitwise
__device__ __forceinline__ u32 pick32(const u32 (&v)[SKM_PPT], u32 s) {
    const u32 m0 = 0u - (s & 1u), m1 = 0u - ((s >> 1) & 1u), m2 = 0u - ((s >> 2) & 1u), m3 = 0u - ((s >> 3) & 1u),
              m4 = 0u - ((s >> 4) & 1u);
    u32 a[16], b[8], c[4];
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = bsel(m0, v[2 * i + 1], v[2 * i]);
#pragma unroll
    for (int i = 0; i < 8; ++i) b[i] = bsel(m1, a[2 * i + 1], a[2 * i]);
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = bsel(m2, b[2 * i + 1], b[2 * i]);
    return bsel(m4, bsel(m3, c[3], c[2]), bsel(m3, c[1], c[0]));
}

// Sliding minimum over windows of WW positions, in registers: in: cur[0 .. PPT + WW - 2], out: cur[j] =
// min(cur[j .. j + WW - 1]) for j < PPT.  Doubling up to the largest power of two L <= WW, then two
// overlapping windows of L.  (Measured and taken out again: a ladder of three-input minimums — windows of 3, of 9, then
// one step to WW: 116 v_min3_u32 / v_min_u32 instead of 162 at WW = 16 — left k_skm_scatter<16> where it was on its
// own, 0.5357 -> 0.5353 ms with a spread of 0.002: profiles/README.md, round 5.)
template <int WW>
__device__ __forceinline__ void window_min(u32 (&cur)[SKM_PPT + WW - 1]) {
    constexpr int L = WW >= 32 ? 32 : (WW >= 16 ? 16 : (WW >= 8 ? 8 : (WW >= 4 ? 4 : (WW >= 2 ? 2 : 1))));
    constexpr int X = (int)SKM_PPT + WW - 1;   // extent
    // after the level of stride s, cur[i] = min over 2s positions for i < X - (2s - 1)
#pragma unroll
    for (int s = 1; s < L; s <<= 1) {
#pragma unroll
        for (int i = 0; i < X - (2 * s - 1); ++i) cur[i] = cur[i] < cur[i + s] ? cur[i] : cur[i + s];
    }
    constexpr int D = WW - L;
    if (D) {
#pragma unroll
        for (int j = 0; j < (int)SKM_PPT; ++j) cur[j] = cur[j] < cur[j + D] ? cur[j] : cur[j + D];
    }
}

struct FlushLds {
    uint4* stage;   // [CAP * RW / 4]: records of RW 32-bit words
    u16* sid;       // [CAP] bucket of every staged record
    u32* bcnt;      // [nbk] records per bucket (zero on entry to a round)
    u32* bstart;    // [nbk + 1]
    u32* gpos;      // [nbk]
    u32* wsum;      // [16]
};
template <u32 CAP, u32 RW = 4> __device__ __forceinline__ FlushLds flush_lds(u8* base, u32 nbk_alloc) {
    FlushLds L;
    L.stage = reinterpret_cast<uint4*>(base);
    L.sid = reinterpret_cast<u16*>(base + (size_t)CAP * 4 * RW);
    L.bcnt = reinterpret_cast<u32*>(base + (size_t)CAP * (4 * RW + 2));
    L.bstart = L.bcnt + nbk_alloc;
    L.gpos = L.bstart + nbk_alloc + 4;
    L.wsum = L.gpos + nbk_alloc;
    return L;
}
template <u32 CAP, u32 RW = 4> constexpr size_t flush_lds_bytes(u32 nbk_alloc) {
    return (size_t)CAP * (4 * RW + 2) + (size_t)(3 * nbk_alloc + 4 + 16) * 4;
}

// Counting sort of the n staged records by bucket inside LDS, then every bucket's run goes to its region,
// consecutive lanes storing consecutive records.  The run's position comes from ONE returning global
// atomic (LOCAL == false: the scatter, whose buckets are shared by all workgroups) or from a cursor in LDS
// (LOCAL: the regroup, where a workgroup owns its buckets).  nbk <= 2 * NT.
// Entry: a barrier has made stage / sid / bcnt visible.  Exit: bcnt zeroed, a barrier passed.
// Records of a slot whose region is full (regroup): they go to a global side list with the number of
// their slot; the slots they belong to are taken by a kernel of their own afterwards (k_skm_big).
struct SkmSpill {
    uint4* rec = nullptr;     // [cap] records (of one or two uint4)
    u32* slot = nullptr;      // [cap]
    u32* n = nullptr;         // records spilled so far (may run past cap: the host then falls back)
    u32 cap = 0;
    u32 first_slot = 0;       // global number of the workgroup's bucket 0
};
template <u32 NT, u32 CAP, bool LOCAL, u32 RW = 4>
__device__ __forceinline__ void skm_flush(const FlushLds& L, const u32 n, const u32 nbk, u32* cursors,
                                          uint4* __restrict__ region, const u32 region_cap, u32* __restrict__ ctl,
                                          const SkmSpill sp = SkmSpill()) {
    constexpr u32 CS = LOCAL ? 1u : KH_SKM_CUR1_STRIDE;   // words between two cursors
    constexpr int RPT = (int)(CAP / NT);
    const u32 tid = threadIdx.x, lane = lane_id(), wid = tid >> 6;
    // ---- exclusive scan of the bucket counts (two buckets per thread), run reservation
    u32 c0 = 0, c1 = 0;
    const u32 b0 = 2 * tid, b1 = 2 * tid + 1;
    if (b0 < nbk) c0 = L.bcnt[b0];
    if (b1 < nbk) c1 = L.bcnt[b1];
    const u32 incl = wave_scan_add(c0 + c1);
    if (lane == KH_WAVE - 1) L.wsum[wid] = incl;
    if (c0) {
        u32 g;
        if (LOCAL) { g = cursors[b0]; cursors[b0] = g + c0; }
        else g = atomicAdd(&cursors[(size_t)b0 * CS], c0);
        L.gpos[b0] = g;
        if (g + c0 > region_cap && !sp.rec) atomicOr(ctl, KH_ERR_CAPACITY);
    }
    if (c1) {
        u32 g;
        if (LOCAL) { g = cursors[b1]; cursors[b1] = g + c1; }
        else g = atomicAdd(&cursors[(size_t)b1 * CS], c1);
        L.gpos[b1] = g;
        if (g + c1 > region_cap && !sp.rec) atomicOr(ctl, KH_ERR_CAPACITY);
    }
    // the staged records of this thread, into registers (they are placed in place)
    constexpr int Q = (int)(RW / 4);   // uint4 per record
    u32 rx[RPT * Q], ry[RPT * Q], rz[RPT * Q], rw[RPT * Q], bk[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const u32 i = tid + (u32)r * NT;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const uint4 v = L.stage[(i < n ? i : 0) * Q + q];
            rx[r * Q + q] = v.x; ry[r * Q + q] = v.y; rz[r * Q + q] = v.z; rw[r * Q + q] = v.w;
        }
        bk[r] = L.sid[i < n ? i : 0];
    }
    __syncthreads();
    if (!LOCAL) SKM_STAMP(12);
    u32 run = incl - (c0 + c1);
    for (u32 w = 0; w < wid; ++w) run += L.wsum[w];
    if (b0 < nbk) { L.bstart[b0] = run; L.bcnt[b0] = 0; }
    if (b1 < nbk) { L.bstart[b1] = run + c0; L.bcnt[b1] = 0; }
    __syncthreads();
    // ---- placement
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const u32 i = tid + (u32)r * NT;
        if (i < n) {
            const u32 at = L.bstart[bk[r]] + atomicAdd(&L.bcnt[bk[r]], 1u);
#pragma unroll
            for (int q = 0; q < Q; ++q) L.stage[at * Q + q] = make_uint4(rx[r * Q + q], ry[r * Q + q], rz[r * Q + q], rw[r * Q + q]);
            L.sid[at] = (u16)bk[r];
        }
    }
    __syncthreads();
    if (!LOCAL) SKM_STAMP(13);
    // ---- write-out
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const u32 i = tid + (u32)r * NT;
        if (i < n) {
            const u32 b = L.sid[i];
            const u32 dest = L.gpos[b] + (i - L.bstart[b]);
            if (dest < region_cap) {
#pragma unroll
                for (int q = 0; q < Q; ++q) region[((u64)b * region_cap + dest) * Q + q] = L.stage[i * Q + q];
            } else if (sp.rec) {   // the slot's region is full
                const u32 at = atomicAdd(sp.n, 1u);
                if (at < sp.cap) {
#pragma unroll
                    for (int q = 0; q < Q; ++q) sp.rec[(u64)at * Q + q] = L.stage[i * Q + q];
                    sp.slot[at] = sp.first_slot + b;
                }
            }
        }
    }
    __syncthreads();
    if (b0 < nbk) L.bcnt[b0] = 0;
    if (b1 < nbk) L.bcnt[b1] = 0;
    __syncthreads();
}

// the code words of one sub-tile, in flight while the previous one is processed
struct SkmFetch { uint4 v[3]; u32 left[3]; };
__device__ __forceinline__ void skm_fetch(const u8* __restrict__ sbase, const u64 len, const u64 p0, SkmFetch& f) {
#pragma unroll
    for (u32 r = 0; r < 3; ++r) {
        const u32 w = threadIdx.x + r * SKM_NT;
        f.left[r] = 0;
        f.v[r] = make_uint4(0, 0, 0, 0);
        if (w < SKM_CW) {
            const u64 b0 = p0 + 16ull * w;
            if (b0 < len) {
                const u64 left = len - b0;
                f.left[r] = left >= 16 ? 16u : (u32)left;
                if (left >= 16) {
                    f.v[r] = *reinterpret_cast<const uint4*>(sbase + b0);
                } else {   // last, partial word of the sequence: never touch bytes past its end
                    u32 w4[4] = {0, 0, 0, 0};
                    for (u32 i = 0; i < (u32)left; ++i) w4[i >> 2] |= (u32)sbase[b0 + i] << (8 * (i & 3));
                    f.v[r] = make_uint4(w4[0], w4[1], w4[2], w4[3]);
                }
            }
        }
    }
}
__device__ __forceinline__ void skm_store(const SkmFetch& f, u32* code, u16* bad16) {
#pragma unroll
    for (u32 r = 0; r < 3; ++r) {
        const u32 w = threadIdx.x + r * SKM_NT;
        if (w < SKM_CW) {
            u32 codes = 0, bad = 0xffffu;
            if (f.left[r]) {
                decode16(f.v[r], codes, bad);
                if (f.left[r] < 16) bad |= (0xffffu << f.left[r]) & 0xffffu;
            }
            code[w] = codes;
            bad16[w] = (u16)bad;
        }
    }
}

// ------------------------------------------------------------------------------------------
// The probe walk of ONE key by one lane (k_skm_big, k_skm_phased; the unions' vectorised rounds make the same
// decisions for all keys of a thread at once and fall back to a loop of their own): KH_TUNE_SKM_FULL_ROUNDS probes
// in the main table of T entries, eight in the second table of T2 with an independent hash, then the main table
// to its end; a full main table is KH_ERR_CAPACITY.  Occupied entries stay occupied, so every copy of a key takes
// the same decisions as the first.  claim(second, S) tries entry S of the main or the second table for the key and
// says what it found; hit(second, S, fresh) is called once, for the entry the key ends in.
// ------------------------------------------------------------------------------------------
enum SkmClaimed : u32 { SKM_OTHER_KEY = 0, SKM_SAME_KEY = 1, SKM_FRESH = 2 };
constexpr u32 skm_log2(u32 x) { return x <= 1u ? 0u : 1u + skm_log2(x >> 1); }
template <u32 T, u32 T2, class Claim, class Hit>
__device__ __forceinline__ void skm_probe_walk(const u32 H, u32* __restrict__ ctl, Claim&& claim, Hit&& hit) {
    static_assert((T & (T - 1u)) == 0u && (T2 & (T2 - 1u)) == 0u, "table indices are hash bits and wrap by a mask");
    constexpr u32 HBITS = skm_log2(T), H2BITS = skm_log2(T2);
    u32 S = H >> (32 - HBITS), probes = 0, level = 0;   // level 0: main table, 1: second table, 2: main table, unbounded
    while (true) {
        const u32 c = claim(level == 1, S);
        if (c != SKM_OTHER_KEY) {
            hit(level == 1, S, c == SKM_FRESH);
            break;
        }
        ++probes;
        if (level == 0 && probes >= (u32)KH_TUNE_SKM_FULL_ROUNDS) {
            level = 1; probes = 0;
            S = ((H ^ (H >> 15)) * 0x85EBCA77u) >> (32 - H2BITS);
        } else if (level == 1 && probes >= 8u) {   // a crowded second table: on in the main one
            level = 2; probes = 0;
            S = ((H >> (32 - HBITS)) + (u32)KH_TUNE_SKM_FULL_ROUNDS) & (T - 1u);
        } else if (level == 2 && probes >= T) {
            atomicOr(ctl, KH_ERR_CAPACITY);   // the main table is full: the key is dropped, the host falls back
            break;
        } else {
            S = (S + 1u) & (level == 1 ? T2 - 1u : T - 1u);
        }
    }
}
// the round (of R < 65536) in which a slot taken in R rounds of key subsets inserts a key: sixteen hash bits scaled to
// [0, R) (k_skm_big, k_skm_cross, k_skm_phased; the unions decide the same for all keys of a thread at once)
__device__ __forceinline__ u32 skm_round_of(const u32 H, const u32 R) { return (((H >> 4) & 0xffffu) * R) >> 16; }

// ------------------------------------------------------------------------------------------
// Read-out: the genome mask of one distinct k-mer -> histogram bins, kept in LDS until the workgroup ends.
// Per group that holds the k-mer: popcount of the mask inside the group -> the group's bin; number of groups -> the
// across-group bin.  hstripe holds 4 / 2 / 1 copies of every bin for <= 72 / 144 / 255 bins (sshift = 2 / 1 / 0; a
// lane adds to the copy of its number: fewer LDS atomics on one address), so 288 words take any of the three.
// Pointers and two uniform values only: `lane` and `tid` are arguments because the unions re-derive them per slot
// from an opaque copy of threadIdx.x (LDS addresses formed from them are then not kept live across the slot loop).
// ------------------------------------------------------------------------------------------
constexpr u32 SKM_HSTRIPE_WORDS = 288;
// an operand's entry of a group table: the mask of its group (two halves) from its ginfo word g (first operand of the
// group, operands in it, first bin: 8 + 8 + 16 bits), and a third word that is the read-out's own
__device__ __forceinline__ uint4 skm_group_entry(const u32 g, const u32 z) {
    const u32 g0 = g & 0xffu, gn = (g >> 8) & 0xffu;
    const u64 gm = gn ? (gn >= 64u ? ~0ull : ((1ull << gn) - 1ull)) << g0 : 0ull;
    return make_uint4((u32)gm, (u32)(gm >> 32), z, 0u);
}
struct SkmReadout {
    uint4* gtab;    // [KH_TAG_MAX_OPS] per operand: its group's mask (two halves), first bin << sshift
    u32* hstripe;   // [SKM_HSTRIPE_WORDS]
    u32* dupc;      // [KH_TAG_MAX_OPS] per genome: instances whose (k-mer, genome) pair was seen before
    u32 sshift, abase;
    // (by threads 0 .. 287 at least; a barrier follows before the first eval_mask)
    __device__ __forceinline__ void init(const u32* __restrict__ ginfo, const u32 nbins, const u32 abase_, const u32 tid) {
        sshift = nbins <= 72u ? 2u : (nbins <= 144u ? 1u : 0u);
        abase = abase_;
        if (tid < (u32)KH_TAG_MAX_OPS) {
            const u32 g = ginfo[tid];
            gtab[tid] = skm_group_entry(g, (g >> 16) << sshift);
            dupc[tid] = 0;
        }
        if (tid < SKM_HSTRIPE_WORDS) hstripe[tid] = 0;
    }
    // one distinct k-mer; true when it sits in exactly one group — nearly all do: the callers count those per wave
    // and hand the wave's total to add_single_group
    __device__ __forceinline__ bool eval_mask(const u32 lane, u32 mlo, u32 mhi, const u32 cs) const {
        const u32 lsel = lane & ((1u << sshift) - 1u);
        u32 ng = 0;
        do {
            const u32 first = mlo ? (u32)__builtin_ctz(mlo) : 32u + (u32)__builtin_ctz(mhi);
            const uint4 g = gtab[first];
            u32 c = (u32)__popc(mlo & g.x) + (u32)__popc(mhi & g.y);
            c = c < cs ? c : cs;
            atomicAdd(&hstripe[g.z + (c << sshift) + lsel], 1u);
            const u32 keep_hi = mlo ? ~0u : mhi - 1u;   // (the lowest bit goes in any case: a tag outside every group cannot hang the loop)
            mlo &= ~g.x & (mlo - 1u);
            mhi &= ~g.y & keep_hi;
            ++ng;
        } while (mlo | mhi);
        if (ng == 1u) return true;
        atomicAdd(&hstripe[((abase + (ng < cs ? ng : cs)) << sshift) + lsel], 1u);
        return false;
    }
    __device__ __forceinline__ void add_single_group(const u32 n) const { atomicAdd(&hstripe[(abase + 1u) << sshift], n); }
    // behind a barrier: the workgroup's bins into one replica of the histogram, its repeats into the genomes' counters
    __device__ __forceinline__ void flush(unsigned long long* __restrict__ rep, const u32 nbins, unsigned long long* __restrict__ dup,
                                          const u32 tid, const u32 nt) const {
        for (u32 i = tid; i < nbins; i += nt) {
            u32 v = 0;
            for (u32 j = 0; j < (1u << sshift); ++j) v += hstripe[(i << sshift) + j];
            if (v) atomicAdd(&rep[i], (unsigned long long)v);
        }
        if (tid < (u32)KH_TAG_MAX_OPS && dupc[tid]) atomicAdd(&dup[tid], (unsigned long long)dupc[tid]);
    }
};

template <u32 Q> struct SkmRecord { uint4 v[Q]; };   // a record in registers; its header: the last word of v[Q - 1]

// ------------------------------------------------------------------------------------------
// SLOTS BY CLAIM: which slots a persistent union workgroup works on (k_skm_union, k_skm2_union).
// The workgroups of a CU do not run at the same speed (the one dispatched first gets the vector issue slots first and
// walks 154 equal slots in 3/4 of the time of its neighbour, which then finishes alone on a half-empty CU).  So only
// the first share of the walk is strided as before (slot blockIdx.x + j * grid, the slots below `first_claimed`);
// behind it a workgroup takes claims of KH_TUNE_SKM_CLAIM consecutive slots from one device counter
// (KhSkmJob::claim, zeroed with the workspace at every call): the faster workgroup takes more slots.
// The pipeline keeps its depth: a workgroup holds the current slot and the next one and asks take() for the one after
// once per slot.  A claim is DRAWN a slot before take() needs it, by one lane of the last wave where that wave has
// the least to do (the end of the insertions: its chunks of the last pass are the first to run out), and handed over
// through a word of LDS that everybody reads behind the next slot's first barrier: no barrier of its own, no wait
// loop, and the round trip of the atomic is not on the path of the other waves.  All state is uniform (scalar
// registers).  A claim that reaches nslots is the last one drawn; slots at or beyond nslots are empty ones to the
// caller.  KH_TUNE_SKM_CLAIM 0: the static walk throughout.
// ------------------------------------------------------------------------------------------
#ifndef KH_TUNE_SKM_CLAIM
#define KH_TUNE_SKM_CLAIM 2   // slots per claim (sweep: profiles/README.md, 2026-10-19)
#endif
#ifndef KH_TUNE_SKM_CLAIM_STATIC_PCT
#define KH_TUNE_SKM_CLAIM_STATIC_PCT 50   // share of a workgroup's rounds (nslots / grid) that is walked strided, in per cent
#endif
// The first slot that is claimed: behind the strided rounds, of which there are at least three (the pipeline's depth:
// no atomic at the head of the kernel).  Host side, an argument of the kernels.
inline u32 skm_first_claimed(const u32 nslots, const u32 grid) {
    if (!KH_TUNE_SKM_CLAIM) return ~0u;
    const u64 rounds = std::max<u64>(3, (u64)(nslots / grid) * (u32)KH_TUNE_SKM_CLAIM_STATIC_PCT / 100);
    return (u32)std::min<u64>(rounds * grid, 0xfffffff0u);
}
struct SkmSlotFeed {
    static constexpr u32 B = KH_TUNE_SKM_CLAIM;
    u32 grid, nslots, base;   // base: the first claimed slot
    u32 stat;                 // the next strided slot
    u32 cnext, cend;          // the claim in hand: slots [cnext, cend)
    // (the workgroup starts with slots blockIdx.x and blockIdx.x + grid in its pipeline)
    __device__ __forceinline__ SkmSlotFeed(const u32 grid_, const u32 nslots_, const u32 first_claimed)
        : grid(grid_), nslots(nslots_), base(first_claimed), stat(blockIdx.x + 2u * grid_), cnext(0), cend(0) {}
    // true: the next take() opens a new claim, which has to be drawn (draw()) before the barrier in front of it
    __device__ __forceinline__ bool wants() const { return B && stat >= base && cnext == cend && cend <= nslots; }
    // one lane draws; `box`: the LDS word that hands the claim over
    __device__ __forceinline__ void draw(u32* __restrict__ counter, u32* box) const { *box = base + atomicAdd(counter, B); }
    // the slot two behind the current one; every thread, behind a barrier that follows the draw
    __device__ __forceinline__ u32 take(const u32* box) {
        if (!B || stat < base) {
            const u32 s = stat;
            stat += grid;
            return s;
        }
        if (cnext == cend && cend <= nslots) {
            cnext = (u32)__builtin_amdgcn_readfirstlane((int)*box);
            cend = cnext + B;
        }
        return cnext++;
    }
};

template <class K> void skm_allow_lds(K kern, size_t bytes) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

}   // namespace

// ------------------------------------------------------------------------------------------
// S2a: one workgroup per coarse bucket walks its records a round at a time and regroups them by fine slot.
// The workgroup owns every slot of its bucket: the slot cursors live in LDS, no global atomic is needed.
// A round is SKM_RG_U4 uint4 of records whatever their size: 8192 one-word records, 4096 two-word ones.
// ------------------------------------------------------------------------------------------
constexpr u32 SKM_RG_U4 = 8192;
template <class Rec> constexpr size_t skm_regroup_lds_bytes(u32 S) {
    return flush_lds_bytes<SKM_RG_U4 / Rec::Q, 4 * Rec::Q>((S + 3) & ~3u) + (size_t)((S + 3) & ~3u) * 4 + 64;
}
template <class Rec>
__global__ __launch_bounds__(SKM_RG_NT, 4) void k_skm_regroup(const KhSkmJob jb) {
    extern __shared__ __attribute__((aligned(16))) u8 lds_raw[];
    constexpr u32 Q = Rec::Q, CAP = SKM_RG_U4 / Q, RW = 4 * Q;
    constexpr int RPT = (int)(CAP / SKM_RG_NT);
    const u32 nbk = (jb.S + 3) & ~3u;
    const FlushLds L = flush_lds<CAP, RW>(lds_raw, nbk);
    u32* lcur = reinterpret_cast<u32*>(lds_raw + flush_lds_bytes<CAP, RW>(nbk));   // [nbk] records written per slot
    const u32 tid = threadIdx.x;
    const u32 b = blockIdx.x;
    const u32 have = jb.cur1[(size_t)b * KH_SKM_CUR1_STRIDE];
    const u32 cnt = have < jb.cap1 ? have : jb.cap1;
    const u32 first_slot = b * jb.S;
    const u32 nfine = jb.nslots - first_slot < jb.S ? jb.nslots - first_slot : jb.S;
    for (u32 i = tid; i < nbk; i += SKM_RG_NT) { L.bcnt[i] = 0; lcur[i] = 0; }
    const uint4* __restrict__ src = jb.reg1 + (u64)b * jb.cap1 * Q;
    uint4* __restrict__ dst = jb.reg2 + (u64)first_slot * jb.cap2 * Q;
    uint4 nx[RPT][Q];
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const u32 i = tid + (u32)r * SKM_RG_NT;
#pragma unroll
        for (u32 q = 0; q < Q; ++q) nx[r][q] = i < cnt ? src[Q * i + q] : make_uint4(0, 0, 0, 0);
    }
    __syncthreads();
    for (u32 start = 0; start < cnt; start += CAP) {
        const u32 n = cnt - start < CAP ? cnt - start : CAP;
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            const u32 i = tid + (u32)r * SKM_RG_NT;
            if (i < n) {
                u32 fine = Rec::fine(nx[r][Q - 1].w);
                if (fine >= nfine) { fine = 0; atomicOr(jb.ctl, KH_ERR_ORDER); }   // a corrupt record never leaves its bucket
#pragma unroll
                for (u32 q = 0; q < Q; ++q) L.stage[Q * i + q] = nx[r][q];
                L.sid[i] = (u16)fine;
                atomicAdd(&L.bcnt[fine], 1u);
            }
        }
        // the next round's records: in flight during the flush
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            const u32 i = start + CAP + tid + (u32)r * SKM_RG_NT;
#pragma unroll
            for (u32 q = 0; q < Q; ++q) nx[r][q] = i < cnt ? src[Q * i + q] : make_uint4(0, 0, 0, 0);
        }
        __syncthreads();
        SkmSpill sp;
        sp.rec = jb.spill_rec; sp.slot = jb.spill_slot; sp.n = jb.ctl + KH_SKM_CTL_SPILLED; sp.cap = jb.spill_cap; sp.first_slot = first_slot;
        skm_flush<SKM_RG_NT, CAP, true, RW>(L, n, nfine, lcur, dst, jb.cap2, jb.ctl, sp);
    }
    for (u32 i = tid; i < nfine; i += SKM_RG_NT) jb.cur2[first_slot + i] = lcur[i];
}
template <class Rec> void skm_launch_regroup(const KhSkmJob& job, hipStream_t st) {
    const size_t lds = skm_regroup_lds_bytes<Rec>(job.S);
    skm_allow_lds(k_skm_regroup<Rec>, lds);
    hipLaunchKernelGGL(k_skm_regroup<Rec>, dim3(job.nb1), dim3(SKM_RG_NT), lds, st, job);
}

// ------------------------------------------------------------------------------------------
// The walk of ONE slot whatever its size, by one workgroup (k_skm_big: the slots the unions leave alone; k_skm_cross:
// every slot of experiment type 3).  The records in the slot's region, then — where asked — its records on the side
// list (found by a scan of the list: it is short); their k-mer instances are counted (N) and taken in
// R = ceil(N / skm_walk_round) rounds of key subsets (skm_round_of).  A round clears the table, numbers the chunks of
// the records in batches of Tr::BATCH, puts every k-mer of its subset into the table by the probe walk above, the bit
// of the record's operand into the mask plane of its half, and hands the table to the read-out the caller supplies,
// which scans it with for_each_occupied.  No merge of identical records: nothing here is tuned, it only has to be right.
//
// One walk for both key widths.  Tr (SkmBig1 in kh_skm.hip, SkmBig2 in kh_skm2.hip) supplies:
//   Rec, Consts, Key         the record format, the per-launch constants of the expander, a canonical key
//   T, T2, KEY_BYTES         main and second table; per entry KEY_BYTES of key planes (u64 planes, the first of
//                            which is all ones in an empty entry), then two u32 planes: the halves of the operand mask
//   BATCH, OB, E             records numbered at a time; bits of a chunk's number inside its record; k-mers per chunk
//   expand(r, first, kc, f)  the chunk expander: f(e, key) for the E k-mers from k-mer `first` of record r on
//   hash(key), claim(main, off, key)      the table hash; the claim functor of the probe walk (key planes of the main
//                            table, the second table's `off` u64 behind them)
// ------------------------------------------------------------------------------------------
constexpr u32 SKM_BIG_NT = 1024, SKM_BIG_IDX = 4096;   // threads; records of one slot on the side list that are indexed
template <class Tr> constexpr u32 skm_walk_round() { return Tr::T - Tr::T / 4; }   // k-mer instances a round takes

// The walk's LDS.  BINW: the words a kernel keeps for its bins.  sidx comes last: a launch that reads no side list
// leaves it out (bytes(false)).
template <class Tr, u32 BINW> struct SkmWalkLds {
    static constexpr u32 T = Tr::T, T2 = Tr::T2, KB = Tr::KEY_BYTES, MAXCH = Tr::BATCH << Tr::OB;
    static constexpr u32 KMAIN = 0, TMLO = KMAIN + T * KB, TMHI = TMLO + T * 4, KSECOND = TMHI + T * 4, OMLO = KSECOND + T2 * KB,
                         OMHI = OMLO + T2 * 4, GTAB = OMHI + T2 * 4, SCRATCH = GTAB + 1024, DUPC = SCRATCH + 128, BINS = DUPC + 256,
                         OWNER = BINS + BINW * 4, SIDX = OWNER + MAXCH * 2;
    static constexpr size_t bytes(bool side) { return SIDX + (side ? SKM_BIG_IDX * 4 : 0); }
    // the second table behind the main one: its mask planes from tmlo in words, its key planes from kmain in u64 (one
    // base pointer and integer offsets: a choice between two pointers held by reference is a choice between their
    // homes in memory)
    static constexpr u32 OMASK_OFF = (OMLO - TMLO) / 4, OKEY_OFF = (KSECOND - KMAIN) / 8;
    u8* kmain;      // [T * KB] key planes of the main table
    u32* tmlo;      // [T] [T] the two halves of its operand masks (tmhi follows tmlo)
    u32* tmhi;
    u8* ksecond;    // [T2 * KB] [T2] [T2] the second table, likewise
    u32* omlo;
    u32* omhi;
    uint4* gtab;    // [KH_TAG_MAX_OPS] per operand: its group's mask (skm_group_entry)
    u32* scratch;   // [0] chunks, [2] k-mers, [3] side-list records
    u32* dupc;      // [KH_TAG_MAX_OPS] per operand: instances whose (k-mer, operand) pair was seen before
    u32* bins;      // [BINW]
    u16* owner;     // [MAXCH] a chunk's record inside the batch << OB | its number inside the record
    u32* sidx;      // [SKM_BIG_IDX] this slot's records on the side list
    __device__ __forceinline__ explicit SkmWalkLds(u8* b)
        : kmain(b + KMAIN), tmlo(reinterpret_cast<u32*>(b + TMLO)), tmhi(reinterpret_cast<u32*>(b + TMHI)), ksecond(b + KSECOND),
          omlo(reinterpret_cast<u32*>(b + OMLO)), omhi(reinterpret_cast<u32*>(b + OMHI)), gtab(reinterpret_cast<uint4*>(b + GTAB)),
          scratch(reinterpret_cast<u32*>(b + SCRATCH)), dupc(reinterpret_cast<u32*>(b + DUPC)), bins(reinterpret_cast<u32*>(b + BINS)),
          owner(reinterpret_cast<u16*>(b + OWNER)), sidx(reinterpret_cast<u32*>(b + SIDX)) {}
};

template <class Tr, u32 BINW> struct SkmSlotWalk {
    using Rec = typename Tr::Rec;
    using Lds = SkmWalkLds<Tr, BINW>;
    static constexpr u32 NT = SKM_BIG_NT, T = Tr::T, T2 = Tr::T2, Q = Rec::Q, MAXCH = Lds::MAXCH, E = (u32)Tr::E;
    static constexpr u64 EMPTY = ~0ull;
    const Lds L;
    const KhSkmJob& jb;
    const typename Tr::Consts kc;
    const u32 tid, lane;
    // the slot in hand (open): its region, records there and in all, k-mer instances, rounds
    const uint4* __restrict__ reg;
    u32 nreg, nall, N, R;
    __device__ __forceinline__ SkmSlotWalk(u8* lds, const KhSkmJob& jb_) : L(lds), jb(jb_), kc(jb_.k), tid(threadIdx.x), lane(lane_id()) {}
    // (a barrier follows before open)
    __device__ __forceinline__ void reset() const { if (tid < 8) L.scratch[tid] = 0; }
    __device__ __forceinline__ u32 side_records() const {
        const u32 n = jb.ctl[KH_SKM_CTL_SPILLED];
        return n < jb.spill_cap ? n : jb.spill_cap;
    }
    // uint4 q of record i; the header sits in the last word of uint4 Q - 1
    __device__ __forceinline__ uint4 rec_q(const u32 i, const u32 q) const {
        return i < nreg ? reg[(u64)Q * i + q] : jb.spill_rec[(u64)Q * L.sidx[i - nreg] + q];
    }
    // Slot `slot` with `have` records written to its region; side (uniform): also its records among the `nspill` of
    // the side list.  Behind it N and R are known to every thread.
    __device__ __forceinline__ void open(const u32 slot, const u32 have, const bool side, const u32 nspill) {
        u32 nside = 0;
        if (side) {
            for (u32 i = tid; i < nspill; i += NT) {
                if (jb.spill_slot[i] == slot) {
                    const u32 at = atomicAdd(&L.scratch[3], 1u);
                    if (at < SKM_BIG_IDX) L.sidx[at] = i;
                }
            }
            __syncthreads();
            nside = L.scratch[3];
            if (nside > SKM_BIG_IDX) {   // (more than the walk indexes: the host falls back)
                if (tid == 0) atomicOr(jb.ctl, KH_ERR_CAPACITY);
                nside = SKM_BIG_IDX;
            }
        }
        nreg = have < jb.cap2 ? have : jb.cap2;   // (full for an overfull slot; a slot listed for its chunks may hold fewer)
        reg = jb.reg2 + (u64)slot * jb.cap2 * Q;
        nall = nreg + nside;
        {
            u32 mine = 0;
            for (u32 i = tid; i < nall; i += NT) mine += Rec::n(rec_q(i, Q - 1).w);
            const u32 tot = wave_scan_add(mine);
            if (lane == KH_WAVE - 1 && tot) atomicAdd(&L.scratch[2], tot);
        }
        __syncthreads();
        N = L.scratch[2];
        R = (N + skm_walk_round<Tr>() - 1u) / skm_walk_round<Tr>();
    }
    // Rounds q0, q0 + qstep, ... of the slot: readout() is called with the round's masks final, a barrier follows it.
    template <class Readout> __device__ __forceinline__ void rounds(const u32 q0, const u32 qstep, Readout&& readout) {
        for (u32 q = q0; q < R; q += qstep) {
            // a fresh table: key planes all ones, both mask planes zero
            for (u32 i = tid; i < T * Tr::KEY_BYTES / 16; i += NT) reinterpret_cast<uint4*>(L.kmain)[i] = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
            for (u32 i = tid; i < T2 * Tr::KEY_BYTES / 16; i += NT) reinterpret_cast<uint4*>(L.ksecond)[i] = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
            for (u32 i = tid; i < T / 2; i += NT) reinterpret_cast<uint4*>(L.tmlo)[i] = make_uint4(0u, 0u, 0u, 0u);
            if (tid < T2) { L.omlo[tid] = 0u; L.omhi[tid] = 0u; }
            __syncthreads();
            for (u32 b0 = 0; b0 < nall; b0 += Tr::BATCH) {   // batches of records, one per thread of the first waves
                const u32 mine_i = b0 + tid;
                const u32 nj = tid < Tr::BATCH && mine_i < nall ? Rec::n(rec_q(mine_i, Q - 1).w) : 0u;
                const u32 nch = (nj + E - 1u) / E;
                {
                    const u32 incl = wave_scan_add(nch);
                    u32 wbase = 0;
                    if (lane == KH_WAVE - 1 && incl) wbase = atomicAdd(&L.scratch[0], incl);
                    wbase = (u32)__builtin_amdgcn_readlane((int)wbase, KH_WAVE - 1);
                    const u32 cstart = wbase + incl - nch;
                    if (cstart + nch <= MAXCH)
                        for (u32 cc = 0; cc < nch; ++cc) L.owner[cstart + cc] = (u16)((tid << Tr::OB) | cc);
                }
                __syncthreads();
                u32 C = L.scratch[0];
                if (C > MAXCH) {   // (cannot happen: a record has at most 1 << OB chunks)
                    if (tid == 0) atomicOr(jb.ctl, KH_ERR_CAPACITY);
                    C = 0;
                }
                for (u32 c = tid; c < C; c += NT) {
                    const u32 o = L.owner[c], ri = b0 + (o >> Tr::OB), first = (o & ((1u << Tr::OB) - 1u)) * E;
                    SkmRecord<Q> r0;
#pragma unroll
                    for (u32 qq = 0; qq < Q; ++qq) r0.v[qq] = rec_q(ri, qq);
                    const u32 hw = r0.v[Q - 1].w;
                    const u32 tg = Rec::tag(hw), bit = 1u << (tg & 31u), half = Rec::half(hw);
                    const u32 cnt = Rec::n(hw) - first;   // k-mers of the record from `first` on: the chunk holds min(cnt, E)
                    Tr::expand(r0, first, kc, [&](const u32 e, const typename Tr::Key& K) __attribute__((always_inline)) {
                        if (e >= cnt) return;
                        const u32 H = Tr::hash(K);
                        if (R != 1 && skm_round_of(H, R) != q) return;   // another round's key
                        skm_probe_walk<T, T2>(H, jb.ctl, Tr::claim(L.kmain, Lds::OKEY_OFF, K), [&](const bool second, const u32 S, bool) __attribute__((always_inline)) {
                            u32* const mp = L.tmlo + (second ? Lds::OMASK_OFF + half * T2 : half * T) + S;
                            if (atomicOr(mp, bit) & bit) atomicAdd(&L.dupc[tg], 1u);   // this operand had the k-mer already
                        });
                    });
                }
                __syncthreads();
                if (tid == 0) L.scratch[0] = 0;
                __syncthreads();
            }
            readout();
            __syncthreads();
        }
    }
    // f(mlo, mhi): the operand mask of every occupied entry of the round's table
    template <class F> __device__ __forceinline__ void for_each_occupied(F&& f) const {
        for (u32 i = tid; i < T; i += NT)
            if (reinterpret_cast<const u64*>(L.kmain)[i] != EMPTY) f(L.tmlo[i], L.tmhi[i]);
        if (tid < T2 && reinterpret_cast<const u64*>(L.ksecond)[tid] != EMPTY) f(L.omlo[tid], L.omhi[tid]);
    }
};

// ------------------------------------------------------------------------------------------
// Overfull slots.  A minimizer that far more k-mers share than a hash predicts — poly-A, a tandem repeat's unit, an
// insertion sequence in 50 copies — fills its slot's region; the regroup puts what does not fit on a side list and
// the union leaves such slots alone (as it does slots with more chunks than it numbers).  Here one workgroup takes
// one of them by the walk above, always with its records on the side list; the rounds are shared out over
// blockIdx.y, and each is read out through SkmReadout into the histograms of experiment type 1.  A handful of slots
// per run.  KH_SKM_CTL_FULLEST: an atomic per slot; KH_SKM_CTL_EXPANDED: by the workgroup of blockIdx.y == 0.
// ------------------------------------------------------------------------------------------
template <class Tr> constexpr size_t skm_big_lds_bytes() { return SkmWalkLds<Tr, SKM_HSTRIPE_WORDS>::bytes(true); }
template <class Tr>
__global__ __launch_bounds__(SKM_BIG_NT) void k_skm_big(const KhSkmJob jb, u32 cs) {
    extern __shared__ __attribute__((aligned(16))) u8 lds_raw[];
    SkmSlotWalk<Tr, SKM_HSTRIPE_WORDS> w(lds_raw, jb);
    SkmReadout ro;
    ro.gtab = w.L.gtab;
    ro.dupc = w.L.dupc;
    ro.hstripe = w.L.bins;
    const u32 slot = jb.big_list[blockIdx.x];
    ro.init(jb.ginfo, jb.nbins, jb.abase, w.tid);
    w.reset();
    __syncthreads();
    w.open(slot, jb.cur2[slot], true, w.side_records());
    if (w.tid == 0 && w.N > Tr::T) atomicMax(jb.ctl + KH_SKM_CTL_FULLEST, w.N);
    // (the rounds are independent: workgroups (slot, y) share them out)
    w.rounds(blockIdx.y, gridDim.y, [&]() __attribute__((always_inline)) {
        u32 ones = 0;   // entries in exactly one group: counted per wave
        w.for_each_occupied([&](const u32 mlo, const u32 mhi) __attribute__((always_inline)) {
            if (ro.eval_mask(w.lane, mlo, mhi, cs)) ++ones;
        });
        ones = wave_scan_add(ones);
        if (w.lane == KH_WAVE - 1 && ones) ro.add_single_group(ones);
    });
    ro.flush(jb.hist + (u64)(blockIdx.x % jb.reps) * jb.nbins, jb.nbins, jb.dup, w.tid, SKM_BIG_NT);
    if (w.tid == 0 && blockIdx.y == 0) atomicAdd(jb.ctl + KH_SKM_CTL_EXPANDED, w.N);
}
template <class Tr> void skm_launch_big(const KhSkmJob& job, u32 cs, u32 nbig, hipStream_t st) {
    if (!nbig) return;
    const char* e = getenv("KHOICE_SKM_BIG_Y");   // the rounds of a slot side by side (1 .. 16 workgroups per slot)
    const int y = e ? atoi(e) : 4;
    const size_t lds = skm_big_lds_bytes<Tr>();
    skm_allow_lds(k_skm_big<Tr>, lds);
    hipLaunchKernelGGL(k_skm_big<Tr>, dim3(nbig, nbig < 2048u ? (u32)(y < 1 ? 1 : (y > 16 ? 16 : y)) : 1u), dim3(SKM_BIG_NT), lds, st, job, cs);
}

// ------------------------------------------------------------------------------------------
// Experiment type 3 (kh_exp3_run above the bitmaps): pivots against groups from the same records.  The operands are
// the genomes in group-major order, then the pivots (read sets) of the pass as further tags: bit t of a key's 64-bit
// mask says that operand t holds it.  The walk above, every round of a slot in turn, and a read-out that knows the
// pivots: an entry whose mask holds pivots P and, of group g, c >= 1 genomes adds one to bin
// q * ngenomes + (first genome of g) + c - 1 for every q in P (k_bmp_cross's bins; the host clamps the counts).  An
// entry no pivot holds counts nowhere.  No counter across groups, no own-group exception (SkmCrossGroups).
//
// Experiment type 2 (kh_exp2_run above the bitmaps) is the same kernel with another read-out: every pivot
// was held out of ONE group, its own.  An entry with genome bits G and pivots P has T = the groups with a genome in G;
// for every q in P, with c = the genomes of q's own group in G: one to q's within bin c (0 .. size of the group) and
// one to its across bin T - (c > 0) (0 .. ngroups - 1 OTHER groups) — every distinct k-mer of a pivot counts once in
// each (SkmCrossOwn).  Pivot q owns size + 1 + ngroups consecutive bins; the host says where (KhSkmPivotJob::pinfo).
// Type 4 will need a read-out of its own beside these two.
//
// Two launches of one body.  DIRECT (cj.nlisted == 0): persistent workgroups walk all slots grid-strided; a slot with
// more records than its region holds is listed (big_list, KH_SKM_CTL_LISTED) as the unions list it, and skipped.  LISTED: work
// item i is slot big_list[i], its region plus its records on the side list.  The bins stay in LDS over the whole walk
// and go to one replica of the device block at the end; so do the statistics, kept in registers until then.
// KH_SKM_CTL_MULTI: slots taken in more than one round.
// ------------------------------------------------------------------------------------------
constexpr u32 SKM_CROSS_BINS = 1024;   // bins of a pass at most (type 3: pivots x genomes, 32 x 32 of 64 operands)
template <class Tr> constexpr size_t skm_cross_lds_bytes(bool listed) { return SkmWalkLds<Tr, SKM_CROSS_BINS>::bytes(listed); }
// The read-outs: what the body below needs of one, both static.  entry(jb, xj, ngen, tid): operand tid's word of gtab
// (threads 0 .. 63, before the first barrier); count(...): one occupied entry of a round's table, counted into `bins`.
// Type 3: the pivots of the mask against every group of its genomes.  gtab .z: the group's first genome.
struct SkmCrossGroups {
    using Job = KhSkmCrossJob;
    static __device__ __forceinline__ const KhSkmCrossJob& cross(const Job& xj) { return xj; }
    static __device__ __forceinline__ uint4 entry(const KhSkmJob& jb, const KhSkmCrossJob&, const u32, const u32 tid) {
        const u32 g = jb.ginfo[tid];
        return skm_group_entry(g, g & 0xffu);
    }
    static __device__ __forceinline__ void count(const uint4* const gtab, u32* const bins, const u32 nbins, const u32 ngen, const u32 pmlo,
                                                 const u32 pmhi, u32 mlo, u32 mhi) {
        const u32 plo = mlo & pmlo, phi = mhi & pmhi;
        if (!(plo | phi)) return;
        mlo &= ~pmlo;
        mhi &= ~pmhi;
        while (mlo | mhi) {
            const u32 first = mlo ? (u32)__builtin_ctz(mlo) : 32u + (u32)__builtin_ctz(mhi);
            const uint4 g = gtab[first];
            const u32 c = (u32)__popc(mlo & g.x) + (u32)__popc(mhi & g.y);
            const u32 bin = g.z + c - 1u;   // (c >= 1: the group's mask holds `first`; a tag outside every group counts as a group of one)
            u32 ql = plo, qh = phi;
            while (ql | qh) {
                const u32 op = ql ? (u32)__builtin_ctz(ql) : 32u + (u32)__builtin_ctz(qh);
                const u32 at = (op - ngen) * ngen + bin;
                if (op >= ngen && bin < ngen && at < nbins) atomicAdd(&bins[at], 1u);
                if (ql) ql &= ql - 1u; else qh &= qh - 1u;
            }
            const u32 keep_hi = mlo ? ~0u : mhi - 1u;   // (the lowest bit goes in any case: the loop ends)
            mlo &= ~g.x & (mlo - 1u);
            mhi &= ~g.y & keep_hi;
        }
    }
};
// Type 2: every pivot of the mask against its own group and against the number of groups.  gtab of a genome: its
// group's mask; of a pivot operand (never looked up by the group walk: the pivots' bits are masked off before it): the
// mask of its OWN group's genomes, .z its first within bin, .w its first across bin.
struct SkmCrossOwn {
    using Job = KhSkmPivotJob;
    static __device__ __forceinline__ const KhSkmCrossJob& cross(const Job& xj) { return xj.cj; }
    static __device__ __forceinline__ uint4 entry(const KhSkmJob& jb, const KhSkmPivotJob& pj, const u32 ngen, const u32 tid) {
        if (tid < ngen) return skm_group_entry(jb.ginfo[tid], 0u);
        const u32 g = pj.pinfo[tid];
        uint4 e = skm_group_entry(g, g >> 16);
        e.w = e.z + ((g >> 8) & 0xffu) + 1u;
        return e;
    }
    static __device__ __forceinline__ void count(const uint4* const gtab, u32* const bins, const u32 nbins, const u32, const u32 pmlo,
                                                 const u32 pmhi, const u32 mlo, const u32 mhi) {
        u32 ql = mlo & pmlo, qh = mhi & pmhi;
        if (!(ql | qh)) return;
        const u32 glo = mlo & ~pmlo, ghi = mhi & ~pmhi;
        u32 T = 0;   // groups with a genome in the mask
        {
            u32 a = glo, b = ghi;
            while (a | b) {
                const u32 first = a ? (u32)__builtin_ctz(a) : 32u + (u32)__builtin_ctz(b);
                const uint4 g = gtab[first];
                ++T;
                const u32 keep_hi = a ? ~0u : b - 1u;   // (the lowest bit goes in any case: the loop ends)
                a &= ~g.x & (a - 1u);
                b &= ~g.y & keep_hi;
            }
        }
        while (ql | qh) {
            const u32 op = ql ? (u32)__builtin_ctz(ql) : 32u + (u32)__builtin_ctz(qh);
            const uint4 e = gtab[op];
            const u32 c = (u32)__popc(glo & e.x) + (u32)__popc(ghi & e.y);
            const u32 wbin = e.z + c, abin = e.w + T - (c ? 1u : 0u);
            if (wbin < nbins) atomicAdd(&bins[wbin], 1u);
            if (abin < nbins) atomicAdd(&bins[abin], 1u);
            if (ql) ql &= ql - 1u; else qh &= qh - 1u;
        }
    }
};
// One kernel, the read-out its second template parameter.  xj: the read-out's job (KhSkmCrossJob itself, or the
// KhSkmPivotJob that holds one).
template <class Tr, class Readout>
__global__ __launch_bounds__(SKM_BIG_NT, 8) void k_skm_cross(const KhSkmJob jb, const typename Readout::Job xj) {
    extern __shared__ __attribute__((aligned(16))) u8 lds_raw[];
    const KhSkmCrossJob& cj = Readout::cross(xj);
    constexpr u32 NT = SKM_BIG_NT;
    SkmSlotWalk<Tr, SKM_CROSS_BINS> w(lds_raw, jb);
    uint4* const gtab = w.L.gtab;
    u32* const bins = w.L.bins;
    const u32 tid = w.tid;
    const u32 cap2 = jb.cap2;
    const bool listed = cj.nlisted != 0u;
    const u32 nwork = listed ? (cj.nlisted < jb.big_cap ? cj.nlisted : jb.big_cap) : jb.nslots;
    const u32 nbins = cj.nbins < SKM_CROSS_BINS ? cj.nbins : SKM_CROSS_BINS;
    const u32 ngen = cj.ngenomes, pmlo = cj.pmlo, pmhi = cj.pmhi;
    if (tid < (u32)KH_TAG_MAX_OPS) {
        gtab[tid] = Readout::entry(jb, xj, ngen, tid);
        w.L.dupc[tid] = 0;
    }
    for (u32 i = tid; i < SKM_CROSS_BINS; i += NT) bins[i] = 0;
    const u32 nspill_all = listed ? w.side_records() : 0u;
    // one occupied entry
    auto count_entry = [&](u32 mlo, u32 mhi) __attribute__((always_inline)) { Readout::count(gtab, bins, nbins, ngen, pmlo, pmhi, mlo, mhi); };
    u32 st_full = 0, st_exp = 0, st_multi = 0;   // fullest slot seen, k-mer instances expanded, slots of several rounds (uniform)
    __syncthreads();
    for (u32 it = blockIdx.x; it < nwork; it += gridDim.x) {
        const u32 slot = listed ? jb.big_list[it] : it;
        if (slot >= jb.nslots) continue;   // (uniform; a listed slot is one the direct launch wrote)
        const u32 have = jb.cur2[slot];
        if (!listed) {   // uniform
            if (!have) continue;
            if (have > cap2) {   // an overfull slot: listed for the second launch, as the unions list theirs
                if (tid == 0) {
                    const u32 at = atomicAdd(jb.ctl + KH_SKM_CTL_LISTED, 1u);
                    if (at < jb.big_cap) jb.big_list[at] = slot;
                }
                continue;
            }
        }
        w.reset();
        __syncthreads();
        w.open(slot, have, listed, nspill_all);
        st_full = w.N > st_full ? w.N : st_full;
        st_exp += w.N;
        st_multi += w.R > 1u ? 1u : 0u;
        w.rounds(0u, 1u, [&]() __attribute__((always_inline)) { w.for_each_occupied(count_entry); });
        __syncthreads();   // (a slot without a round: scratch is written again only behind this)
    }
    __syncthreads();
    unsigned long long* __restrict__ rep = cj.bins + (u64)(blockIdx.x % cj.reps) * cj.nbins;
    for (u32 i = tid; i < nbins; i += NT)
        if (bins[i]) atomicAdd(&rep[i], (unsigned long long)bins[i]);
    if (tid < (u32)KH_TAG_MAX_OPS && w.L.dupc[tid]) atomicAdd(&jb.dup[tid], (unsigned long long)w.L.dupc[tid]);
    if (tid == 0) {
        if (st_full > Tr::T) atomicMax(jb.ctl + KH_SKM_CTL_FULLEST, st_full);
        if (st_exp) atomicAdd(jb.ctl + KH_SKM_CTL_EXPANDED, st_exp);
        if (st_multi) atomicAdd(jb.ctl + KH_SKM_CTL_MULTI, st_multi);
    }
}
// workgroups of k_skm_cross<Tr, Readout> a CU holds in the direct launch: by its LDS (160 KB a CU) and by its
// 1024 threads (sixteen waves: two workgroups when the kernel keeps to 64 VGPRs, which `vgprs64` says it does)
template <class Tr> constexpr u32 skm_cross_per_cu(bool vgprs64) {
    return vgprs64 && 2 * skm_cross_lds_bytes<Tr>(false) <= 160 * 1024 ? 2u : 1u;
}
template <class Tr> void skm_launch_cross(const KhSkmJob& job, const KhSkmCrossJob& cj, u32 grid, hipStream_t st) {
    if (!grid) return;
    skm_allow_lds(k_skm_cross<Tr, SkmCrossGroups>, skm_cross_lds_bytes<Tr>(true));
    hipLaunchKernelGGL((k_skm_cross<Tr, SkmCrossGroups>), dim3(grid), dim3(SKM_BIG_NT), skm_cross_lds_bytes<Tr>(cj.nlisted != 0u), st, job, cj);
}
template <class Tr> void skm_launch_pivot(const KhSkmJob& job, const KhSkmPivotJob& pj, u32 grid, hipStream_t st) {
    if (!grid) return;
    skm_allow_lds(k_skm_cross<Tr, SkmCrossOwn>, skm_cross_lds_bytes<Tr>(true));
    hipLaunchKernelGGL((k_skm_cross<Tr, SkmCrossOwn>), dim3(grid), dim3(SKM_BIG_NT), skm_cross_lds_bytes<Tr>(pj.cj.nlisted != 0u), st, job, pj);
}
