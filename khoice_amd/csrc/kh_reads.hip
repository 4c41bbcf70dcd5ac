// khoice_amd — read-level classification votes (experiment type 6, src/merge_lists.py:151-183) for gfx950.
//
// The reference walks every read's k-mers in text order; a k-mer that the datasets M hold adds 1/len(M) to the vote
// of every dataset in M; the read goes to a dataset of the highest vote, drawn by random.choice among the ties.  The
// device computes everything but the draw, bit for bit: the votes (an ordered sum of doubles), the number of k-mers
// no dataset holds, and the set of datasets that tie for the maximum.
//
//   k_read_masks   one thread per text position: the window's canonical key, mixed, searched in every set
//                  (kh_set_holds, the search of k_membership) -> nwords mask words per position
//   k_read_lookup  the same for k <= 13 without a search: the window's canonical code addresses the mask table that
//                  k_bmp_group_masks (kh_bmp.hip) made of the groups' presence bitmaps
//   k_read_fold    one wave per read, reads claimed from a counter: the masks of a read in window order, 64 at a
//                  time; lane d owns dataset d (d, d + 64, ... beyond 64 sets); v += inv[L] — additions only, one
//                  rounding each, in window order, which is what CPython does with `votes[m] += 1/len(matches)`
//
// Text layout: read i is buf[off[i], off[i + 1] - 1) and a '\n' follows every read.  A window that touches a '\n'
// does not exist; a window that touches any other byte outside upper-case ACGT is an error (the reference's KeyError
// at :66) and records its read.  decode16 of kh_device.h folds case, so it cannot tell 'a' from 'A'; the windows
// here are decoded byte by byte from the staged tile instead.
#include <hip/hip_runtime.h>

#include "kh_device.h"
#include "kh_launch.h"

constexpr u32 KH_RD_TILE = 256;           // positions per workgroup of k_read_masks
constexpr u32 KH_RD_STAGE = KH_RD_TILE + 64;   // 256 + k - 1 <= 319 bytes staged
constexpr u32 KH_RD_FOLD_WAVES = 4;

// index (in the whole call) of the read that holds position p of the batch: the last i with off[i] <= p
__device__ __forceinline__ u32 read_of(const KhReadsJob& j, const u64 p) {
    u32 lo = 0, hi = j.nreads;   // off[lo] <= p < off[hi]
    while (hi - lo > 1) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (j.off[mid] <= p) lo = mid; else hi = mid;
    }
    return j.read0 + lo;
}

template <int W>
__global__ __launch_bounds__(256) void k_read_masks(const KhReadsJob j) {
    __shared__ u8 raw[KH_RD_STAGE];
    const u32 k = (u32)j.k;
    const u64 p0 = (u64)blockIdx.x * KH_RD_TILE;            // < npos: the grid is ceil(npos / 256)
    const u64 left = j.npos - p0;
    const u32 nst = left < KH_RD_TILE + k - 1 ? (u32)left : KH_RD_TILE + k - 1;
    for (u32 i = threadIdx.x; i < nst; i += KH_RD_TILE) raw[i] = j.buf[p0 + i];
    __syncthreads();
    const u32 t = threadIdx.x;
    if (t + k > nst) return;                                // the window would run past the text
    const u64 p = p0 + t;
    KmerKey<W> f, r;                                        // the window and its reverse complement
    f.lo = r.lo = 0;
    if constexpr (W == 2) f.hi = r.hi = 0;
    bool sep = false, bad = false;
    for (u32 i = 0; i < k; ++i) {
        const u32 ch = raw[t + i];
        const u32 code = ((ch >> 1) ^ (ch >> 2)) & 3u;      // A C G T -> 0 1 2 3
        sep |= ch == (u32)'\n';
        bad |= ch != ((0x54474341u >> (8 * code)) & 0xffu); // "ACGT"[code]
        const u64 comp = 3u - code;
        if constexpr (W == 2) {
            f.hi = (f.hi << 2) | (f.lo >> 62);
            if (i >= 32) r.hi |= comp << (2 * (i - 32));
        }
        f.lo = (f.lo << 2) | code;
        if (i < 32) r.lo |= comp << (2 * i);
    }
    if (sep) return;                                        // no window here: nothing written, the fold never looks
    u64* __restrict__ out = j.masks + p * j.nwords;
    if (bad) {
        atomicMin(&j.ctl[1], read_of(j, p));
        for (u32 w = 0; w < j.nwords; ++w) out[w] = 0;
        return;
    }
    const KmerKey<W> key = kh_mix(key_lt(r, f) ? r : f, (int)k);
    const u64 top = (u64)kh_top32(key, (int)k) << 32;
    for (u32 w = 0; w < j.nwords; ++w) {
        u64 m = 0;
        const u32 dend = min(j.nsets, (w + 1) * 64);
        for (u32 d = w * 64; d < dend; ++d)
            if (kh_set_holds<W>(j.sets[d], key, top)) m |= 1ull << (d & 63);
        out[w] = m;
    }
    if (j.check && !kh_set_holds<W>(*j.check, key, top)) atomicMin(&j.ctl[2], read_of(j, p));
}

// The masks of k <= 13 by direct address: the staging, the byte-by-byte decode and the three outcomes of k_read_masks
// (the decode restated on 32-bit codes; k_read_masks works on KmerKey<W>), but the canonical code is not mixed and not
// searched for: it indexes the mask table that k_bmp_group_masks made of the groups' presence bitmaps, first base most
// significant, A C G T = 0 1 2 3, the smaller of the two strands — the numbering of k_bmp_build.
__global__ __launch_bounds__(256) void k_read_lookup(const KhReadsJob j, const u64* __restrict__ table) {
    __shared__ u8 raw[KH_RD_STAGE];
    const u32 k = (u32)j.k;
    const u64 p0 = (u64)blockIdx.x * KH_RD_TILE;            // < npos: the grid is ceil(npos / 256)
    const u64 left = j.npos - p0;
    const u32 nst = left < KH_RD_TILE + k - 1 ? (u32)left : KH_RD_TILE + k - 1;
    for (u32 i = threadIdx.x; i < nst; i += KH_RD_TILE) raw[i] = j.buf[p0 + i];
    __syncthreads();
    const u32 t = threadIdx.x;
    if (t + k > nst) return;                                // the window would run past the text
    const u64 p = p0 + t;
    u32 f = 0, r = 0;                                       // the window and its reverse complement: 2 k <= 26 bits
    bool sep = false, bad = false;
    for (u32 i = 0; i < k; ++i) {
        const u32 ch = raw[t + i];
        const u32 code = ((ch >> 1) ^ (ch >> 2)) & 3u;      // A C G T -> 0 1 2 3
        sep |= ch == (u32)'\n';
        bad |= ch != ((0x54474341u >> (8 * code)) & 0xffu); // "ACGT"[code]
        f = (f << 2) | code;
        r |= (3u - code) << (2 * i);
    }
    if (sep) return;                                        // no window here: nothing written, the fold never looks
    u64* __restrict__ out = j.masks + p * j.nwords;
    if (bad) {
        atomicMin(&j.ctl[1], read_of(j, p));
        for (u32 w = 0; w < j.nwords; ++w) out[w] = 0;
        return;
    }
    const u64* __restrict__ cell = table + (u64)(f < r ? f : r) * j.nwords;
    for (u32 w = 0; w < j.nwords; ++w) out[w] = cell[w];
}

__device__ __forceinline__ u64 readlane64(const u64 v, const u32 i) {
    const u32 lo = (u32)__builtin_amdgcn_readlane((int)(u32)v, (int)i);
    const u32 hi = (u32)__builtin_amdgcn_readlane((int)(u32)(v >> 32), (int)i);
    return ((u64)hi << 32) | lo;
}

// ONE: at most 64 sets, the vote of lane d's dataset stays in a register; otherwise the votes of a wave live in its
// own stripe of LDS throughout (vl[wave][word * 64 + lane]: a lane touches only its own cells, no barrier).
template <bool ONE>
__global__ __launch_bounds__(64 * KH_RD_FOLD_WAVES) void k_read_fold(const KhReadsJob j, const double* __restrict__ inv,
                                                                    u64* __restrict__ tie, double* __restrict__ votes,
                                                                    u32* __restrict__ unmatched) {
    extern __shared__ double vl[];
    const u32 lane = lane_id(), nwords = j.nwords, k = (u32)j.k;
    double* mine = vl + (size_t)(threadIdx.x >> 6) * nwords * 64;
    for (;;) {
        u32 r = 0;
        if (lane == 0) r = atomicAdd(&j.ctl[0], 1u);
        r = (u32)__builtin_amdgcn_readfirstlane((int)r);
        if (r >= j.nreads) break;
        const u64 b = j.off[r];
        const u64 len = j.off[r + 1] - 1 - b;
        const u64 nwin = len >= k ? len - k + 1 : 0;
        double v = 0.0;
        if constexpr (!ONE)
            for (u32 w = 0; w < nwords; ++w) mine[w * 64 + lane] = 0.0;
        u32 unm = 0;
        for (u64 c0 = 0; c0 < nwin; c0 += 64) {
            const u32 cnt = nwin - c0 < 64 ? (u32)(nwin - c0) : 64u;
            const u64* __restrict__ mp = j.masks + (b + c0 + lane) * nwords;   // lane i: window c0 + i
            u32 L = 0;                                                         // len(M) of lane i's window
            u64 m0 = 0;
            if (lane < cnt) {
                m0 = mp[0];
                L = (u32)__popcll(m0);
                if constexpr (!ONE)
                    for (u32 w = 1; w < nwords; ++w) L += (u32)__popcll(mp[w]);
            }
            if constexpr (ONE) {
                for (u32 i = 0; i < cnt; ++i) {
                    const u32 Li = (u32)__builtin_amdgcn_readlane((int)L, (int)i);
                    if (!Li) { ++unm; continue; }
                    const u64 mi = readlane64(m0, i);
                    if ((mi >> lane) & 1) v += inv[Li];
                }
            } else {
                for (u32 w = 0; w < nwords; ++w) {   // words are different datasets: each sum keeps its window order
                    const u64 m = w == 0 ? m0 : (lane < cnt ? mp[w] : 0ull);
                    double acc = mine[w * 64 + lane];
                    for (u32 i = 0; i < cnt; ++i) {
                        const u32 Li = (u32)__builtin_amdgcn_readlane((int)L, (int)i);
                        if (!Li) { unm += w == 0; continue; }
                        const u64 mi = readlane64(m, i);
                        if ((mi >> lane) & 1) acc += inv[Li];
                    }
                    mine[w * 64 + lane] = acc;
                }
            }
        }
        // exact maximum over the datasets (votes are >= 0; lanes past nsets stay out with -1)
        double mx = -1.0;
        if constexpr (ONE) {
            if (lane < j.nsets) mx = v;
        } else {
            for (u32 w = 0; w < nwords; ++w)
                if (w * 64 + lane < j.nsets) mx = fmax(mx, mine[w * 64 + lane]);
        }
        for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
        for (u32 w = 0; w < nwords; ++w) {
            const u32 d = w * 64 + lane;
            const double vw = ONE ? v : mine[w * 64 + lane];
            const u64 tm = __ballot(d < j.nsets && vw == mx);
            if (lane == 0) tie[(u64)r * nwords + w] = tm;
            if (votes && d < j.nsets) votes[(u64)r * j.nsets + d] = vw;
        }
        if (unmatched && lane == 0) unmatched[r] = unm;
    }
}

void kh_launch_read_masks(int W, const KhReadsJob& job, hipStream_t st) {
    if (!job.npos) return;
    const u32 grid = (u32)((job.npos + KH_RD_TILE - 1) / KH_RD_TILE);
    if (W == 1) hipLaunchKernelGGL((k_read_masks<1>), dim3(grid), dim3(KH_RD_TILE), 0, st, job);
    else hipLaunchKernelGGL((k_read_masks<2>), dim3(grid), dim3(KH_RD_TILE), 0, st, job);
}

void kh_launch_read_lookup(const KhReadsJob& job, const u64* table, hipStream_t st) {
    if (!job.npos) return;
    const u32 grid = (u32)((job.npos + KH_RD_TILE - 1) / KH_RD_TILE);
    hipLaunchKernelGGL(k_read_lookup, dim3(grid), dim3(KH_RD_TILE), 0, st, job, table);
}

void kh_launch_read_fold(const KhReadsJob& job, const double* inv, u64* tie, double* votes, u32* unmatched, u32 grid,
                         hipStream_t st) {
    if (!job.nreads) return;
    if (job.nwords == 1)
        hipLaunchKernelGGL((k_read_fold<true>), dim3(grid), dim3(64 * KH_RD_FOLD_WAVES), 0, st, job, inv, tie, votes, unmatched);
    else
        hipLaunchKernelGGL((k_read_fold<false>), dim3(grid), dim3(64 * KH_RD_FOLD_WAVES),
                           (size_t)KH_RD_FOLD_WAVES * job.nwords * 64 * sizeof(double), st, job, inv, tie, votes, unmatched);
}
