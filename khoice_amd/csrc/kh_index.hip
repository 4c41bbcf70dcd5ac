// khoice_amd — the merged mask index for gfx950: the union of D sorted sets, every key with the mask of the sets that
// hold it, and a bucket directory over the mixed key space in front ("Merged mask index").  A lookup is
// one directory read and a bisection among the few keys of one bucket, whatever D is.
//
//   k_index_dir     one thread per record i in [0, n]: dir[b] = i for every bucket b in (slot(i - 1), slot(i)], with
//                   slot(-1) = -1 and slot(n) = nb.  The intervals cut [0, nb] without overlap: every entry is stored
//                   exactly once, nothing is zeroed first, no search
//   k_index_tag     one thread per (set d, record j of set d): the key's record in the index (kh_index_find), bit d
//                   ORed into its mask word by a global atomic without return
//   k_index_member  one thread per key of a probe set: one kh_index_find, mwords mask words out
//   k_read_index    the counterpart of k_read_masks (kh_reads.hip): the same tile, staging, decode and outcomes, but
//                   ONE kh_index_find per window instead of a search in every set
#include <hip/hip_runtime.h>

#include "kh_index_device.h"

constexpr u32 KH_IX_TILE = 256;               // positions per workgroup of k_read_index: the tile of k_read_masks
constexpr u32 KH_IX_STAGE = KH_IX_TILE + 64;  // 256 + k - 1 <= 319 bytes staged

template <int W>
__global__ __launch_bounds__(256) void k_index_dir(const KmerKey<W>* __restrict__ keys, const u64 n, const u32 nb, const int k,
                                                   u64* __restrict__ dir) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    const long long prev = i == 0 ? -1ll : (long long)kh_slot<W>(keys[i - 1], k, nb);
    const long long cur = i == n ? (long long)nb : (long long)kh_slot<W>(keys[i], k, nb);
    for (long long b = prev + 1; b <= cur; ++b) dir[b] = i;     // 0 <= b <= nb; a run of empty buckets is one thread's
}

template <int W>
__global__ __launch_bounds__(256) void k_index_tag(const KhIndexView v, u64* __restrict__ masks,
                                                   const KhSetView* __restrict__ sets, const int k, u32* __restrict__ err) {
    const u32 d = blockIdx.y;
    const KhSetView sv = sets[d];
    const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
    if (j >= sv.n) return;
    const u64 r = kh_index_find<W>(v, reinterpret_cast<const KmerKey<W>*>(sv.keys)[j], k);
    if (r == KH_INDEX_ABSENT) { atomicOr(err, 1u); return; }    // the union holds every key of every set
    atomicOr(reinterpret_cast<unsigned long long*>(masks + r * v.mwords + (d >> 6)), 1ull << (d & 63));
}

template <int W>
__global__ __launch_bounds__(256) void k_index_member(const KhIndexView v, const KmerKey<W>* __restrict__ probe, const u64 n,
                                                      const int k, u64* __restrict__ out) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 r = kh_index_find<W>(v, probe[i], k);
    for (u32 w = 0; w < v.mwords; ++w) out[i * v.mwords + w] = r == KH_INDEX_ABSENT ? 0ull : v.masks[r * v.mwords + w];
}

// index (in the whole call) of the read that holds position p of the batch: the last i with off[i] <= p
__device__ __forceinline__ u32 ix_read_of(const KhReadsJob& j, const u64 p) {
    u32 lo = 0, hi = j.nreads;   // off[lo] <= p < off[hi]
    while (hi - lo > 1) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (j.off[mid] <= p) lo = mid; else hi = mid;
    }
    return j.read0 + lo;
}

// The staging, the byte-by-byte decode and the three outcomes of k_read_masks, restated (kh_reads.hip keeps its own
// kernels as they compile today).  j.nwords == v.mwords; j.sets is not read.
template <int W>
__global__ __launch_bounds__(256) void k_read_index(const KhReadsJob j, const KhIndexView v) {
    __shared__ u8 raw[KH_IX_STAGE];
    const u32 k = (u32)j.k;
    const u64 p0 = (u64)blockIdx.x * KH_IX_TILE;            // < npos: the grid is ceil(npos / 256)
    const u64 left = j.npos - p0;
    const u32 nst = left < KH_IX_TILE + k - 1 ? (u32)left : KH_IX_TILE + k - 1;
    for (u32 i = threadIdx.x; i < nst; i += KH_IX_TILE) raw[i] = j.buf[p0 + i];
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
        atomicMin(&j.ctl[1], ix_read_of(j, p));
        for (u32 w = 0; w < j.nwords; ++w) out[w] = 0;
        return;
    }
    const KmerKey<W> key = kh_mix(key_lt(r, f) ? r : f, (int)k);
    const u64 rec = kh_index_find<W>(v, key, (int)k);
    if (rec == KH_INDEX_ABSENT) {
        for (u32 w = 0; w < j.nwords; ++w) out[w] = 0;
    } else {
        const u64* __restrict__ cell = v.masks + rec * j.nwords;
        for (u32 w = 0; w < j.nwords; ++w) out[w] = cell[w];
    }
    if (j.check && !kh_set_holds<W>(*j.check, key, (u64)kh_top32(key, (int)k) << 32)) atomicMin(&j.ctl[2], ix_read_of(j, p));
}

template <int W> static const KmerKey<W>* ix_keys(const void* p) { return reinterpret_cast<const KmerKey<W>*>(p); }

void kh_launch_index_dir(int W, const KhIndexView& v, u64* dir, int k, hipStream_t st) {
    const u32 grid = (u32)((v.n + 1 + 255) / 256);
    if (W == 1) hipLaunchKernelGGL((k_index_dir<1>), dim3(grid), dim3(256), 0, st, ix_keys<1>(v.keys), v.n, v.nb, k, dir);
    else hipLaunchKernelGGL((k_index_dir<2>), dim3(grid), dim3(256), 0, st, ix_keys<2>(v.keys), v.n, v.nb, k, dir);
}

void kh_launch_index_tag(int W, const KhIndexView& v, u64* masks, const KhSetView* sets, u32 nsets, u64 max_n, int k, u32* err,
                         hipStream_t st) {
    if (!max_n || !nsets) return;
    const dim3 grid((u32)((max_n + 255) / 256), nsets);
    if (W == 1) hipLaunchKernelGGL((k_index_tag<1>), grid, dim3(256), 0, st, v, masks, sets, k, err);
    else hipLaunchKernelGGL((k_index_tag<2>), grid, dim3(256), 0, st, v, masks, sets, k, err);
}

void kh_launch_index_member(int W, const KhIndexView& v, const void* probe, u64 n, int k, u64* out, hipStream_t st) {
    if (!n) return;
    const u32 grid = (u32)((n + 255) / 256);
    if (W == 1) hipLaunchKernelGGL((k_index_member<1>), dim3(grid), dim3(256), 0, st, v, ix_keys<1>(probe), n, k, out);
    else hipLaunchKernelGGL((k_index_member<2>), dim3(grid), dim3(256), 0, st, v, ix_keys<2>(probe), n, k, out);
}

void kh_launch_read_index(int W, const KhReadsJob& job, const KhIndexView& v, hipStream_t st) {
    if (!job.npos) return;
    const u32 grid = (u32)((job.npos + KH_IX_TILE - 1) / KH_IX_TILE);
    if (W == 1) hipLaunchKernelGGL((k_read_index<1>), dim3(grid), dim3(KH_IX_TILE), 0, st, job, v);
    else hipLaunchKernelGGL((k_read_index<2>), dim3(grid), dim3(KH_IX_TILE), 0, st, job, v);
}
