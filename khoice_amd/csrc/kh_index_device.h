// khoice_amd — the one search of the merged mask index (kh_index.hip), shared by its kernels.
#pragma once
#include "kh_device.h"

constexpr u64 KH_INDEX_ABSENT = ~0ull;

// The record of the mixed key `key` in the index, or KH_INDEX_ABSENT.  One directory read (two neighbouring words) says
// where the keys of the key's bucket lie; the bucket is searched by bisection, so the answer is exact however the keys
// spread: a bucket of thousands of keys costs log2 of them.  An empty index (n == 0: nb == 1, dir = {0, 0}) holds no key
// and reads none.
template <int W>
__device__ __forceinline__ u64 kh_index_find(const KhIndexView& v, const KmerKey<W> key, const int k) {
    const u32 b = kh_slot<W>(key, k, v.nb);                 // < nb
    const KmerKey<W>* __restrict__ keys = reinterpret_cast<const KmerKey<W>*>(v.keys);
    u64 lo = v.dir[b];
    const u64 end = v.dir[b + 1];                           // lo <= end <= n
    u64 hi = end;
    while (lo < hi) {
        const u64 mid = lo + ((hi - lo) >> 1);
        if (key_lt(keys[mid], key)) lo = mid + 1; else hi = mid;
    }
    return lo < end && key_eq(keys[lo], key) ? lo : KH_INDEX_ABSENT;
}
