// khoice_amd — the two super-k-mer record formats, for the kernels of kh_skm.hip / kh_skm2.hip and for the host
// code that reads records (kh_engine.cpp: the side-list pieces).  No device code: fields and their accessors only.
#pragma once
#include <hip/hip_runtime.h>

#include "kh_common.h"

// A record is Q uint4.  Bits [0, 2(n+k-1)) are the bases of its n consecutive k-mers (base j at bits 2j, A0 C1 G2
// T3); its LAST 32-bit word holds, above the bases: the fine index of the slot inside its coarse bucket, the tag
// (the genome's operand number, or its group: 6 bits) and n, which fills the word up to bit 31.
template <u32 Q_, u32 FINE_SHIFT_, u32 FINE_BITS_> struct SkmRecFmt {
    static constexpr u32 Q = Q_;                                 // uint4 per record
    static constexpr u32 FINE_SHIFT = FINE_SHIFT_, FINE_BITS = FINE_BITS_;
    static constexpr u32 TAG_SHIFT = FINE_SHIFT + FINE_BITS, TAG_BITS = 6;
    static constexpr u32 HALF_SHIFT = TAG_SHIFT + TAG_BITS - 1;  // the tag's top bit: low or high half of the 64-bit genome mask
    static constexpr u32 N_SHIFT = TAG_SHIFT + TAG_BITS, N_BITS = 32 - N_SHIFT;
    static constexpr u32 N_MAX = (1u << N_BITS) - 1u;

    static __host__ __device__ __forceinline__ u32 n(u32 w) { return w >> N_SHIFT; }
    static __host__ __device__ __forceinline__ u32 tag(u32 w) { return (w >> TAG_SHIFT) & ((1u << TAG_BITS) - 1u); }
    static __host__ __device__ __forceinline__ u32 half(u32 w) { return (w >> HALF_SHIFT) & 1u; }
    static __host__ __device__ __forceinline__ u32 fine(u32 w) { return (w >> FINE_SHIFT) & ((1u << FINE_BITS) - 1u); }
    static __host__ __device__ __forceinline__ u32 bases(u32 w) { return w & ((1u << FINE_SHIFT) - 1u); }   // the last word without its header
    static __host__ __device__ __forceinline__ u32 header(u32 fine, u32 tag, u32 n) {   // ORed onto the last word of the bases (the scatter)
        return (fine << FINE_SHIFT) | (tag << TAG_SHIFT) | (n << N_SHIFT);
    }
    // "The same content" = the same piece of sequence, whatever genome it came from.  The merge of identical records keeps
    // ONE 32-bit mask per surviving record, i.e. one half of the 64-bit genome mask, so records whose tags lie in different
    // halves must not merge.  Hence two masks that differ in one bit: the HASH ignores all six tag bits (copies of both
    // halves walk one probe chain of the set of contents), the COMPARE ignores only the five low ones (the sixth, the mask
    // half, has to agree).
    static __host__ __device__ __forceinline__ u32 content_hash_word(u32 w) { return w & ~(((1u << TAG_BITS) - 1u) << TAG_SHIFT); }
    // (the last words' difference under the COMPARE rule, zero: the same; for callers that OR it with the other words')
    static __host__ __device__ __forceinline__ u32 content_diff(u32 wa, u32 wb) {
        return (wa ^ wb) & ~(((1u << (TAG_BITS - 1)) - 1u) << TAG_SHIFT);
    }
    static __host__ __device__ __forceinline__ bool same_content(u32 wa, u32 wb) { return content_diff(wa, wb) == 0u; }
};
using SkmRec1 = SkmRecFmt<1, 12, 9>;    // 16 bytes, k <= 32:       fine 12..20, tag 21..26, n 27..31
using SkmRec2 = SkmRecFmt<2, 10, 10>;   // 32 bytes, 33 <= k <= 63: fine 10..19, tag 20..25, n 26..31
