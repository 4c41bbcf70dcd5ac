// khoice_amd — presence-bitmap forms of the fused experiment types 1-4 and 6 for small k (gfx950).
//
// A k-mer of k <= 13 is a number below 2^26: "which genomes hold it" is one bit per genome in a directly addressed
// bitmap of 4^k bits, and every histogram of the forms is a count over those bits.  There is no genome mask: any number
// of genomes and groups (up to 1023 per counter) is answered in one pass.
//
// Two kernels read text, tile by tile with the same staging, written out in each:
//   k_bmp_build<K>  text -> presence bitmaps, one partial bitmap per split of an operand (every form)
//   k_bmp_count<K>  text -> how often every code occurs in a pivot (type 4)
// Four kernels walk the bitmaps with the same walk, written out in each (the comment above k_bmp_readout describes it):
// a lane owns one 64-bit word, the operands' words are handed to wave 0, which counts them with bit-sliced counters
// into bins in LDS.
//   k_bmp_readout   type 1: the bins per count of every group and the bins of the counter over groups
//   k_bmp_pivot     type 2: a pivot's word masks the counter of its group, then the counter over groups
//   k_bmp_cross     type 3: every pivot's word, kept in LDS, masks the counter of every group
//   k_bmp_present   types 4 and 6: the within-group bins, the groups' presence words, the pivots' words and popcounts
// And two kernels of their own shape:
//   k_bmp_member    type 4: one (membership mask, count) record per pivot k-mer in code order
//   k_bmp_group_masks  type 6: the groups' presence words transposed into one mask of groups per code
// The launchers share one dispatch on k (bmp_for_k) and one body for the four walk kernels (launch_walk).
#include <type_traits>

#include "kh_device.h"
#include "kh_launch.h"

namespace {

constexpr u32 BMP_NT = 1024;          // threads of a build workgroup: with the 128 KiB bitmap one workgroup fills a CU
constexpr u32 BMP_CHUNK = 16;         // positions per thread and round: one staged word (+ the next for the k - 1 halo)
constexpr u32 BMP_FETCH = (KH_BMP_TILE / BMP_CHUNK + 1 + BMP_NT - 1) / BMP_NT;   // staged words a thread fetches per tile
constexpr u32 BMP_PREFILTER_RANGES = 16;   // from this many ranges on, candidates are picked by their leading bases first
constexpr u32 BMP_MAX_LEAD = 5;       // leading bases of a range at most (k = 13 with ranges of 2^16 codes)
// LDS of a tile's staging: [code: tile_pos / 16 + 1 u32][bad16: tile_pos / 16 + 1 u16]
constexpr size_t bmp_stage_lds_bytes(u32 tile_pos) { return ((size_t)(tile_pos / BMP_CHUNK + 1) * 6 + 15) & ~(size_t)15; }

// ------------------------------------------------------------------------------------------
// k_bmp_build
// LDS: [bitmap: rw u64][code: tile_pos / 16 + 1 u32][bad16: tile_pos / 16 + 1 u16][count: 1 u32]
// ------------------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(BMP_NT) void k_bmp_build(const KhBmpJob jb) {
    extern __shared__ __attribute__((aligned(16))) u8 lds_raw[];
    const u32 tid = threadIdx.x;
    const u32 rw = 1u << (jb.range_bits - 6);                    // 64-bit words of this workgroup's range
    const u32 nranges = jb.nranges;
    const u32 range = blockIdx.x % nranges, si = blockIdx.x / nranges;
    const KhBmpSplit sp = jb.splits[si];
    const u32 twords = jb.tile_pos / BMP_CHUNK;                  // chunks of a tile; one more word is staged for the halo
    u32* bm = reinterpret_cast<u32*>(lds_raw);
    u32* code = reinterpret_cast<u32*>(lds_raw + 8 * (size_t)rw);
    u16* bad16 = reinterpret_cast<u16*>(code + twords + 1);
    u32* total = reinterpret_cast<u32*>(lds_raw + 8 * (size_t)rw + (((size_t)(twords + 1) * 6 + 15) & ~(size_t)15));

    if (rw >= 2) {
        uint4* b4 = reinterpret_cast<uint4*>(bm);
        for (u32 i = tid; i < rw / 2; i += BMP_NT) b4[i] = make_uint4(0, 0, 0, 0);
    } else if (tid < 2) {
        bm[tid] = 0;
    }
    if (tid == 0) *total = 0;

    constexpr u32 KMASK = (1u << (2 * K)) - 1u;                  // K <= 13: 26 bits
    constexpr u64 PAIRS = 0x5555555555555555ull;
    const u32 rlo = range << jb.range_bits;                      // first code of the range
    const u32 rmask = (1u << jb.range_bits) - 1u;                // (range_bits <= 2K: codes of other ranges differ above it)
    // Many ranges (k = 12: sixteen passes over the text): the range is the leading `nlead` bases of the canonical
    // code, i.e. the first bases of the k-mer or the complements of its last ones.  Both are compared for all
    // positions of a chunk at once on the staged 2-bit codes, and only the candidates (2 in `nranges` positions) get
    // their codes worked out.  lead_fw[d] / lead_rc[d]: base d of the range / its complement in every pair of bits.
    const u32 lead_bits = 2 * K - jb.range_bits;
    const u32 nlead = (lead_bits & 1u) || nranges < BMP_PREFILTER_RANGES ? 0u : lead_bits / 2;
    u64 lead_fw[BMP_MAX_LEAD], lead_rc[BMP_MAX_LEAD];
#pragma unroll
    for (u32 d = 0; d < BMP_MAX_LEAD; ++d) {
        const u32 v = d < nlead ? (range >> (2 * (nlead - 1 - d))) & 3u : 0u;
        lead_fw[d] = PAIRS * v;
        lead_rc[d] = PAIRS * (3u - v);
    }
    // the raw bytes of the next tile are fetched while the current one is worked on
    const u32 swords = twords + 1;
    kh_u32x4 pre[BMP_FETCH];
    auto fetch = [&](const u64 t0) {
#pragma unroll
        for (u32 i = 0; i < BMP_FETCH; ++i) {
            const u32 w = tid + i * BMP_NT;
            pre[i] = codes_fetch(sp.seq, sp.len, t0 + 16ull * w, w < swords, jb.splits);
        }
    };
    u32 nvalid = 0;
    if (sp.p0 < sp.p1) fetch(sp.p0);
    for (u64 t0 = sp.p0; t0 < sp.p1; t0 += jb.tile_pos) {
        __syncthreads();                                         // the bitmap is cleared; the last tile has been read
#pragma unroll
        for (u32 i = 0; i < BMP_FETCH; ++i) {
            const u32 w = tid + i * BMP_NT;
            u32 codes, bad;
            codes_decode(pre[i], sp.seq, sp.len, t0 + 16ull * w, codes, bad);
            if (w < swords) {
                code[w] = codes;
                bad16[w] = (u16)bad;
            }
        }
        __syncthreads();
        if (t0 + jb.tile_pos < sp.p1) fetch(t0 + jb.tile_pos);
        const u64 tend = t0 + jb.tile_pos < sp.p1 ? t0 + jb.tile_pos : sp.p1;
        const u32 nch = (u32)((tend - t0 + BMP_CHUNK - 1) / BMP_CHUNK);
        for (u32 c = tid; c < nch; c += BMP_NT) {
            // bases 16c .. 16c + 31 of the tile: base j at bits 2j; a position breaks where any of its k bases does.
            // (A split ends at a multiple of 16 or at the genome's last position, behind which every base is flagged.)
            const u64 cw = (u64)code[c] | ((u64)code[c + 1] << 32);
            u32 inv = (u32)bad16[c] | ((u32)bad16[c + 1] << 16);
            {
                u32 w = 1;
#pragma unroll
                for (int s = 0; s < 3; ++s)
                    if (2 * w <= (u32)K) { inv |= inv >> w; w *= 2; }
                inv |= inv >> ((u32)K - w);
            }
            const u32 valid = ~inv & 0xffffu;
            nvalid += __builtin_popcount(valid);
            if (!valid) continue;
            const u64 fwd = kh_revpairs64(cw);                   // base j at bits 62 - 2j: first base most significant
            const u64 rcw = ~cw;                                 // the complement of base j + m at bits 2(j + m): the reverse complement's digit m
            if (nlead) {
                u64 cf = PAIRS, cr = PAIRS;                      // bit 2j: position j may have its canonical code in the range
#pragma unroll
                for (u32 d = 0; d < BMP_MAX_LEAD; ++d) {
                    if (d < nlead) {
                        const u64 tf = cw ^ lead_fw[d], tr = cw ^ lead_rc[d];
                        cf &= ~(tf | (tf >> 1)) >> (2 * d);
                        cr &= ~(tr | (tr >> 1)) >> (2 * ((u32)K - 1 - d));
                    }
                }
                // candidates that are valid positions: bit 2j of m.  The code of position j is cut out of a 64-bit
                // word by a shift below 32 and a truncation: one v_alignbit each for the two strands.
                u32 vp = valid;                                  // bit j -> bit 2j
                vp = (vp | (vp << 8)) & 0x00ff00ffu;
                vp = (vp | (vp << 4)) & 0x0f0f0f0fu;
                vp = (vp | (vp << 2)) & 0x33333333u;
                vp = (vp | (vp << 1)) & 0x55555555u;
                u32 m = (u32)(cf | cr) & vp;
                const u64 fwk = fwd >> (64 - 2 * (15 + K));      // the forward code of position j at bits 2(15 - j)
                const u32 fl = (u32)fwk, fh = (u32)(fwk >> 32), rl = (u32)rcw, rh = (u32)(rcw >> 32);
                while (m) {
                    const u32 t = (u32)__builtin_ctz(m);         // 2j
                    m &= m - 1;
                    const u32 fw = __builtin_amdgcn_alignbit(fh, fl, 30u - t) & KMASK;
                    const u32 rc = __builtin_amdgcn_alignbit(rh, rl, t) & KMASK;
                    const u32 canon = fw < rc ? fw : rc;
                    if ((canon >> jb.range_bits) == range) {
                        const u32 b = canon & rmask;
                        atomicOr(&bm[b >> 5], 1u << (b & 31u));
                    }
                }
                continue;
            }
#pragma unroll
            for (u32 j = 0; j < BMP_CHUNK; ++j) {
                const u32 fw = (u32)(fwd >> (64 - 2 * (j + K))) & KMASK;
                const u32 rc = (u32)(rcw >> (2 * j)) & KMASK;
                const u32 canon = fw < rc ? fw : rc;
                if (((valid >> j) & 1u) && (canon & ~rmask) == rlo) {
                    const u32 b = canon & rmask;
                    atomicOr(&bm[b >> 5], 1u << (b & 31u));
                }
            }
        }
    }
    // valid positions of the genome (the `kmers` statistic): counted once, by the workgroups of range 0
    if (range == 0) {
        const u32 wsum = wave_scan_add(nvalid);
        if (lane_id() == KH_WAVE - 1 && wsum) atomicAdd(total, wsum);
    }
    __syncthreads();
    if (range == 0 && tid == 0 && *total) atomicAdd(&jb.inst[sp.op], (unsigned long long)*total);
    // every word of the range, zeros included
    u64* out = jb.partial + (size_t)si * jb.nwords + (size_t)range * rw;
    if (rw >= 2) {
        const uint4* b4 = reinterpret_cast<const uint4*>(bm);
        uint4* o4 = reinterpret_cast<uint4*>(out);
        for (u32 i = tid; i < rw / 2; i += BMP_NT) o4[i] = b4[i];
    } else if (tid == 0) {
        out[0] = (u64)bm[0] | ((u64)bm[1] << 32);
    }
}

// ------------------------------------------------------------------------------------------
// k_bmp_readout
// LDS: [bins: nbins + nops u32][gx: 2 x waves x 64 u64]  (bins of the groups, the across-group bins, then one counter
// per genome; the genome words the waves hand to wave 0)
// ------------------------------------------------------------------------------------------
constexpr int BMP_SLICES = 10;        // counts up to 1023: genomes of a group, groups

// x (one bit per code) is added to the bit-sliced counter c: ripple carry over the first `ns` slices
__device__ __forceinline__ void slices_add(u64 (&c)[BMP_SLICES], u64 x, const u32 ns) {
#pragma unroll
    for (int s = 0; s < BMP_SLICES; ++s) {
        if ((u32)s < ns) {   // wave-uniform: the slices stay in registers
            const u64 t = c[s] & x;
            c[s] ^= x;
            x = t;
        }
    }
}
// codes whose counter equals v
__device__ __forceinline__ u64 slices_equal(const u64 (&c)[BMP_SLICES], const u32 v, const u32 ns) {
    u64 eq = ~0ull;
#pragma unroll
    for (int s = 0; s < BMP_SLICES; ++s)
        if ((u32)s < ns) eq &= ((v >> s) & 1u) ? c[s] : ~c[s];
    return eq;
}
__device__ __forceinline__ u32 bit_length(u32 n) { return 32u - (u32)__builtin_clz(n | 1u); }

// the sum of v over the wave is added to *bin by one lane (all lanes of the wave must be here)
__device__ __forceinline__ void wave_add_to_bin(u32* bin, const u32 v) {
    const u32 sum = wave_scan_add(v);
    if (lane_id() == KH_WAVE - 1 && sum) atomicAdd(bin, sum);
}

// blockDim = (64, wy): the 64 lanes of a wave own 64 consecutive words.  The genomes are taken wy at a time: wave y ORs
// the splits of genome i0 + y (so the loads of wy genomes are in flight together, not one genome's after the other's)
// and leaves the word in LDS; wave 0 then counts the wy words in order.  One barrier per round, two buffers in turn:
// round n + 2 writes the buffer of round n only behind barrier n + 1, which wave 0 reaches when it has counted round n.
__global__ __launch_bounds__(1024) void k_bmp_readout(const KhBmpJob jb) {
    extern __shared__ __attribute__((aligned(16))) u8 lds_raw[];
    u32* bins = reinterpret_cast<u32*>(lds_raw);
    const u32 nb = jb.nbins + jb.nops;
    u64* gx = reinterpret_cast<u64*>(lds_raw + ((4 * (size_t)nb + 15) & ~(size_t)15));   // [2][wy][64]
    const u32 lane = threadIdx.x, y = threadIdx.y, wy = blockDim.y;
    const u32 tid = y * KH_WAVE + lane, nt = wy * KH_WAVE;
    for (u32 i = tid; i < nb; i += nt) bins[i] = 0;
    __syncthreads();
    const u32 asl = bit_length(jb.ngroups);
    u32 round = 0;
    for (u64 wb = blockIdx.x; wb * KH_WAVE < jb.nwords; wb += gridDim.x) {
        const u64 w = wb * KH_WAVE + lane;
        const bool active = w < jb.nwords;
        // wave 0: the group being counted, its bit-sliced counter c, and the counter a over groups
        u32 g = 0;
        KhBmpGroup gr = jb.groups[0];
        u32 ns = bit_length(gr.size);
        u64 a[BMP_SLICES], c[BMP_SLICES], any = 0;
#pragma unroll
        for (int s = 0; s < BMP_SLICES; ++s) a[s] = c[s] = 0;
        for (u32 i0 = 0; i0 < jb.nops; i0 += wy, ++round) {
            u64 x = 0;
            if (i0 + y < jb.nops && active) {
                const KhBmpOp op = jb.ops[i0 + y];
                const u64* p = jb.partial + (size_t)op.split0 * jb.nwords + w;
#pragma unroll 8
                for (u32 s = 0; s < op.nsplits; ++s) x |= p[(size_t)s * jb.nwords];
            }
            u64* buf = gx + (size_t)(round & 1u) * wy * KH_WAVE;
            buf[y * KH_WAVE + lane] = x;
            __syncthreads();
            if (y != 0) continue;
            const u32 n = jb.nops - i0 < wy ? jb.nops - i0 : wy;
            for (u32 j = 0; j < n; ++j) {
                const u32 i = i0 + j;
                const u64 xx = buf[j * KH_WAVE + lane];
                wave_add_to_bin(&bins[jb.nbins + i], (u32)__builtin_popcountll(xx));   // the genome's distinct k-mers
                any |= xx;
                slices_add(c, xx, ns);
                if (i + 1 == gr.first + gr.size) {   // the group is complete: one bin per count, and its presence counted
                    for (u32 v = 1; v <= gr.size; ++v)
                        wave_add_to_bin(&bins[gr.bin0 + v], (u32)__builtin_popcountll(slices_equal(c, v, ns)));
                    slices_add(a, any, asl);
                    any = 0;
#pragma unroll
                    for (int s = 0; s < BMP_SLICES; ++s) c[s] = 0;
                    if (++g < jb.ngroups) {
                        gr = jb.groups[g];
                        ns = bit_length(gr.size);
                    }
                }
            }
        }
        if (y == 0)
            for (u32 v = 1; v <= jb.ngroups; ++v)
                wave_add_to_bin(&bins[jb.abase + v], (u32)__builtin_popcountll(slices_equal(a, v, asl)));
    }
    __syncthreads();
    unsigned long long* rep = jb.hist + (size_t)(blockIdx.x % jb.reps) * nb;
    for (u32 i = tid; i < nb; i += nt)
        if (bins[i]) atomicAdd(&rep[i], (unsigned long long)bins[i]);
}

// ------------------------------------------------------------------------------------------
// k_bmp_pivot
// LDS: as k_bmp_readout, [bins: nbins + nops u32][gx: 2 x waves x 64 u64]
// ------------------------------------------------------------------------------------------
// Experiment type 2 with the walk of k_bmp_readout.  The operands of a group are its genomes, then the pivots held
// out of it.  First phase: a genome's word goes into the group's counter c and into `any`; behind the last genome `any`
// is kept in present[group] (groups with pivots only) and added to the counter a over groups; a pivot's word P is
// counted against c, which still stands: bin(pivot, v) += popcount(P & (c == v)), v = 0 .. size.  Second phase, a
// complete: the pivots alone are handed over again, and with G = present[group], read back by the lane that stored it,
// the other groups holding a code are a - 1 where G is set, else a.
__global__ __launch_bounds__(1024) void k_bmp_pivot(const KhBmpPivotJob jb) {
    extern __shared__ __attribute__((aligned(16))) u8 lds_raw[];
    u32* bins = reinterpret_cast<u32*>(lds_raw);
    const u32 nb = jb.nbins + jb.nops;
    u64* gx = reinterpret_cast<u64*>(lds_raw + ((4 * (size_t)nb + 15) & ~(size_t)15));   // [2][wy][64]
    const u32 lane = threadIdx.x, y = threadIdx.y, wy = blockDim.y;
    const u32 tid = y * KH_WAVE + lane, nt = wy * KH_WAVE;
    for (u32 i = tid; i < nb; i += nt) bins[i] = 0;
    __syncthreads();
    const u32 asl = bit_length(jb.ngroups);
    u32 round = 0;
    // wave y: the word of operand `i` (none: zero) into this round's buffer
    auto hand_over = [&](const bool have, const u32 i, const u64 w) {
        u64 x = 0;
        if (have) {
            const KhBmpOp op = jb.ops[i];
            const u64* p = jb.partial + (size_t)op.split0 * jb.nwords + w;
#pragma unroll 8
            for (u32 s = 0; s < op.nsplits; ++s) x |= p[(size_t)s * jb.nwords];
        }
        u64* buf = gx + (size_t)(round & 1u) * wy * KH_WAVE;
        buf[y * KH_WAVE + lane] = x;
        __syncthreads();
        return buf;
    };
    for (u64 wb = blockIdx.x; wb * KH_WAVE < jb.nwords; wb += gridDim.x) {
        const u64 w = wb * KH_WAVE + lane;
        const bool active = w < jb.nwords;
        u32 g = 0;
        KhBmpPivotGroup gr = jb.groups[0];
        u32 ns = bit_length(gr.size);
        u64 a[BMP_SLICES], c[BMP_SLICES], any = 0;
#pragma unroll
        for (int s = 0; s < BMP_SLICES; ++s) a[s] = c[s] = 0;
        for (u32 i0 = 0; i0 < jb.nops; i0 += wy, ++round) {
            const u64* buf = hand_over(i0 + y < jb.nops && active, i0 + y, w);
            if (y != 0) continue;
            const u32 n = jb.nops - i0 < wy ? jb.nops - i0 : wy;
            for (u32 j = 0; j < n; ++j) {
                const u32 i = i0 + j, gend = gr.first + gr.size;
                const u64 xx = buf[j * KH_WAVE + lane];
                wave_add_to_bin(&bins[jb.nbins + i], (u32)__builtin_popcountll(xx));   // the operand's distinct k-mers
                if (i < gend) {
                    any |= xx;
                    slices_add(c, xx, ns);
                    if (i + 1 == gend) {   // the genomes of the group are counted
                        if (gr.npiv && active) jb.present[(size_t)gr.prow * jb.nwords + w] = any;
                        slices_add(a, any, asl);
                    }
                } else {
                    const u32 b0 = jb.pivots[gr.q0 + (i - gend)].bin0;
                    for (u32 v = 0; v <= gr.size; ++v)
                        wave_add_to_bin(&bins[b0 + v], (u32)__builtin_popcountll(xx & slices_equal(c, v, ns)));
                }
                if (i + 1 == gend + gr.npiv) {   // and its pivots
                    any = 0;
#pragma unroll
                    for (int s = 0; s < BMP_SLICES; ++s) c[s] = 0;
                    if (++g < jb.ngroups) {
                        gr = jb.groups[g];
                        ns = bit_length(gr.size);
                    }
                }
            }
        }
        u32 gcur = ~0u;
        u64 G = 0;
        for (u32 q0 = 0; q0 < jb.npivots; q0 += wy, ++round) {
            const bool have = q0 + y < jb.npivots && active;
            const u64* buf = hand_over(have, have ? jb.pivots[q0 + y].op : 0u, w);
            if (y != 0) continue;
            const u32 n = jb.npivots - q0 < wy ? jb.npivots - q0 : wy;
            for (u32 j = 0; j < n; ++j) {
                const KhBmpPivot pv = jb.pivots[q0 + j];
                const u64 xx = buf[j * KH_WAVE + lane];
                if (pv.group != gcur) {
                    gcur = pv.group;
                    G = active ? jb.present[(size_t)jb.groups[gcur].prow * jb.nwords + w] : 0;
                }
                u64 e0 = slices_equal(a, 0, asl);
                for (u32 v = 0; v < jb.ngroups; ++v) {
                    const u64 e1 = slices_equal(a, v + 1, asl);
                    wave_add_to_bin(&bins[pv.abin0 + v], (u32)__builtin_popcountll(xx & ((G & e1) | (~G & e0))));
                    e0 = e1;
                }
            }
        }
    }
    __syncthreads();
    unsigned long long* rep = jb.hist + (size_t)(blockIdx.x % jb.reps) * nb;
    for (u32 i = tid; i < nb; i += nt)
        if (bins[i]) atomicAdd(&rep[i], (unsigned long long)bins[i]);
}

// ------------------------------------------------------------------------------------------
// k_bmp_cross
// LDS: [bins: nbins + nops u32][gx: 2 x waves x 64 u64][pw: npivots x 64 u64]
// ------------------------------------------------------------------------------------------
// Experiment type 3 with the walk of k_bmp_readout: every pivot of the launch's batch against every group.  Operands of
// the launch: the batch's pivots (build operands pop0 ..), then the genomes in group-major order (build operands 0 ..).
// A pivot's word is kept in LDS as pw[q][lane]: the lane reads back only what it stored itself, so no barrier guards it.
// A genome's word goes into the group's counter c; behind the last genome of group g the mask e = (c == v) is worked out
// once per v = 1 .. size and bin(q, g, v) += popcount(pw[q] & e) for every pivot q.  Bins: per pivot one per genome
// (group g: gr.bin0 + v - 1), then one distinct counter per operand of the launch.  No counter over groups, no device
// scratch, one phase.
__global__ __launch_bounds__(1024) void k_bmp_cross(const KhBmpCrossJob jb) {
    extern __shared__ __attribute__((aligned(16))) u8 lds_raw[];
    u32* bins = reinterpret_cast<u32*>(lds_raw);
    const u32 nops = jb.npivots + jb.ngenomes, nb = jb.nbins + nops;
    const u32 lane = threadIdx.x, y = threadIdx.y, wy = blockDim.y;
    u64* gx = reinterpret_cast<u64*>(lds_raw + ((4 * (size_t)nb + 15) & ~(size_t)15));   // [2][wy][64]
    u64* pw = gx + 2 * (size_t)wy * KH_WAVE;                                             // [npivots][64]
    const u32 tid = y * KH_WAVE + lane, nt = wy * KH_WAVE;
    for (u32 i = tid; i < nb; i += nt) bins[i] = 0;
    __syncthreads();
    u32 round = 0;
    for (u64 wb = blockIdx.x; wb * KH_WAVE < jb.nwords; wb += gridDim.x) {
        const u64 w = wb * KH_WAVE + lane;
        const bool active = w < jb.nwords;
        u32 g = 0;
        KhBmpGroup gr = jb.groups[0];
        u32 ns = bit_length(gr.size);
        u64 c[BMP_SLICES];
#pragma unroll
        for (int s = 0; s < BMP_SLICES; ++s) c[s] = 0;
        for (u32 i0 = 0; i0 < nops; i0 += wy, ++round) {
            u64 x = 0;
            if (i0 + y < nops && active) {
                const u32 i = i0 + y;
                const KhBmpOp op = jb.ops[i < jb.npivots ? jb.pop0 + i : i - jb.npivots];
                const u64* p = jb.partial + (size_t)op.split0 * jb.nwords + w;
#pragma unroll 8
                for (u32 s = 0; s < op.nsplits; ++s) x |= p[(size_t)s * jb.nwords];
            }
            u64* buf = gx + (size_t)(round & 1u) * wy * KH_WAVE;
            buf[y * KH_WAVE + lane] = x;
            __syncthreads();
            if (y != 0) continue;
            const u32 n = nops - i0 < wy ? nops - i0 : wy;
            for (u32 j = 0; j < n; ++j) {
                const u32 i = i0 + j;
                const u64 xx = buf[j * KH_WAVE + lane];
                wave_add_to_bin(&bins[jb.nbins + i], (u32)__builtin_popcountll(xx));   // the operand's distinct k-mers
                if (i < jb.npivots) {
                    pw[i * KH_WAVE + lane] = xx;
                    continue;
                }
                slices_add(c, xx, ns);
                if (i - jb.npivots + 1 == gr.first + gr.size) {   // the group is complete: every pivot against its counter
                    for (u32 v = 1; v <= gr.size; ++v) {
                        const u64 e = slices_equal(c, v, ns);
                        u32* bin = &bins[gr.bin0 + v - 1];
                        for (u32 q = 0; q < jb.npivots; ++q, bin += jb.ngenomes)
                            wave_add_to_bin(bin, (u32)__builtin_popcountll(pw[q * KH_WAVE + lane] & e));
                    }
#pragma unroll
                    for (int s = 0; s < BMP_SLICES; ++s) c[s] = 0;
                    if (++g < jb.ngroups) {
                        gr = jb.groups[g];
                        ns = bit_length(gr.size);
                    }
                }
            }
        }
    }
    __syncthreads();
    unsigned long long* rep = jb.hist + (size_t)(blockIdx.x % jb.reps) * nb;
    for (u32 i = tid; i < nb; i += nt)
        if (bins[i]) atomicAdd(&rep[i], (unsigned long long)bins[i]);
}

// ------------------------------------------------------------------------------------------
// experiment type 4: k_bmp_count, k_bmp_present, k_bmp_member
// ------------------------------------------------------------------------------------------
// k_bmp_count: how often every code occurs in a pivot.  A workgroup owns one split of a pivot and walks it with the
// staging of k_bmp_build, all positions, no ranges and no bitmap in LDS: one device-scope add of 1 per valid position
// into the pivot's table of 4^k cells, result unused.  The cells do not saturate; they are clamped where they are read.
// LDS: [code: tile_pos / 16 + 1 u32][bad16: tile_pos / 16 + 1 u16]
template <int K>
__global__ __launch_bounds__(BMP_NT) void k_bmp_count(const KhBmpMemberJob jb) {
    extern __shared__ __attribute__((aligned(16))) u8 lds_raw[];
    const u32 tid = threadIdx.x;
    const KhBmpSplit sp = jb.splits[jb.psplit0 + blockIdx.x];
    const u32 twords = jb.tile_pos / BMP_CHUNK;
    u32* code = reinterpret_cast<u32*>(lds_raw);
    u16* bad16 = reinterpret_cast<u16*>(code + twords + 1);
    u32* cnt = jb.cnt + (size_t)(sp.op - jb.ngenomes) * jb.ncells;
    constexpr u32 KMASK = (1u << (2 * K)) - 1u;
    const u32 swords = twords + 1;
    kh_u32x4 pre[BMP_FETCH];
    auto fetch = [&](const u64 t0) {
#pragma unroll
        for (u32 i = 0; i < BMP_FETCH; ++i) {
            const u32 w = tid + i * BMP_NT;
            pre[i] = codes_fetch(sp.seq, sp.len, t0 + 16ull * w, w < swords, jb.splits);
        }
    };
    if (sp.p0 < sp.p1) fetch(sp.p0);
    for (u64 t0 = sp.p0; t0 < sp.p1; t0 += jb.tile_pos) {
        __syncthreads();                                         // the last tile has been read
#pragma unroll
        for (u32 i = 0; i < BMP_FETCH; ++i) {
            const u32 w = tid + i * BMP_NT;
            u32 codes, bad;
            codes_decode(pre[i], sp.seq, sp.len, t0 + 16ull * w, codes, bad);
            if (w < swords) {
                code[w] = codes;
                bad16[w] = (u16)bad;
            }
        }
        __syncthreads();
        if (t0 + jb.tile_pos < sp.p1) fetch(t0 + jb.tile_pos);
        const u64 tend = t0 + jb.tile_pos < sp.p1 ? t0 + jb.tile_pos : sp.p1;
        const u32 nch = (u32)((tend - t0 + BMP_CHUNK - 1) / BMP_CHUNK);
        for (u32 c = tid; c < nch; c += BMP_NT) {
            const u64 cw = (u64)code[c] | ((u64)code[c + 1] << 32);   // as in k_bmp_build
            u32 inv = (u32)bad16[c] | ((u32)bad16[c + 1] << 16);
            {
                u32 w = 1;
#pragma unroll
                for (int s = 0; s < 3; ++s)
                    if (2 * w <= (u32)K) { inv |= inv >> w; w *= 2; }
                inv |= inv >> ((u32)K - w);
            }
            const u32 valid = ~inv & 0xffffu;
            if (!valid) continue;
            const u64 fwd = kh_revpairs64(cw);
            const u64 rcw = ~cw;
#pragma unroll
            for (u32 j = 0; j < BMP_CHUNK; ++j) {
                const u32 fw = (u32)(fwd >> (64 - 2 * (j + K))) & KMASK;
                const u32 rc = (u32)(rcw >> (2 * j)) & KMASK;
                if ((valid >> j) & 1u) atomicAdd(&cnt[fw < rc ? fw : rc], 1u);
            }
        }
    }
}

// k_bmp_present: launch shape, LDS layout and walk of k_bmp_readout over the genomes (group-major), then the pivots.
// A genome's word goes into its group's counter and into `any`; behind the group's last genome the bins of the counter
// are added and `any` is stored to present[group] (every group, every word: nothing is cleared beforehand).  A
// pivot's word is stored to pword[pivot], and the wave's popcount sum to blk[pivot][block of 64 words]: one writer per
// word and per block, nothing atomic.  No counter over groups.
__global__ __launch_bounds__(1024) void k_bmp_present(const KhBmpMemberJob jb) {
    extern __shared__ __attribute__((aligned(16))) u8 lds_raw[];
    u32* bins = reinterpret_cast<u32*>(lds_raw);
    const u32 nb = jb.nbins + jb.nops;
    u64* gx = reinterpret_cast<u64*>(lds_raw + ((4 * (size_t)nb + 15) & ~(size_t)15));   // [2][wy][64]
    const u32 lane = threadIdx.x, y = threadIdx.y, wy = blockDim.y;
    const u32 tid = y * KH_WAVE + lane, nt = wy * KH_WAVE;
    for (u32 i = tid; i < nb; i += nt) bins[i] = 0;
    __syncthreads();
    u32 round = 0;
    for (u64 wb = blockIdx.x; wb * KH_WAVE < jb.nwords; wb += gridDim.x) {
        const u64 w = wb * KH_WAVE + lane;
        const bool active = w < jb.nwords;
        u32 g = 0;
        KhBmpGroup gr = jb.groups[0];
        u32 ns = bit_length(gr.size);
        u64 c[BMP_SLICES], any = 0;
#pragma unroll
        for (int s = 0; s < BMP_SLICES; ++s) c[s] = 0;
        for (u32 i0 = 0; i0 < jb.nops; i0 += wy, ++round) {
            u64 x = 0;
            if (i0 + y < jb.nops && active) {
                const KhBmpOp op = jb.ops[i0 + y];
                const u64* p = jb.partial + (size_t)op.split0 * jb.nwords + w;
#pragma unroll 8
                for (u32 s = 0; s < op.nsplits; ++s) x |= p[(size_t)s * jb.nwords];
            }
            u64* buf = gx + (size_t)(round & 1u) * wy * KH_WAVE;
            buf[y * KH_WAVE + lane] = x;
            __syncthreads();
            if (y != 0) continue;
            const u32 n = jb.nops - i0 < wy ? jb.nops - i0 : wy;
            for (u32 j = 0; j < n; ++j) {
                const u32 i = i0 + j;
                const u64 xx = buf[j * KH_WAVE + lane];
                const u32 sum = wave_scan_add((u32)__builtin_popcountll(xx));   // lane 63: the wave's distinct codes
                if (lane == KH_WAVE - 1 && sum) atomicAdd(&bins[jb.nbins + i], sum);
                if (i >= jb.ngenomes) {
                    const u32 p = i - jb.ngenomes;
                    if (active) jb.pword[(size_t)p * jb.nwords + w] = xx;
                    if (lane == KH_WAVE - 1) jb.blk[(size_t)p * jb.nblocks + wb] = sum;
                    continue;
                }
                any |= xx;
                slices_add(c, xx, ns);
                if (i + 1 == gr.first + gr.size) {   // the group is complete
                    for (u32 v = 1; v <= gr.size; ++v)
                        wave_add_to_bin(&bins[gr.bin0 + v], (u32)__builtin_popcountll(slices_equal(c, v, ns)));
                    if (active) jb.present[(size_t)g * jb.nwords + w] = any;
                    any = 0;
#pragma unroll
                    for (int s = 0; s < BMP_SLICES; ++s) c[s] = 0;
                    if (++g < jb.ngroups) {
                        gr = jb.groups[g];
                        ns = bit_length(gr.size);
                    }
                }
            }
        }
    }
    __syncthreads();
    unsigned long long* rep = jb.hist + (size_t)(blockIdx.x % jb.reps) * nb;
    for (u32 i = tid; i < nb; i += nt)
        if (bins[i]) atomicAdd(&rep[i], (unsigned long long)bins[i]);
}

// k_bmp_member: the records of a pivot in ascending code order.  blockDim = (64, BMP_MEMBER_WAVES); a workgroup owns
// BMP_MEMBER_RUN consecutive blocks of 64 words of one pivot (blockIdx.y), a wave one block at a time, a lane one word.
// Rank of a word's first record: the pivot's distinct codes in front of the run (blk, written by k_bmp_present, summed
// by the whole workgroup in the prologue), the blocks of the run in front of this one, and the exclusive wave scan of
// the popcounts.  The lane keeps its `present` words in LDS only to index them by group without scratch: it reads back
// what it stored itself, so no barrier guards them.
// LDS: [pres: waves x ngroups x 64 u64][part: waves u32][run: BMP_MEMBER_RUN u32]
constexpr u32 BMP_MEMBER_WAVES = 4;
constexpr u32 BMP_MEMBER_RUN = 16;
__global__ __launch_bounds__(BMP_MEMBER_WAVES * KH_WAVE) void k_bmp_member(const KhBmpMemberJob jb) {
    extern __shared__ __attribute__((aligned(16))) u8 lds_raw[];
    const u32 lane = threadIdx.x, y = threadIdx.y, tid = y * KH_WAVE + lane;
    u64* pres = reinterpret_cast<u64*>(lds_raw) + (size_t)y * jb.ngroups * KH_WAVE;
    u32* part = reinterpret_cast<u32*>(lds_raw + 8 * (size_t)BMP_MEMBER_WAVES * jb.ngroups * KH_WAVE);
    u32* run = part + BMP_MEMBER_WAVES;
    const u32 p = blockIdx.y;
    const u32 b0 = blockIdx.x * BMP_MEMBER_RUN, b1 = b0 + BMP_MEMBER_RUN < jb.nblocks ? b0 + BMP_MEMBER_RUN : jb.nblocks;
    const u32* blk = jb.blk + (size_t)p * jb.nblocks;
    u32 s = 0;
    for (u32 i = tid; i < b0; i += BMP_MEMBER_WAVES * KH_WAVE) s += blk[i];
    s = wave_scan_add(s);
    if (lane == KH_WAVE - 1) part[y] = s;
    if (tid < b1 - b0) run[tid] = blk[b0 + tid];
    __syncthreads();
    u32 front = 0;
    for (u32 i = 0; i < BMP_MEMBER_WAVES; ++i) front += part[i];
    const u32* cnt = jb.cnt + (size_t)p * jb.ncells;
    const u64 r0 = jb.rec_off[p];
    for (u32 b = b0 + y; b < b1; b += BMP_MEMBER_WAVES) {
        u32 base = front;
        for (u32 i = b0; i < b; ++i) base += run[i - b0];
        const u64 w = (u64)b * KH_WAVE + lane;
        const bool active = w < jb.nwords;
        u64 pw = active ? jb.pword[(size_t)p * jb.nwords + w] : 0;
        for (u32 d = 0; d < jb.ngroups; ++d) pres[d * KH_WAVE + lane] = active ? jb.present[(size_t)d * jb.nwords + w] : 0;
        const u32 pc = (u32)__builtin_popcountll(pw);
        u64 r = r0 + base + (wave_scan_add(pc) - pc);
        while (pw) {
            const u32 bit = (u32)__builtin_ctzll(pw);
            pw &= pw - 1;
            u64 m = 0;
            for (u32 d = 0; d < jb.ngroups; ++d) m |= ((pres[d * KH_WAVE + lane] >> bit) & 1ull) << d;
            const u32 n = cnt[64 * w + bit];
            jb.rec_mask[r] = m;
            jb.rec_count[r] = n < jb.pivot_cs ? n : jb.pivot_cs;
            ++r;
        }
    }
}

// k_bmp_group_masks: the groups' presence rows transposed into the mask table of the read-level votes (type 6):
// table[code * mwords + j] bit g = group 64 j + g holds canonical code `code`.  blockDim = (64, BMP_MASKS_WAVES); a
// workgroup owns 64 consecutive bitmap words (blockIdx.x) and one mask word j (blockIdx.y).  The 64 x 64 tile
// present[64 j + g][w0 + i] is loaded into LDS, lane = i, a wave every fourth g; groups from ngroups on load as 0.  A
// wave then owns every fourth word i, lane = bit: one broadcast read of tile[g][i] per group, bit `lane` of it goes to
// bit g of the lane's cell.  One writer per cell, nothing atomic; every cell of the words below nwords is written,
// zeros included (the table comes from the pool, k_read_fold counts whole words).
constexpr u32 BMP_MASKS_WAVES = 4;
__global__ __launch_bounds__(BMP_MASKS_WAVES * KH_WAVE) void k_bmp_group_masks(const u64* __restrict__ present, u64* __restrict__ table,
                                                                              const u64 nwords, const u32 ngroups, const u32 mwords) {
    __shared__ u64 tile[KH_WAVE][KH_WAVE];                     // [group of the mask word][bitmap word of the block]: 32 KiB
    const u32 lane = threadIdx.x, y = threadIdx.y, j = blockIdx.y;
    const u64 w0 = (u64)blockIdx.x * KH_WAVE;                  // < nwords: the grid is ceil(nwords / 64)
    for (u32 g = y; g < KH_WAVE; g += BMP_MASKS_WAVES) {
        const u32 grp = j * KH_WAVE + g;
        tile[g][lane] = grp < ngroups && w0 + lane < nwords ? present[(size_t)grp * nwords + w0 + lane] : 0ull;
    }
    __syncthreads();
    for (u32 i = y; i < KH_WAVE && w0 + i < nwords; i += BMP_MASKS_WAVES) {
        u64 m = 0;
#pragma unroll 8
        for (u32 g = 0; g < KH_WAVE; ++g) m |= ((tile[g][i] >> lane) & 1ull) << g;
        table[((w0 + i) * KH_WAVE + lane) * mwords + j] = m;
    }
}

template <class K> void bmp_allow_lds(K kern, size_t bytes) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
// f(std::integral_constant<int, k>) for the k the kernels are instantiated for; another k: nothing (the host asks for
// k <= KH_BMP_INST_MAX_K only)
template <class F> void bmp_for_k(u32 k, F f) {
    switch (k) {
#define BMP_K(KK) case KK: f(std::integral_constant<int, KK>{}); break;
        BMP_K(1) BMP_K(2) BMP_K(3) BMP_K(4) BMP_K(5) BMP_K(6) BMP_K(7) BMP_K(8) BMP_K(9) BMP_K(10) BMP_K(11) BMP_K(12)
        BMP_K(13)
#undef BMP_K
        default: break;
    }
}
// a kernel of the walk: grid workgroups of `waves` waves
template <class Job> void launch_walk(void (*kern)(Job), const Job& job, size_t lds, u32 grid, u32 waves, hipStream_t st) {
    bmp_allow_lds(kern, lds);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(KH_WAVE, waves), lds, st, job);
}

}   // namespace

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
size_t kh_bmp_build_lds_bytes(u32 range_bits, u32 tile_pos) {
    return ((size_t)1 << (range_bits - 3)) + bmp_stage_lds_bytes(tile_pos) + 16;
}
size_t kh_bmp_readout_lds_bytes(u32 nbins, u32 nops, u32 waves) {
    return ((4 * ((size_t)nbins + nops) + 15) & ~(size_t)15) + 2 * (size_t)waves * KH_WAVE * 8;
}
size_t kh_bmp_cross_lds_bytes(u32 nbins, u32 npivots, u32 ngenomes, u32 waves) {
    return kh_bmp_readout_lds_bytes(nbins, npivots + ngenomes, waves) + (size_t)npivots * KH_WAVE * 8;
}
size_t kh_bmp_member_lds_bytes(u32 ngroups) {
    return 8 * (size_t)BMP_MEMBER_WAVES * ngroups * KH_WAVE + 4 * (size_t)(BMP_MEMBER_WAVES + BMP_MEMBER_RUN);
}
void kh_launch_bmp_build(const KhBmpJob& job, u32 nsplits, hipStream_t st) {
    if (!nsplits) return;
    const size_t lds = kh_bmp_build_lds_bytes(job.range_bits, job.tile_pos);
    bmp_for_k(job.k, [&](auto k) {
        bmp_allow_lds(k_bmp_build<k()>, lds);
        hipLaunchKernelGGL(k_bmp_build<k()>, dim3(nsplits * job.nranges), dim3(BMP_NT), lds, st, job);
    });
}
void kh_launch_bmp_count(const KhBmpMemberJob& job, hipStream_t st) {
    if (!job.npsplits) return;
    const size_t lds = bmp_stage_lds_bytes(job.tile_pos);   // 24 KiB at most
    bmp_for_k(job.k, [&](auto k) { hipLaunchKernelGGL(k_bmp_count<k()>, dim3(job.npsplits), dim3(BMP_NT), lds, st, job); });
}
void kh_launch_bmp_readout(const KhBmpJob& job, u32 grid, u32 waves, hipStream_t st) {
    launch_walk(k_bmp_readout, job, kh_bmp_readout_lds_bytes(job.nbins, job.nops, waves), grid, waves, st);
}
void kh_launch_bmp_pivot(const KhBmpPivotJob& job, u32 grid, u32 waves, hipStream_t st) {
    launch_walk(k_bmp_pivot, job, kh_bmp_readout_lds_bytes(job.nbins, job.nops, waves), grid, waves, st);
}
void kh_launch_bmp_cross(const KhBmpCrossJob& job, u32 grid, u32 waves, hipStream_t st) {
    launch_walk(k_bmp_cross, job, kh_bmp_cross_lds_bytes(job.nbins, job.npivots, job.ngenomes, waves), grid, waves, st);
}
void kh_launch_bmp_present(const KhBmpMemberJob& job, u32 grid, u32 waves, hipStream_t st) {
    launch_walk(k_bmp_present, job, kh_bmp_readout_lds_bytes(job.nbins, job.nops, waves), grid, waves, st);
}
void kh_launch_bmp_member(const KhBmpMemberJob& job, hipStream_t st) {
    if (!job.npivots) return;
    const size_t lds = kh_bmp_member_lds_bytes(job.ngroups);
    bmp_allow_lds(k_bmp_member, lds);
    hipLaunchKernelGGL(k_bmp_member, dim3((job.nblocks + BMP_MEMBER_RUN - 1) / BMP_MEMBER_RUN, job.npivots),
                       dim3(KH_WAVE, BMP_MEMBER_WAVES), lds, st, job);
}
void kh_launch_bmp_group_masks(const u64* present, u64* table, u64 nwords, u32 ngroups, u32 mwords, hipStream_t st) {
    hipLaunchKernelGGL(k_bmp_group_masks, dim3((u32)((nwords + KH_WAVE - 1) / KH_WAVE), mwords), dim3(KH_WAVE, BMP_MASKS_WAVES), 0, st,
                       present, table, nwords, ngroups, mwords);
}
