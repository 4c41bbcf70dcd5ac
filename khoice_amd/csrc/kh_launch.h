// Host-callable launchers for the gfx950 kernels in kh_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include "kh_common.h"

// one input sequence (genome) of a batched build
struct KhSeg {
    const u8* seq;    // device pointer to base 0 (16-B aligned; bytes past len are never read)
    u64 len;          // bases (bytes)
    u64 npos;         // k-mer start positions: len >= k ? len-k+1 : 0
    u64 thist_base;   // index of tile 0 / bucket 0 in the tile-histogram matrix
    u32 nbuckets;     // B_s: buckets this build keeps (cursor rows, bucket arrays)
    u32 bucket_base;  // index of its first bucket in the global bucket arrays
    u32 tile_base;    // global index of its first tile
    u32 ntiles;
    // Key-range waves (a build that keeps only one slice of the key space, kh_exp1_run under a memory
    // budget): the key space is cut into nb_virtual equal-width buckets, of which this build keeps
    // [b_first, b_first + nbuckets); keys of other buckets are dropped in passes A and B.  A build of
    // the whole key space has nb_virtual == nbuckets and b_first == 0.
    u32 nb_virtual;
    u32 b_first;
};
struct KhTile { u32 seg; u32 tile_in_seg; };

// What one pass-C workgroup needs, in the order the workgroups are started (written by
// k_col_offsets).  Buckets of different segments are INTERLEAVED in that order and every
// segment has its own look-back chain and output region: a workgroup's chain predecessor was
// started (number of interleaved segments) workgroups earlier, so its aggregate is almost
// always published by the time it is looked at (the single chain of before spent a quarter of a
// workgroup's life waiting for the slowest of its 512 concurrent predecessors).
struct KhBucketWork {
    u64 lo;         // first key of the bucket in the partition array
    u64 out_base;   // first output record of the bucket's segment
    u32 n;          // keys in the bucket
    u32 nb;         // equal-width buckets of the whole key space (the fine-bin scale; KhSeg::nb_virtual)
    u32 b;          // index of the bucket inside its segment = index in the segment's chain
    u32 gb;         // global bucket index (segment's chain starts at gb - b)
};

struct KhSetView {    // one operand of a set operation (device-resident, sorted by mixed key)
    const void* keys;
    const u32* counts;   // nullptr => every counter == uniform
    u64 n;
    u32 uniform;
    u32 pad;
};

struct KhBoundsJob {   // one set operation's share of a batched range-bounds launch
    const KhSetView* sets;
    u64* bounds;
    u64* zero;          // workspace to clear (look-back descriptors, control words, histogram)
    u64 zero_words;
    u32 nsets, nranges;
};

// Several independent set operations of the same kind (W, payload mode, operation, cs) run as ONE
// launch: blockIdx.y picks the operation from this table, which travels in the kernel arguments
// (scalar loads, no extra global round trip in front of a workgroup's first useful load).
constexpr int KH_SETOP_BATCH = 16;
struct KhSetopJob {
    const KhSetView* sets;
    const u64* bounds;          // [nsets][nslots + 1] of the whole operation
    void* out_keys;
    u32* out_counts;
    u64* desc;                  // this chain's look-back descriptors [nranges]
    u32* ctl;                   // the operation's control words: ticket, err, fullest slot, pad, u64 outputs
    unsigned long long* hist;   // nullptr: no fused histogram
    u32 nsets;
    u32 nslots;                 // slots of the whole operation (the key -> slot scale)
    u32 slot0, nranges;         // this chain covers slots [slot0, slot0 + nranges)
};
// An operation whose output set nobody reads as ONE array (histogram-only unions) is run as several
// chains: consecutive slot ranges with their own look-back chain, each writing at the offset its
// inputs start at (sum over operands of bounds[slot0]) — same bytes written, no global order to
// wait for.  A chain adds its output count to ctl's u64 when its last slot finishes.
struct KhSetopBatch { KhSetopJob job[KH_SETOP_BATCH]; };

// ---- fused experiment-type-1 path (kh_exp1_run when no per-group set is wanted) ----
// Pass C in GRID mode: every genome of the batch uses the SAME bucket grid (nb equal-width slots
// of the mixed key space), a bucket's distinct keys are written where its input starts (index
// `lo` of an output array laid out like the partition array: no compaction, hence no look-back
// chain), and for every bucket an index of S + 1 u16 offsets is emitted: off[f] = number of the
// bucket's keys in front of sub-range f (S equal-width sub-ranges of the bucket), off[S] = d.
// Slot r = b * S + f of the key space then is, in EVERY genome g, the contiguous record range
// [bstart[g*nb+b] + off[f], bstart[g*nb+b] + off[f+1]) — what a set operation otherwise finds by
// binary search (k_range_bounds) is a table lookup.
struct KhGrid {
    u16* off;                       // [nseg * nb][S + 1]; nullptr: normal (compact, look-back) mode
    unsigned long long* distinct;   // [nseg]: distinct keys per genome, added bucket by bucket
    u32 S;
    u32 nb;
};
// One tagged n-ary union over the gridded genome sets of up to 64 genomes: operand g carries tag
// g, a run of equal keys becomes a 64-bit genome mask, and from the mask come, in ONE pass,
//   * for every group holding the key, "in how many of its genomes" -> step_4 histograms,
//   * "in how many groups"                                          -> step_8 histogram
// (exp_type_1.smk:175-191, :243-259).  Histograms are compact: bin = first bin of the group +
// count; across-group bins follow at `abase`.  A workgroup (one slot) keeps its histogram in LDS and
// adds it to one of `reps` replicas in device memory (the host sums them): the replicas spread
// what would otherwise be ~10^6 atomics per step on a handful of cache lines.
constexpr int KH_TAG_MAX_OPS = 64;
constexpr int KH_TAG_MAX_BINS = 255;
struct KhTagJob {
    const void* keys;           // gapped key arrays of all operands (one allocation)
    const u64* bstart;          // [nops * nb + 1]
    const u16* off;             // [nops * nb][S + 1]
    const u32* ginfo;           // [64] per operand: first operand of its group | group size << 8 | first bin << 16
    unsigned long long* hist;   // [reps][nbins]
    u32* ctl;                   // [0] error bits, [1] fullest slot seen
    u32 nb, S, nops, nbins, abase, ngroups, reps;
    u32 nbv;                    // buckets of the whole key space (== nb unless the build was a key-range wave)
    u32 binmul;                 // 2^26 / (fine bins of the widest sub-range): in-slot fine-bin scale
    // optional ordered output (multi-GPU: the local across-group set, counter = groups holding the key)
    void* out_keys;
    u32* out_counts;
    u64* desc;                  // look-back descriptors [nb * S], zeroed; nullptr: histograms only
    unsigned long long* out_n;  // number of records written
};

// ---- super-k-mer form of the fused path (kh_skm.hip): records of n consecutive k-mers that share their
// minimizer slot, partitioned in two levels (coarse bucket, then slot = coarse * S + fine), then one LDS
// hash set per slot.  A record is 16 bytes (32 with two-word keys): the bases, the fine index of its slot, the genome
// (operand) number and n; kh_skm_rec.h is the one definition of both formats.
#ifndef KH_TUNE_SKM_STAGE
#define KH_TUNE_SKM_STAGE 2048   // (1024 / 1536 / 2048 / 2304 / 2560: scatter 0.82 / 0.68 / 0.645 / 0.69 / 0.735 ms; above 2048 only two workgroups fit a CU)
#endif
constexpr u32 KH_SKM_STAGE = KH_TUNE_SKM_STAGE;   // records counting-sorted in LDS per flush of the scatter
constexpr u32 KH_SKM_MAX_COARSE = 256;    // coarse buckets (LDS counters of the scatter); 512 (KH_SKM2_MAX_COARSE) for inputs too large for 256
constexpr u32 KH_SKM_MAX_FINE = 512;      // slots per coarse bucket (9 bits in the record)
constexpr int KH_SKM_MIN_K = 17, KH_SKM_MAX_K = 32;   // (below 17 the key arrays are faster; the kernels take k >= 15)
#ifndef KH_TUNE_SKM_CUR1_STRIDE
#define KH_TUNE_SKM_CUR1_STRIDE 1088
#endif
// u32 words between the cursors of two coarse buckets: every flush of every workgroup adds to all of them,
// so they are kept on different memory channels (4352 bytes apart) instead of sixteen to a cache line
constexpr u32 KH_SKM_CUR1_STRIDE = KH_TUNE_SKM_CUR1_STRIDE;
// the words of KhSkmJob::ctl (zeroed before the scatter, read back by the host after the union or the cross kernel)
enum : u32 {
    KH_SKM_CTL_ERR = 0,             // error bits (KH_ERR_CAPACITY, KH_ERR_ORDER)
    KH_SKM_CTL_FULLEST = 1,         // k-mer instances of the fullest slot seen (above the table's size only)
    KH_SKM_CTL_RECORDS = 2,         // records written by the scatter
    KH_SKM_CTL_EXPANDED = 3,        // k-mer instances expanded from the records
    // (word 4 is unused; the words behind it keep their places: kernels address them by immediate offsets)
    KH_SKM_CTL_SPILLED = 5,         // records spilled to the side list (spill_rec / spill_slot)
    KH_SKM_CTL_LISTED = 6,          // slots listed in big_list
    KH_SKM_CTL_MULTI = 7,           // slots taken in more than one subset (k_skm_union) or round (k_skm_cross)
    KH_SKM_CTL_WORDS = 8,
};
// the words of KhSkmPackJob::ctl and KhSkmPhasedJob::ctl; behind them, in the host's block of a pack, the part cursors
enum : u32 {
    KH_SKM_XCTL_ERR = 0,            // error bits
    KH_SKM_XCTL_FULLEST = 1,        // k_skm_phased: k-mer instances of the fullest slot seen
    KH_SKM_XCTL_CURSORS = 16,       // k_skm_pack: KhSkmPackJob::part_cursor starts here, [nparts][nsub]
};
struct KhSkmJob {
    const KhSeg* segs;
    const KhTile* tiles;
    const u8* seg_tag;              // [nseg] tag of a segment's records; nullptr: the segment number (operand = genome)
    uint4* reg1;                    // [nb1][cap1] records by coarse bucket
    uint4* reg2;                    // [nslots][cap2] records by slot
    u32* cur1;                      // [nb1 * KH_SKM_CUR1_STRIDE] zeroed: cursor of bucket b at b * KH_SKM_CUR1_STRIDE
    u32* cur2;                      // [nslots] zeroed
    unsigned long long* inst;       // [nops] valid k-mer instances per genome
    unsigned long long* dup;        // [64] instances whose (k-mer, genome) pair was seen before
    const u32* ginfo;               // as KhTagJob
    unsigned long long* hist;       // [reps][nbins]
    u32* ctl;                       // [KH_SKM_CTL_WORDS] zeroed: the control words, KH_SKM_CTL_*
    u32* claim;                     // zeroed, a 128-byte line of its own: the unions' slot claims (SkmSlotFeed, kh_skm_device.h)
    u32 tile_pos;
    int k, m;                       // m-mer length of the minimizer (<= 16)
    u32 w;                          // m-mers per k-mer: k - m + 1
    u32 nmax;                       // k-mers per record at most
    u32 nslots, S, nb1, cap1, cap2;
    u32 nbins, abase, reps, nops;
    // one-word keys: records of slots whose region is full (regroup) and the slots the union leaves to k_skm_big
    uint4* spill_rec;               // [spill_cap] records (one or two uint4 each); nullptr: a full region is an error
    u32* spill_slot;                // [spill_cap]
    u32* big_list;                  // [big_cap] slots with more records than their region holds
    u32 spill_cap, big_cap;         // counters: ctl[KH_SKM_CTL_SPILLED], ctl[KH_SKM_CTL_LISTED]
};
// ---- experiment type 3 from the same records (k_skm_cross, kh_skm_device.h): the operands of the scatter are the
// genomes in group-major order, then the pivots of the pass, every pivot a group of its own in `ginfo`.  What the
// kernel needs beyond KhSkmJob, which stays as the other kernels know it:
struct KhSkmCrossJob {
    unsigned long long* bins;       // [reps][nbins] zeroed: pivot q, c >= 1 genomes of the group whose first genome is g0: q * ngenomes + g0 + c - 1
    u32 pmlo, pmhi;                 // the pivots' bits of the operand mask
    u32 ngenomes;                   // operands [0, ngenomes) are genomes, the rest pivots
    u32 nbins, reps;                // nbins = pivots * ngenomes <= 1024
    u32 nlisted;                    // 0: the direct launch over all slots; else the listed launch over big_list[0 .. nlisted)
};
// ---- experiment type 2 from the same records (k_skm_cross with the read-out SkmCrossOwn): the same operands, the same walk; every pivot is counted
// against its own group (in how many of its genomes: size + 1 within bins from w0, count 0 included) and against the
// groups (in how many OTHER groups: ngroups across bins from a0 = w0 + size + 1).  cj as above with
// bins: [reps][nbins], nbins = the sum of size + 1 + ngroups over the pivots of the pass <= 1024.
struct KhSkmPivotJob {
    KhSkmCrossJob cj;
    u32 pinfo[KH_TAG_MAX_OPS];      // per pivot OPERAND (entries of genomes unused), as a ginfo word: first genome of its own
                                    // group | genomes in that group << 8 | w0 << 16
};
// What the host needs to know about a key width: one-word keys (k <= 32, 16-byte records, kh_skm.hip) and two-word
// keys (k <= 63, 32-byte records: two uint4 per record in reg1 / reg2, kh_skm2.hip) fill one table each.
constexpr int KH_SKM2_MAX_K = 63;         // k = 64: the all-ones low key word is a k-mer (A^32 T^32)
constexpr u32 KH_SKM2_MAX_COARSE = 512;
constexpr u32 KH_SKM2_MAX_FINE = 1024;    // slots per coarse bucket with two-word keys (10 bits in the record)
struct KhSkmWidth {
    u32 rec_bytes;
    u32 max_coarse, max_fine;       // coarse buckets (LDS counters of the scatter), slots per coarse bucket (bits in the record)
    u32 max_cap2;                   // records of a slot the union takes
    u32 table;                      // entries of the union's hash set: the k-mer instances of a slot it takes per round
    u32 union_per_cu, cross_per_cu; // workgroups of the persistent union / of the direct cross launch that fit a CU
    u32 pivot_per_cu;               // likewise of the direct launch with the type-2 read-out
    u32 cross_round;                // k-mer instances of a slot the cross kernel takes in one round
    bool (*supports_w)(u32 w);      // m-mers per k-mer the scatter kernel is instantiated for
    void (*scatter)(const KhSkmJob& job, u32 ntiles, hipStream_t st);
    void (*regroup)(const KhSkmJob& job, hipStream_t st);
    void (*unite)(const KhSkmJob& job, u32 cs, u32 grid, hipStream_t st);    // persistent: grid workgroups walk the slots
    void (*big)(const KhSkmJob& job, u32 cs, u32 nbig, hipStream_t st);      // the slots of big_list, one workgroup each
    void (*cross)(const KhSkmJob& job, const KhSkmCrossJob& cj, u32 grid, hipStream_t st);
    void (*pivot)(const KhSkmJob& job, const KhSkmPivotJob& pj, u32 grid, hipStream_t st);
};
const KhSkmWidth& kh_skm_width1();     // kh_skm.hip
const KhSkmWidth& kh_skm_width2();     // kh_skm2.hip
inline const KhSkmWidth& kh_skm_width(bool two) { return two ? kh_skm_width2() : kh_skm_width1(); }
// the workspace of a super-k-mer run zeroed and its descriptors fetched from the pinned staging in one kernel; its
// results stored to the pinned staging by a kernel (kh_skm.hip: k_skm_ws_init, k_skm_ws_down)
void kh_launch_skm_ws_init(void* ws, size_t zero_bytes, const void* up, size_t up_bytes, hipStream_t st);   // multiples of 16
void kh_launch_skm_ws_down(void* down, const void* ws, size_t bytes, hipStream_t st);                       // a multiple of 8
// ---- the exchange form of the across-group step (multi-GPU; kh_skm.hip k_skm_pack / k_skm_phased)
struct KhSkmPackJob {
    const uint4* reg2;              // [nslots][cap2] this rank's records by slot (tag = local group, < 32)
    const u32* cur2;                // [nslots]
    uint4* out_rec;                 // [nparts][part_cap] the records that travel, by owner of their slot
    u32* out_mask;                  // [nparts][part_cap] their masks of local groups
    u32* part_cursor;               // [nparts] zeroed
    u32* slot_count;                // [nslots] records that travel
    u32* slot_off;                  // [nslots] where they start in their part's array
    u32* ctl;                       // KH_SKM_XCTL_ERR
    unsigned long long* dup;        // [32] or null: per tag, k-mer instances of records that repeat one of the SAME tag
    u64 part_cap;
    u32 cap2, nslots, spp;          // spp: slots per part (slot s belongs to part s / spp)
    u32 nsub;                       // cursors per part (slot s uses cursor s % nsub over 1 / nsub of the part's array): 1 = the
                                    // part is filled without gaps (it travels); more = no single hot atomic (one GPU)
};
struct KhSkmCompactJob {            // a part packed through several cursors -> the same records without gaps (they travel)
    const uint4* tmp_rec;           // [nparts][part_cap], sub-range q of a part at q * (part_cap / nsub)
    const u32* tmp_mask;
    uint4* out_rec;                 // [nparts][part_cap], filled from 0
    u32* out_mask;
    const u32* cursors;             // [nparts][nsub] records per sub-range
    u32* slot_off;                  // [nslots] rewritten to the compacted positions
    u32* part_n;                    // [nparts] out: records of the part
    u64 part_cap;
    u32 nslots, spp, nsub, nparts;
};
void kh_launch_skm_pack_compact(const KhSkmCompactJob& job, hipStream_t st);
struct KhSkmPiece {                 // what one source rank sent for this rank's slots
    const uint4* rec;
    const u32* mask;
    const u32* count;               // [nslots of this rank]
    const u32* off;                 // [nslots of this rank] first record of the slot in `rec`
    u32 dup_row;                    // row of KhSkmPhasedJob::dup its tags count into
    u32 join_next;                  // 1: the next piece continues this phase (the same tags: no fold in between)
};
struct KhSkmPhasedJob {
    const KhSkmPiece* pieces;       // device array [npieces]
    unsigned long long* hist;       // [hist_len], zeroed
    u32* ctl;                       // KH_SKM_XCTL_ERR, KH_SKM_XCTL_FULLEST
    unsigned long long* dup;        // [npieces][32] or null: per (piece, tag), instances that repeat a k-mer of the same tag
    u32 npieces, nslots, hist_len, cs;
    u32 share_q8;                   // distinct k-mers expected per 256 instances of a slot (256: the pieces share nothing;
                                    // sub-batches of one group share most): the rounds of a slot are sized from it
    int k;
};
constexpr u32 KH_SKM_PHASED_MAX_DUP_PIECES = 32;   // pieces whose repeats can be counted (LDS counters)
size_t kh_skm_phased_lds_bytes();
void kh_launch_skm_pack(const KhSkmPackJob& job, hipStream_t st);
void kh_launch_skm_phased(const KhSkmPhasedJob& job, u32 grid, hipStream_t st);

// ---- presence-bitmap form of the fused path (kh_bmp.hip): k <= KH_BMP_MAX_K, histograms and distinct counts only.
// k_bmp_build writes one partial bitmap of 4^k bits (at least one 64-bit word) per split of a genome, k_bmp_readout
// counts over them with bit-sliced counters: no genome mask, any number of genomes and groups up to the limits below.
#ifndef KH_TUNE_BMP_RANGE_BITS
#define KH_TUNE_BMP_RANGE_BITS 20   // codes per build workgroup: 2^20 bits = 128 KiB of LDS, one workgroup per CU
#endif
constexpr int KH_BMP_RANGE_BITS = KH_TUNE_BMP_RANGE_BITS;
constexpr int KH_BMP_MAX_K = 12;         // the form is taken up to this k (KHOICE_BMP_MAX_K: up to KH_BMP_INST_MAX_K)
constexpr int KH_BMP_INST_MAX_K = 13;    // largest k the build kernel is instantiated for
constexpr u32 KH_BMP_MAX_COUNT = 1023;   // genomes of a group, groups: ten counter slices
constexpr u32 KH_BMP_MAX_BINS = 4096;
constexpr u32 KH_BMP_TILE = 65520;       // positions staged per round of a build workgroup: 4095 words of 16 and the halo word
struct KhBmpSplit {                 // a run of consecutive k-mer positions of one genome
    const u8* seq;                  // the genome's base 0 (16-B aligned; bytes past len are never read)
    u64 len;
    u64 p0, p1;                     // positions [p0, p1); p0 a multiple of 16, p1 a multiple of 16 or the genome's last
    u32 op;                         // the genome's operand number
    u32 pad;
};
struct KhBmpOp { u32 split0, nsplits; };              // an operand's partial bitmaps: [split0, split0 + nsplits), at least one
struct KhBmpGroup { u32 first, size, bin0, pad; };    // operands [first, first + size) (group-major order), first bin
struct KhBmpJob {
    const KhBmpSplit* splits;
    const KhBmpOp* ops;             // [nops]
    const KhBmpGroup* groups;       // [ngroups]
    u64* partial;                   // [splits][nwords]
    unsigned long long* inst;       // [nops] zeroed: valid k-mer positions per genome
    unsigned long long* hist;       // [reps][nbins + nops] zeroed: the bins, then the distinct k-mers of every operand
    u64 nwords;                     // 64-bit words of one bitmap: max(1, 4^k / 64)
    u32 tile_pos;                   // positions staged per round: a multiple of 16
    u32 range_bits, nranges;        // codes per build workgroup (log2, >= 6), ranges of the code space
    u32 nops, ngroups, nbins, abase, reps;
    int k;
};
size_t kh_bmp_build_lds_bytes(u32 range_bits, u32 tile_pos);
size_t kh_bmp_readout_lds_bytes(u32 nbins, u32 nops, u32 waves);
void kh_launch_bmp_build(const KhBmpJob& job, u32 nsplits, hipStream_t st);   // nsplits * nranges workgroups
void kh_launch_bmp_readout(const KhBmpJob& job, u32 grid, u32 waves, hipStream_t st);   // grid workgroups of `waves` waves walk the words

// ---- experiment type 2 from the same bitmaps (k_bmp_pivot): the pivots are further operands of k_bmp_build, placed
// behind the genomes of the group they were held out of.  Bins: per pivot (group-major order) size + 1 within-group
// bins (count 0 .. size of its group) and ngroups across-group bins (count 0 .. ngroups - 1 of the OTHER groups), then
// one distinct counter per operand.
struct KhBmpPivotGroup {            // operands [first, first + size): genomes; [first + size, first + size + npiv): pivots
    u32 first, size, npiv;
    u32 q0;                         // the group's first pivot (group-major pivot number)
    u32 prow;                       // its row of `present` (npiv != 0 only)
    u32 pad;
};
struct KhBmpPivot { u32 op, group, bin0, abin0; };    // operand number, group, first within-group bin, first across-group bin
struct KhBmpPivotJob {
    const KhBmpOp* ops;             // [nops]
    const KhBmpPivotGroup* groups;  // [ngroups]
    const KhBmpPivot* pivots;       // [npivots]
    const u64* partial;             // [splits][nwords], written by k_bmp_build
    u64* present;                   // [groups with pivots][nwords] scratch: a word is stored and read back by one lane
    unsigned long long* hist;       // [reps][nbins + nops] zeroed
    u64 nwords;
    u32 nops, ngroups, npivots, nbins, reps;
};
void kh_launch_bmp_pivot(const KhBmpPivotJob& job, u32 grid, u32 waves, hipStream_t st);   // launch shape and LDS of the read-out

// ---- experiment type 3 from the same bitmaps (k_bmp_cross): the operands of k_bmp_build are the genomes in group-major
// order, then all pivots (read sets).  A launch takes a batch of pivots against every group.  Bins of a launch: per pivot
// of the batch one per genome (count 1 .. size of group g at groups[g].bin0 ..), then one distinct counter per operand
// of the launch (the batch's pivots, then the genomes).
constexpr u32 KH_BMP_CROSS_PIVOTS = 64;    // pivots of a launch at most: their words stay in LDS, 512 bytes each
struct KhBmpCrossJob {
    const KhBmpOp* ops;             // the build's table: genomes [0, ngenomes), then the pivots
    const KhBmpGroup* groups;       // [ngroups]: first = the group's first genome, bin0 = genomes in front of it
    const u64* partial;             // [splits][nwords], written by k_bmp_build
    unsigned long long* hist;       // [reps][nbins + npivots + ngenomes] zeroed, this launch's own
    u64 nwords;
    u32 pop0, npivots;              // the batch: build operands [pop0, pop0 + npivots)
    u32 ngenomes, ngroups;
    u32 nbins, reps;                // nbins = npivots * ngenomes
};
size_t kh_bmp_cross_lds_bytes(u32 nbins, u32 npivots, u32 ngenomes, u32 waves);
void kh_launch_bmp_cross(const KhBmpCrossJob& job, u32 grid, u32 waves, hipStream_t st);   // launch shape of the read-out

// ---- experiment type 4 from the same bitmaps (kh_exp4_run): the operands of k_bmp_build are the genomes in group-major
// order, then all pivots.  k_bmp_count adds up the pivots' multiplicities in tables of 4^k cells, k_bmp_present walks the
// bitmaps like k_bmp_readout (within-group bins, distinct counters, the groups' presence words, the pivots' own words and
// their popcounts per block of 64 words), k_bmp_member writes one (membership mask, count) record per pivot k-mer in
// ascending code order.  Bins: per group size + 1, then one distinct counter per operand.
constexpr u32 KH_BMP_MEMBER_GROUPS = 64;   // one mask word per record
struct KhBmpMemberJob {
    const KhBmpSplit* splits;       // the build's table; the pivots' splits are its last npsplits entries
    const KhBmpOp* ops;             // [nops]
    const KhBmpGroup* groups;       // [ngroups]
    const u64* partial;             // [splits][nwords], written by k_bmp_build
    u64* present;                   // [ngroups][nwords]: codes any genome of the group holds
    u64* pword;                     // [npivots][nwords]: the pivot's bitmap, its splits ORed
    u32* cnt;                       // [npivots][ncells] zeroed: occurrences of every code in the pivot (not saturated)
    u32* blk;                       // [npivots][nblocks]: distinct codes of the pivot in every block of 64 words
    unsigned long long* hist;       // [reps][nbins + nops] zeroed
    const u64* rec_off;             // [npivots]: the pivot's first record
    u64* rec_mask;                  // records, struct of arrays: bit d = group d holds the k-mer
    u32* rec_count;                 //                            min(occurrences, pivot_cs)
    u64 nwords, ncells;             // ncells = 64 * nwords
    u32 nops, ngenomes, ngroups, npivots, nbins, reps, nblocks;
    u32 psplit0, npsplits;          // the pivots' splits
    u32 tile_pos, pivot_cs;
    int k;
};
size_t kh_bmp_member_lds_bytes(u32 ngroups);
void kh_launch_bmp_count(const KhBmpMemberJob& job, hipStream_t st);     // one workgroup per split of a pivot
void kh_launch_bmp_present(const KhBmpMemberJob& job, u32 grid, u32 waves, hipStream_t st);   // launch shape and LDS of the read-out
void kh_launch_bmp_member(const KhBmpMemberJob& job, hipStream_t st);    // (runs of blocks) x pivots workgroups

// ---- experiment type 6 from the same bitmaps (kh_exp6_run): the operands of k_bmp_build are the genomes in group-major
// order; k_bmp_present with no pivots leaves the within-group bins, the distinct counters and present[ngroups][nwords].
// k_bmp_group_masks transposes `present` into the mask table of the votes: table[code * mwords + j] (64 * nwords codes,
// mwords = max(1, (ngroups + 63) / 64) = KhReadsJob::nwords), bit g & 63 of word g >> 6: group g holds canonical code
// `code`.  Every cell is written, the bits of groups >= ngroups are 0.
void kh_launch_bmp_group_masks(const u64* present, u64* table, u64 nwords, u32 ngroups, u32 mwords, hipStream_t st);

struct KhLookback {      // workspace of one ordered single-pass launch
    u64* desc;           // [nparts] tile descriptors, zeroed before launch
    u32* ticket;         // zeroed before launch
    u32* err;            // sticky error bits
    // Part order.  0: part = blockIdx.x, relying on workgroups being started in index order
    // (what the hardware does; saves a device-wide atomic and its round trip at every
    // workgroup start).  1: parts are handed out by an atomic ticket, which needs no such
    // assumption.  The host starts with 0 and switches a context to 1 for good if a look-back
    // ever times out (KH_ERR_SPIN_TIMEOUT), re-running the launch.
    u32 dynamic;
};
enum : u32 { KH_ERR_SPIN_TIMEOUT = 1u, KH_ERR_CAPACITY = 2u, KH_ERR_ORDER = 4u };

size_t kh_extract_lds_bytes(u32 nb_alloc);
size_t kh_sort_lds_bytes(int W, u32 cap, bool pay);

void kh_launch_extract(int W, bool scatter, const u8* seq, const KhSeg* segs, const KhTile* tiles,
                       u32 ntiles, u32 nb_alloc, int k, u32* thist, const u64* bstart, void* part,
                       u32 tile_pos, hipStream_t st);   // tile_pos: k-mer positions per workgroup, a multiple of 16384
void kh_launch_col_totals(const KhSeg* segs, u32 nseg, u32 max_nb, const u32* thist, u64* tot,
                          hipStream_t st);
// over / over_cap: grid mode only (else nullptr / 0): buckets of more than over_cap keys are listed in over[1..], over[0] = count
void kh_launch_col_offsets(const KhSeg* segs, u32 nseg, u32 max_nb, u32* thist, const u64* bstart,
                           const u32* rank, const u64* seg_out_base, KhBucketWork* work, u32* over, u32 over_cap,
                           hipStream_t st);
size_t kh_exscan_tmp_words(u64 n);
void kh_launch_exscan(const u64* in, u64* out, u64 n, u64* tmp, hipStream_t st);   // out has n+1 entries
void kh_launch_bucket_sort(int W, const void* part, const KhBucketWork* work,
                           u32 nbuckets, int k,
                           void* out_keys, u32* out_counts, KhLookback lb, u32 ci, u32 cx, u32 cs,
                           hipStream_t st);
// pass C in grid mode: k_grid_bucket over all buckets (three workgroups per CU; buckets above the LDS
// capacity skipped) + k_grid_oversize over the list k_col_offsets made of those
u32 kh_grid_bucket_capacity(int W);
void kh_launch_grid_bucket(int W, const void* part, const KhBucketWork* work, u32 nbuckets, int k, void* out_keys,
                           const u32* over, u32* err, const KhGrid& grid, hipStream_t st);
size_t kh_tag_lds_bytes(int W, u32 cap, u32 nbins);
// one-word keys, nothing emitted: the hash-set form (k_union_hash), one workgroup per slot
u32 kh_union_hash_capacity();
void kh_launch_union_hash(const KhTagJob& job, u32 grid, int k, u32 cs, hipStream_t st);
void kh_launch_union_tagged(int W, const KhTagJob& job, u32 grid, int k, u32 cs, hipStream_t st);
void kh_launch_range_bounds(int W, const KhSetView* sets, u32 nsets, u32 nranges, int k,
                            u64* bounds, u64* zero, u64 zero_words, hipStream_t st);
void kh_launch_range_bounds_batch(int W, const KhBoundsJob* jobs, u32 njobs, u64 max_threads, int k,
                                  hipStream_t st);
void kh_launch_setop(int W, bool pay, u32 cap, const KhSetopBatch& batch, u32 njobs, int k, int op, int mode,
                     u32 cs, u32 hist_len, bool dynamic_order, hipStream_t st);
void kh_launch_histogram(const u32* counts, u64 n, unsigned long long* hist, u32 hist_len,
                         hipStream_t st);
void kh_launch_unmix(int W, const void* in, void* out, u64 n, int k, hipStream_t st);
void kh_launch_fill_u32(u32* p, u64 n, u32 v, hipStream_t st);
void kh_launch_membership(int W, const void* pivot, u64 n, const KhSetView* sets, u32 nsets, int k,
                          u32 nwords, u64* masks, hipStream_t st);
// ---- read-level votes (kh_reads.hip; src/merge_lists.py:151-183 but for the draw) ----
// One batch of whole reads: read i is buf[off[i], off[i + 1] - 1), the byte behind it is '\n'.
constexpr u32 KH_READS_MAX_SETS = 1024;   // k_read_fold keeps 8 bytes of LDS per set and wave
struct KhReadsJob {
    const u8* buf;           // the batch's text
    u64 npos;                // its bytes = off[nreads]
    const u64* off;          // [nreads + 1], relative to buf
    u32 nreads;
    u32 read0;               // index of the batch's first read in the whole call (error reports)
    const KhSetView* sets;
    const KhSetView* check;  // one view, or nullptr
    u32 nsets, nwords;
    int k;
    u64* masks;              // [npos][nwords]; only positions that start a window are written and read
    u32* ctl;                // [0] read counter of the fold, [1] lowest read with a byte outside ACGT in a window,
                             // [2] lowest read with a k-mer that `check` lacks (both start at 0xffffffff)
};
void kh_launch_read_masks(int W, const KhReadsJob& job, hipStream_t st);
// the masks by direct address (k <= KH_BMP_INST_MAX_K): masks[p] = table[canonical code of the window at p], nwords words
// each, the table of k_bmp_group_masks.  job.sets and job.check are not read.
void kh_launch_read_lookup(const KhReadsJob& job, const u64* table, hipStream_t st);
// inv[L] = 1.0 / L for L = 0 .. 64 * nwords (host IEEE division; [0] unused); tie [nreads][nwords];
// votes [nreads][nsets] or null; unmatched [nreads] or null
void kh_launch_read_fold(const KhReadsJob& job, const double* inv, u64* tie, double* votes, u32* unmatched, u32 grid,
                         hipStream_t st);
// ---- merged mask index (kh_index.hip, kh_index_device.h): the union of nsets sorted sets, every key with the mask of
// the sets that hold it, behind a bucket directory over the mixed key space.
struct KhIndexView {
    const void* keys;        // [n] distinct MIXED keys, ascending (nullptr when n == 0)
    const u64* masks;        // [n][mwords]: bit d & 63 of word d >> 6 = sets[d] holds the key (the numbering of k_membership)
    const u64* dir;          // [nb + 1]: dir[b] = first record whose kh_slot(key, k, nb) is at least b; dir[0] = 0, dir[nb] = n
    u64 n;
    u32 nb;                  // buckets, 1 .. 2^31
    u32 mwords;              // max(1, (nsets + 63) / 64)
};
// dir of `v` from its keys: n + 1 threads, every entry written exactly once
void kh_launch_index_dir(int W, const KhIndexView& v, u64* dir, int k, hipStream_t st);
// masks of `v` (zeroed by the caller on the same stream) from the sets: bit d for every key of sets[d]; a key that the
// index lacks sets *err (zeroed by the caller).  max_n: keys of the largest set
void kh_launch_index_tag(int W, const KhIndexView& v, u64* masks, const KhSetView* sets, u32 nsets, u64 max_n, int k, u32* err,
                         hipStream_t st);
// out[i][mwords] = the mask of probe[i] (mixed keys, any order), zeros for a key the index lacks
void kh_launch_index_member(int W, const KhIndexView& v, const void* probe, u64 n, int k, u64* out, hipStream_t st);
// the masks of a batch of reads from the index: the contract of kh_launch_read_masks (job.sets is not read, job.check is)
void kh_launch_read_index(int W, const KhReadsJob& job, const KhIndexView& v, hipStream_t st);
void kh_launch_table_add(const void* keys, u64 n, int k, void* table, u32 cell_bytes, hipStream_t st);
void kh_launch_table_hist(const void* table, u32 cell_bytes, u64 lo, u64 hi, u32 cs,
                          unsigned long long* hist, u32 hist_len, hipStream_t st);
