/* khoice_hip.h — C ABI of libkhoice_hip.so, the MI355X (gfx950) k-mer engine.
 *
 * The reference (vshiv18/khoice) has no FFI: its boundary to the k-mer engine is
 * process + argv + files, i.e. Snakemake `shell:` calls to KMC 3.2.1's `kmc` and
 * `kmc_tools`.  Each entry point below is what a binding for one of those call forms
 * would bind; the reference call site it replaces is cited as file:line into
 * /root/reference.  The `kmc` / `kmc_tools` executables shipped in bin/ are thin argv
 * parsers over exactly these functions.
 *
 * Conventions
 *   - plain C types only; handles are opaque pointers owned by the library
 *   - every function returns 0 on success or a negative KH_E_* code; the message of the
 *     last failure on the calling thread is kh_last_error()
 *   - a kh_ctx owns one HIP stream on one device; calls on one ctx must not overlap,
 *     different ctxs may be used from different threads / processes concurrently
 *   - k-mers are 2k-bit integers, first base most significant, A=0 C=1 G=2 T=3;
 *     host-side key arrays use W = ceil(2k/64) little-endian 64-bit words per key
 *   - there is NO CPU fallback: without a usable HIP device every call fails
 *   - counters and cs are 32-bit: every set operation combines the whole counters of its
 *     operands (sums and differences in 64-bit arithmetic) and saturates the result at cs, so
 *     any counter and any cs in [1, 2^32 - 1] is exact; a counter of 0 never occurs in a set
 */
#ifndef KHOICE_HIP_H
#define KHOICE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kh_ctx kh_ctx;
typedef struct kh_set kh_set;

enum {
    KH_OK = 0,
    KH_E_ARG = -1,      /* bad argument */
    KH_E_HIP = -2,      /* HIP runtime error */
    KH_E_IO = -3,       /* file error */
    KH_E_FORMAT = -4,   /* not a khoice_amd database */
    KH_E_KMISMATCH = -5,/* operands built with different k */
    KH_E_CAPACITY = -6, /* a bucket could not be fitted after retries */
    KH_E_INTERNAL = -7,
    KH_E_NOMEM = -8
};

/* set operations of `kmc_tools simple` / `complex` */
enum { KH_UNION = 0, KH_INTERSECT = 1, KH_KMERS_SUBTRACT = 2, KH_COUNTERS_SUBTRACT = 3 };
/* counter calculation modes, `-oc<mode>` */
enum { KH_MODE_MIN = 0, KH_MODE_MAX = 1, KH_MODE_SUM = 2, KH_MODE_DIFF = 3,
       KH_MODE_LEFT = 4, KH_MODE_RIGHT = 5 };

#define KH_NO_MAX 0xffffffffu          /* cx: no upper cut-off */
#define KH_KMC_DEFAULT_CS 255u         /* kmc / kmc_tools default counter saturation */

/* ---------------------------------------------------------------- context */
int kh_ctx_create(int device, kh_ctx **out);
void kh_ctx_destroy(kh_ctx *ctx);
const char *kh_last_error(void);
int kh_device_count(void);
/* JSON: device, op counts, bytes/keys processed, per-kernel-class time when profiling
   (text_packed: bytes of sequence text copied into a batch buffer; a device text at a multiple of 16 adds none) */
int kh_stats(kh_ctx *ctx, char *buf, size_t buflen);
/* record HIP events around every kernel class (adds a sync when stats are read) */
int kh_profile_enable(kh_ctx *ctx, int on);
int kh_stats_reset(kh_ctx *ctx);
int kh_sync(kh_ctx *ctx);
/* release cached device allocations */
int kh_trim(kh_ctx *ctx);

/* ---------------------------------------------------------------- K1: build
 * `kmc -fm -m64 -k{k} -ci1 IN.fna.gz OUT tmp/`   workflow/rules/exp_type_1.smk:163
 * (also exp_type_2.smk:297,306; exp_type_3.smk:183,192; exp_type_4.smk:143,152;
 * exp_type_6.smk:171,181).  Canonical counting; symbols other than ACGTacgt break a run;
 * keep ci <= count <= cx; counters saturate at cs.
 *
 * kh_build_batch: nseq sequences in ONE launch sequence.  seqs[i] points at len[i] bytes
 * of cleaned sequence text (records separated by any non-ACGT byte, e.g. '\n'); host
 * pointers when on_device == 0, device pointers (any alignment) when on_device != 0.
 * with_counts == 0 builds plain sets (every counter 1): the fused form of
 * `kmc ...` followed by `kmc_tools transform ... set_counts 1` (exp_type_1.smk:163+173).
 */
int kh_build_batch(kh_ctx *ctx, int nseq, const uint8_t *const *seqs, const uint64_t *lens,
                   int on_device, int k, uint32_t ci, uint32_t cx, uint32_t cs, int with_counts,
                   kh_set **out_sets);
/* one (gz) multi-FASTA file -> one set; host ingest (inflate + record parsing) included */
int kh_build_fasta(kh_ctx *ctx, const char *path, int k, uint32_t ci, uint32_t cx, uint32_t cs,
                   kh_set **out);
/* ingest only: cleaned sequence text of a (gz) multi-FASTA; caller frees with kh_free_host */
int kh_read_fasta(const char *path, uint8_t **seq, uint64_t *len);
void kh_free_host(void *p);

/* Batched ingest (the inputs the dataset_N/GENOME.fna.gz files of exp_type_1.smk:44-47,158):
 * nfiles (gz) multi-FASTA files -> cleaned sequence text RESIDENT IN DEVICE MEMORY, exactly the
 * bytes kh_read_fasta returns.  nthreads host threads inflate the files (0 = one per
 * core, at most 32); files are shipped and cleaned on the device as they complete, overlapping
 * the inflation of the others.  The texts are read in place by kh_build_batch / kh_exp1_run
 * (on_device = 1): kh_seqs_get gives pointer and length of text i; kh_seqs_free releases them. */
typedef struct kh_seqs kh_seqs;
int kh_ingest_fasta(kh_ctx *ctx, int nfiles, const char *const *paths, int nthreads, kh_seqs **out);
int kh_seqs_count(const kh_seqs *seqs);
int kh_seqs_get(const kh_seqs *seqs, int i, const uint8_t **dev_ptr, uint64_t *len);
void kh_seqs_free(kh_seqs *seqs);

/* ---------------------------------------------------------------- K2: set_counts
 * `kmc_tools transform IN set_counts {v} OUT`     exp_type_1.smk:173,241
 * O(1): the result shares IN's key storage and carries a uniform counter. */
int kh_set_counts(kh_ctx *ctx, const kh_set *in, uint32_t value, kh_set **out);

/* ---------------------------------------------------------------- K3: complex union
 * `kmc_tools complex OPS.txt` with  out = (set1 + set2 + ... ), OUTPUT_PARAMS -cs{cs}
 * ops file written at exp_type_1.smk:52-61,75-84; call sites :182,:250.
 * Counters add and saturate at cs.  hist (optional, may be NULL) receives the counter
 * histogram of the result fused into the same pass (K4): hist[c] for c in [0,hist_len),
 * counters >= hist_len fall into the last bin. */
int kh_union_sum(kh_ctx *ctx, const kh_set *const *sets, int nsets, uint32_t cs, kh_set **out,
                 uint64_t *hist, uint32_t hist_len);

/* The fused histogram alone (exp_type_1.smk:243-259 when the caller keeps no step_7 database;
 * the merged slices of the multi-GPU exchange): same counters as kh_union_sum, no set handle. */
int kh_union_histogram(kh_ctx *ctx, const kh_set *const *sets, int nsets, uint32_t cs,
                       uint64_t *hist, uint32_t hist_len);

/* ---------------------------------------------------------------- K5/K6: simple
 * `kmc_tools simple A B intersect OUT -ocsum`     exp_type_2.smk:363-365,479-481
 * `kmc_tools simple A B kmers_subtract OUT`       exp_type_2.smk:377-379,493-495
 * op: KH_UNION | KH_INTERSECT | KH_KMERS_SUBTRACT | KH_COUNTERS_SUBTRACT */
int kh_simple(kh_ctx *ctx, const kh_set *a, const kh_set *b, int op, int mode, uint32_t cs,
              kh_set **out);

/* ---------------------------------------------------------------- K4: histogram
 * `kmc_tools transform IN histogram OUT.txt`      exp_type_1.smk:191,259
 * hist[c], c in [0, hist_len); counters >= hist_len are added to the last bin. */
int kh_histogram(kh_ctx *ctx, const kh_set *set, uint64_t *hist, uint32_t hist_len);
/* Small-k form of the across-group occurrence count (exp_type_1.smk:243-259 for k <= 16): a
 * direct-addressed table of 4^k cells in DEVICE memory (cell_bytes 1 or 4, caller-owned, zeroed by
 * the caller); kh_table_add_set adds 1 (saturating) to the cell of every k-mer of `set`, so after
 * adding each group set once, cell v = number of groups holding canonical k-mer v.  Tables of
 * several GPUs are summed by the caller (RCCL all-reduce).  kh_table_histogram:
 * hist[min(cell, cs, hist_len-1)] += 1 over the non-zero cells of [lo, hi) (cs 0 = no cap);
 * lo*cell_bytes must be a multiple of 16.  Work is queued on the context's stream. */
int kh_table_add_set(kh_ctx *ctx, const kh_set *set, void *d_table, uint32_t cell_bytes);
int kh_table_histogram(kh_ctx *ctx, const void *d_table, uint32_t cell_bytes, uint64_t lo, uint64_t hi,
                       uint32_t cs, uint64_t *hist, uint32_t hist_len);
/* ---------------------------------------------------------------- experiment type 4
 * Replaces the text dumps + Python dict of src/merge_lists.py:14-33 (build_dictionary /
 * update_dictionary; rules exp_type_4.smk:247-294): for every k-mer of `pivot` (with its count),
 * which of `sets` hold it.  Outputs are HOST arrays in `dump -s` order (ascending canonical
 * key): keys_out[n*W] (may be NULL), counts_out[n] (may be NULL), masks_out[n*nwords] with
 * nwords = max(1, (nsets+63)/64), bit d%64 of word d/64 = "sets[d] holds the k-mer". */
int kh_membership(kh_ctx *ctx, const kh_set *pivot, const kh_set *const *sets, int nsets,
                  uint64_t *keys_out, uint32_t *counts_out, uint64_t *masks_out);
/* One feature-level confusion-matrix row, summed in the reference's order and arithmetic
 * (src/merge_lists.py:122-141): row[d] (d < nsets) = sum over pivot k-mers held by the sets M
 * of 1/len(M)*count for d in M; *unique_pivot_count = sum of counts of k-mers no set holds. */
int kh_confusion_row(kh_ctx *ctx, const kh_set *pivot, const kh_set *const *sets, int nsets,
                     double *row, uint64_t *unique_pivot_count);
/* ---------------------------------------------------------------- experiment type 6 (read level)
 * src/merge_lists.py:151-183 for one pivot, everything but the draw.  For every read, in text order, each k-mer that
 * the sets M hold adds 1/len(M) to the vote of every set in M (:165-171: one rounding per addition, in window order,
 * bit for bit what CPython computes); the read then belongs to a set of the highest vote, drawn among the ties by
 * random.choice (:178-180).  The draw is the caller's: this returns the ties.
 *   reads, read_off      read i is reads[read_off[i] .. read_off[i+1]-1) and one '\n' follows every read, so
 *                        read_off[nreads] is the length of the text.  `reads` is a host or a device buffer
 *                        (on_device; the layout of a device buffer is not checked), read_off always a host array
 *   sets, check          what kh_membership takes: only the keys are read.  check (may be NULL) stands for the pivot
 *                        dictionary of :167
 *   tie_masks [nreads * nwords], nwords = max(1, (nsets+63)/64): bit d%64 of word d/64 = "sets[d] has the highest
 *                        vote of the read".  A read without k-mers has every vote 0.0: all sets tie
 *   votes [nreads * nsets] (may be NULL), unmatched [nreads] (may be NULL): the k-mers of the read no set holds
 * KH_E_ARG: nsets < 1 (the reference's max([]) raises), more than 1024 sets, k outside 1..64, a read of at least k
 * bytes with a byte outside upper-case ACGT (KeyError at :66), with `check` a k-mer it does not hold (KeyError at
 * :167); the message names the lowest such read.  KH_E_KMISMATCH: a set of another k.  A read shorter than k may hold
 * any bytes but '\n'; nreads == 0 is KH_OK.  On an error the outputs are unspecified.
 * The masks of all windows take 8 * nwords bytes per byte of text on the device: a text above a quarter of the free
 * memory runs as batches of whole reads (KHOICE_READS_MAX_POS lowers that budget, in bytes of text). */
int kh_read_votes(kh_ctx *ctx, const uint8_t *reads, const uint64_t *read_off, uint64_t nreads, int on_device,
                  int k, const kh_set *const *sets, int nsets, const kh_set *check /* may be NULL */,
                  uint64_t *tie_masks /* [nreads*nwords] */, double *votes /* [nreads*nsets] or NULL */,
                  uint32_t *unmatched /* [nreads] or NULL */);
/* ---------------------------------------------------------------- merged mask index
 * The union of nsets sets as ONE device-resident table: n distinct keys (mixed, ascending), per key the mask of the
 * sets that hold it (mask_words = max(1, (nsets+63)/64) words, bit d%64 of word d/64 = "sets[d] holds the key", the
 * numbering of kh_membership) and a directory of nbuckets = clamp(ceil(n / 4), 1, 2^31) equal-width buckets of the
 * mixed key space in front (KHOICE_INDEX_BUCKET_KEYS, read per build, replaces the 4).  A lookup is one directory read
 * and a bisection inside one bucket, whatever nsets is; it is exact for any distribution of the keys.  Any k from 1 to
 * 64; only the keys of the sets are read; empty sets are fine, and all sets empty give a valid index with n = 0 in
 * which every lookup misses.  The index keeps no reference to the sets: it outlives them.
 * KH_E_ARG: nsets < 1, more than 1024 sets, a NULL set.  KH_E_KMISMATCH: sets of different k.  KH_E_NOMEM: the index
 * does not fit. */
typedef struct kh_index kh_index;
int kh_index_build(kh_ctx *ctx, const kh_set *const *sets, int nsets, kh_index **out);
void kh_index_free(kh_index *index);
/* any output may be NULL */
int kh_index_info(const kh_index *index, uint64_t *n, int *k, int *nsets, int *mask_words, uint64_t *nbuckets);
/* HOST arrays in the index's storage order: keys[n*W] as kh_set_download gives them for the union of the sets (may be
 * NULL), masks[n*mask_words] (may be NULL) */
int kh_index_download(kh_ctx *ctx, const kh_index *index, uint64_t *keys /* as kh_set_download of the union */,
                      uint64_t *masks /* [n*mask_words] */);
/* The search of kh_membership against an index: for every key of `probe`, in the probe's STORAGE order (the order of
 * kh_set_download, not dump order), the mask of the sets that hold it; zeros for a key the index lacks.
 * KH_E_KMISMATCH: a probe of another k. */
int kh_index_masks(kh_ctx *ctx, const kh_index *index, const kh_set *probe,
                   uint64_t *masks_out /* [probe n * mask_words], probe's storage order */);
/* kh_read_votes against the sets an index was built from (k and nsets are the index's): the same reads, outputs,
 * batches and errors, the same numbers bit for bit, but one lookup per k-mer of a read instead of a search in every
 * set.  KH_E_KMISMATCH: a check set of another k. */
int kh_read_votes_index(kh_ctx *ctx, const uint8_t *reads, const uint64_t *read_off, uint64_t nreads, int on_device,
                        const kh_index *index, const kh_set *check /* may be NULL */,
                        uint64_t *tie_masks /* [nreads*mask_words] */, double *votes /* [nreads*nsets] or NULL */,
                        uint32_t *unmatched /* [nreads] or NULL */);

/* text form consumed at exp_type_1.smk:210-212: lines "c<TAB>n", c = 1..cmax; counters above cmax are added to line
 * cmax (kh_histogram with hist_len = cmax + 1).  KH_E_ARG: cmax = 0 or above 2^24 - 1; no file is written */
int kh_histogram_file(kh_ctx *ctx, const kh_set *set, uint32_t cmax, const char *path);

/* the same text from a histogram array in host memory (what kh_exp1_run returns): counters past
 * hist_len read 0; entries of the array past cmax are not written and NOT added to line cmax (the array is taken as
 * the histogram it is).  KH_E_ARG: cmax = 0 or above 2^24 - 1 */
int kh_write_histogram_text(const char *path, const uint64_t *hist, uint32_t hist_len, uint32_t cmax);

/* ---------------------------------------------------------------- K7: sorted dump
 * `kmc_tools transform IN dump -s OUT.txt`        exp_type_4.smk:255-257,268-270
 * lines "KMER<TAB>count", sorted A<C<G<T (consumer src/merge_lists.py:19-22). */
int kh_dump_sorted(kh_ctx *ctx, const kh_set *set, const char *path);

/* ---------------------------------------------------------------- set handles */
void kh_set_free(kh_set *set);
int kh_set_info(const kh_set *set, uint64_t *n, int *k, int *words_per_key, int *has_counts,
                uint32_t *uniform_count);
/* saturation value the set's counters were produced with (kmc -cs, OUTPUT_PARAMS -cs, or the
 * kmc_tools default 255); `kmc_tools transform histogram` prints 2^(8*bytes(counter_max))-1 lines.
 *   kh_build_batch / kh_build_fasta (cs), kh_union_sum (cs), kh_simple (cs)   cs
 *   kh_set_counts (value)                                                     max(value, 255), not the input's
 *   kh_load                                                                   what kh_save wrote
 *   kh_set_upload, kh_set_from_device, kh_set_wrap_device                     255: these do NOT look at the counters
 *                                                                             they are given, which may be larger */
int kh_set_counter_max(const kh_set *set, uint32_t *counter_max);
/* copy to host in storage order (NOT sorted by key): keys un-mixed, n*W words; counts n */
int kh_set_download(kh_ctx *ctx, const kh_set *set, uint64_t *keys, uint32_t *counts);
/* build a set from host arrays of DISTINCT keys in any order (counts may be NULL => 1); a key of
 * 4^k or more, or a counter of 0, fails with KH_E_ARG */
int kh_set_upload(kh_ctx *ctx, int k, uint64_t n, const uint64_t *keys, const uint32_t *counts,
                  kh_set **out);
/* raw device views for zero-copy exchange (multi-GPU): mixed keys sorted ascending,
 * counts NULL when uniform.  Valid until the set is freed. */
int kh_set_device_ptrs(const kh_set *set, const void **keys_mixed, const uint32_t **counts);
/* copy the raw storage (mixed keys in storage order; counters, materialised when uniform) into
 * caller-owned DEVICE buffers of n*W*8 and n*4 bytes: the send side of the exchange */
int kh_set_export_device(kh_ctx *ctx, const kh_set *set, void *keys_out, uint32_t *counts_out);
/* the same for elements [lo, hi); stream-ordered on the ctx stream (kh_sync before use elsewhere) */
int kh_set_export_range(kh_ctx *ctx, const kh_set *set, uint64_t lo, uint64_t hi, void *keys_out,
                        uint32_t *counts_out);
/* zero-copy handle over caller-owned device arrays (mixed keys ascending and distinct; counts may
 * be NULL => every counter == uniform): the receive side of the exchange.  The arrays must stay
 * alive and unchanged until kh_set_free. */
int kh_set_wrap_device(kh_ctx *ctx, int k, uint64_t n, const void *keys_mixed, const uint32_t *counts,
                       uint32_t uniform, kh_set **out);
/* wrap device arrays of already mixed, sorted, distinct keys (copied into the library) */
int kh_set_from_device(kh_ctx *ctx, int k, uint64_t n, const void *keys_mixed,
                       const uint32_t *counts, kh_set **out);
/* index of the first key of every one of `nparts` equal-width slots of the mixed key
 * space: bounds[nparts+1] (host).  Used to slice a set for the all-to-all exchange. */
int kh_set_partition_bounds(kh_ctx *ctx, const kh_set *set, uint32_t nparts, uint64_t *bounds);
/* the same for nsets sets in one launch: bounds[nsets][nparts+1] */
int kh_sets_partition_bounds(kh_ctx *ctx, const kh_set *const *sets, int nsets, uint32_t nparts,
                             uint64_t *bounds);

/* ---------------------------------------------------------------- database files
 * `<prefix>.kmc_pre` + `<prefix>.kmc_suf` (names required by the Snakemake rules,
 * exp_type_1.smk:160-161); khoice_amd container format ("Database files"), written atomically: each file
 * through a temporary in the same directory and a rename; a failed save leaves no partial file.
 * kh_load returns KH_E_IO for a file that cannot be opened and KH_E_FORMAT, before anything is allocated on the
 * device, for a header that is not this format's (magic, version, k, words, mixing fingerprint, no counters with a
 * uniform counter of 0), a suffix file whose size is not the header's, and a body whose keys do not ascend, are not
 * distinct or lie outside the 2k-bit key space, or that holds a zero counter.  The message names the file and, for
 * the body, the first offending record. */
int kh_save(kh_ctx *ctx, const kh_set *set, const char *prefix);
int kh_load(kh_ctx *ctx, const char *prefix, kh_set **out);

/* ---------------------------------------------------------------- fused experiment type 1
 * The whole device side of exp_type_1.smk:156-259 for one k on resident sequences:
 * per genome build+set (steps 1-2), per group union-sum + histogram (steps 3-4),
 * group sets (step 6), across-group union-sum + histogram (steps 7-8).
 *   group_of[i]    group index (0-based) of sequence i; ngroups groups
 *   within_hist    [ngroups * hist_len]  step_4 histograms
 *   across_hist    [hist_len]            step_8 histogram
 *   distinct_per_seq [nseq]              distinct canonical k-mers of each genome
 *   group_sets     optional [ngroups]: the step_3 group unions (caller frees)
 *   across_set     optional: the step_7 union (caller frees)
 * When across_hist and across_set are both NULL steps 7-8 are skipped (multi-GPU callers run
 * them after the exchange of the group sets).
 *
 * Forms.  With group_sets the call builds per-genome sets and unions them (the general path).  Without, one of
 * three fused forms answers, the same numbers in each:
 *   k <= 12, no across_set      presence bitmaps (kh_bmp.hip): one bit per genome and k-mer code in directly
 *                               addressed bitmaps built in LDS, counted with bit-sliced counters; no 64-genome
 *                               mask: up to 1023 genomes per group, 1023 groups, 4096 histogram bins in one pass
 *   17 <= k <= 63, no across_set  super-k-mer records (kh_skm.hip, kh_skm2.hip)
 *   otherwise                   key arrays (k = 13..16, k = 64, across_set, and whatever the other two decline)
 * Switches (environment): KHOICE_NO_BMP, KHOICE_NO_SKM (also keeps the bitmaps off: "the key arrays, please"),
 * KHOICE_BMP_MAX_K (up to 13), KHOICE_BMP_MAX_BYTES (memory the partial bitmaps may take), KHOICE_NO_FUSED.
 */
int kh_exp1_run(kh_ctx *ctx, int nseq, const uint8_t *const *seqs, const uint64_t *lens,
                int on_device, const int *group_of, int ngroups, int k, uint32_t cs,
                uint64_t *within_hist, uint64_t *across_hist, uint32_t hist_len,
                uint64_t *distinct_per_seq, kh_set **group_sets, kh_set **across_set);

/* ---------------------------------------------------------------- fused experiment type 2
 * The device side of exp_type_2.smk:289-507 for one k on resident sequences: a pivot genome was held out of every
 * dataset (group); in how many genomes of its own group, and in how many of the OTHER groups, does each of its k-mers
 * occur?  Replaces per k: `kmc` + `set_counts 1` per genome and pivot (:297,306,318,330), the -cs{cs} `complex` union
 * per group (:342), `simple PIVOT UNION intersect -ocsum` + `transform histogram` (:363-365) and
 * `simple PIVOT UNION kmers_subtract` + histogram (:377-379), `set_counts 1` of the group unions (:391), the
 * `complex` union of the other groups per pivot (:465), and the same intersect / kmers_subtract pair against it
 * (:479-481, :493-495).
 *   seqs, lens, group_of, ngroups   the rest_of_set genomes, as for kh_exp1_run; every group needs a genome
 *   pivot_seqs, pivot_lens          npivots pivot texts (host or device like seqs); pivot_group[p] = the group pivot p
 *                                   was held out of; any number of pivots per group, none included
 * With occ_w[v] = distinct canonical k-mers of pivot p in exactly v genomes of its group (the pivot is not one of
 * them) and occ_a[v] = in exactly v groups other than its own (a group holds what any of its genomes holds):
 *   within_hist  [npivots * hist_len]  bin min(1 + min(v, cs), cs, hist_len - 1) += occ_w[v], v >= 1: the histogram of
 *                                      the intersect -ocsum result (the pivot's counter 1 + the union's, saturating)
 *   within_only  [npivots]             occ_w[0]: bin 1 of the kmers_subtract result
 *   across_hist, across_only           the same over occ_a; one group: no k-mer is met, all are in across_only
 *   distinct_per_seq [nseq], distinct_per_pivot [npivots]   distinct canonical k-mers of every text
 * Any output may be NULL.
 *
 * Forms, the same numbers in each: k <= 12 presence bitmaps (kh_bmp.hip: the pivots are further genomes of the
 * bitmap build, one read-out kernel counts every pivot against its group's and the groups' bit-sliced counters);
 * otherwise, and whenever the bitmaps do not fit (1023 genomes per group, 1023 groups, 4096 bins and counters, the
 * memory budget), the calls above on sets in device memory.  Switches as for kh_exp1_run: KHOICE_NO_BMP,
 * KHOICE_NO_SKM, KHOICE_BMP_MAX_K, KHOICE_BMP_MAX_BYTES.
 *
 * KHOICE_EXP2_SKM=1 (read at the call; any other value or unset: as above) adds a third form for 17 <= k <= 63, at
 * least one pivot and at most 63 genomes: genomes and pivots go through the super-k-mer scatter and regroup of
 * kh_exp1_run as one list of at most 64 operands, and kh_exp3_run's kernel (k_skm_cross) with a read-out of its own
 * counts, per slot, every k-mer of a pivot once by the genomes of its own group that hold it and once by the OTHER
 * groups that do.  A pass takes pivots in the caller's order while genomes + pivots <= 64 and their bins (per pivot
 * the size of its group + 1 + ngroups) <= 1024; further pivots go in further passes, which stage the genomes again.
 * It declines (the set form answers, nothing counted) without a pivot, with 64 genomes or more, for a pass without a
 * k-mer position, where the slot geometry or the memory does not fit, under KHOICE_NO_SKM, and for k > 32 under
 * KHOICE_NO_SKM2; an overflow on the way, or a later pass that does not fit, counts one retry in kh_stats and the set
 * form answers.  KH_E_INTERNAL: a pivot's bins do not add up to its distinct k-mers.  The default above k = 12 stays
 * the set form (DESIGN.md section 3 has the measured table). */
int kh_exp2_run(kh_ctx *ctx, int nseq, const uint8_t *const *seqs, const uint64_t *lens, int on_device,
                const int *group_of, int ngroups, int npivots, const uint8_t *const *pivot_seqs,
                const uint64_t *pivot_lens, const int *pivot_group, int k, uint32_t cs,
                uint64_t *within_hist, uint64_t *across_hist, uint32_t hist_len,
                uint64_t *within_only, uint64_t *across_only,
                uint64_t *distinct_per_seq, uint64_t *distinct_per_pivot);

/* ---------------------------------------------------------------- fused experiment type 3
 * The device side of exp_type_3.smk:176-277 for one k on resident sequences: the simulated reads of every pivot
 * against the rest-of-set union of EVERY dataset (group): how many of the pivot's k-mers lie in exactly v genomes of
 * the group.  Replaces per k: `kmc` per genome and per read set (:183,192), `set_counts 1` of both (:206,219), the
 * -cs{cs} `complex` union per dataset (:233), the pivots x datasets `simple intersect -ocsum` databases (:248-250) and
 * the `transform histogram` of each and of every pivot (:261-263, :274-276).
 *   seqs, lens, group_of, ngroups   the rest_of_set genomes, as for kh_exp1_run; every group needs a genome
 *   pivot_seqs, pivot_lens          npivots read sets (host or device like seqs): cleaned texts, the reads separated by
 *                                   a line feed; a text may be empty or shorter than k; npivots may be 0
 * With occ[v] = distinct canonical k-mers of pivot p in exactly v genomes of group g:
 *   inter_hist [npivots * ngroups * hist_len]   inter_hist[p][g]: bin min(1 + min(v, cs), cs, hist_len - 1) += occ[v],
 *                                   v >= 1: the histogram of the intersect -ocsum result (the pivot's counter 1 + the
 *                                   union's, saturating), the fold of kh_exp2_run's within_hist
 *   distinct_per_seq [nseq], distinct_per_pivot [npivots]   distinct canonical k-mers of every text (line 1 of the
 *                                   pivot's own histogram)
 * Any output may be NULL.  KH_E_ARG: a group outside [0, ngroups), a group without genome, hist_len < 2, k outside
 * 1..64, cs == 0.
 *
 * Forms, the same numbers in each: k <= 12 presence bitmaps (kh_bmp.hip: the pivots are further genomes of the bitmap
 * build; one read-out kernel per batch of pivots keeps their words in LDS and masks the bit-sliced counter of every
 * group with them); otherwise, and whenever the bitmaps do not fit (1023 genomes per group, a pivot whose bins and the
 * operand counters exceed 4096, the memory budget), one batched build, the unions and intersect + histogram on sets in
 * device memory.  Switches as for kh_exp1_run: KHOICE_NO_BMP, KHOICE_NO_SKM, KHOICE_BMP_MAX_K, KHOICE_BMP_MAX_BYTES;
 * KHOICE_BMP_MAX_BINS lowers the 4096 (more, smaller batches of pivots).
 *
 * KHOICE_EXP3_SKM=1 (read at the call; any other value or unset: as above) adds a third form for 17 <= k <= 63, pivots
 * and at most 63 genomes: genomes and read sets go through the super-k-mer scatter and regroup of kh_exp1_run as one
 * list of operands and one kernel (k_skm_cross) reads, per slot, every k-mer's mask of operands out into the same bins
 * as the bitmap form; pivots beyond 64 - nseq go in further passes.  It declines (the set form answers, nothing
 * counted) where the slot geometry or the memory does not fit, under KHOICE_NO_SKM, and for k > 32 under
 * KHOICE_NO_SKM2; an overflow on the way counts one retry in kh_stats and the set form answers.  The default above
 * k = 12 stays the set form until the measured table says otherwise. */
int kh_exp3_run(kh_ctx *ctx, int nseq, const uint8_t *const *seqs, const uint64_t *lens, int on_device,
                const int *group_of, int ngroups,
                int npivots, const uint8_t *const *pivot_seqs, const uint64_t *pivot_lens,
                int k, uint32_t cs,
                uint64_t *inter_hist, uint32_t hist_len,       /* [npivots * ngroups * hist_len] */
                uint64_t *distinct_per_seq, uint64_t *distinct_per_pivot);

/* ---------------------------------------------------------------- fused experiment type 4
 * The device side of exp_type_4.smk:139-303 for one k on resident sequences: every pivot against the rest-of-set
 * union of EVERY dataset (group), summed into one confusion-matrix row per pivot as src/merge_lists.py:101-141 does.
 * Replaces per k: `kmc` per genome and pivot (:143,152), `set_counts 1` per genome (:164-168), the -cs{cs} `complex`
 * union per dataset (:183) and its `transform histogram` (:191-196), `set_counts 1` of the unions (:205-209), the D x D
 * `simple intersect -ocsum` databases (:226-228), every `dump -s` (:247-271) and the dictionaries of
 * src/merge_lists.py:14-33.
 *   seqs, lens, group_of, ngroups   the rest_of_set genomes, as for kh_exp1_run; every group needs a genome
 *   pivot_seqs, pivot_lens          npivots pivot texts (host or device like seqs), each compared against ALL groups;
 *                                   npivots need not equal ngroups and may be 0
 *   within_hist [ngroups * hist_len]   histogram of the -cs{cs} union of group g: bins and clamps of kh_exp1_run
 *   rows [npivots * ngroups], unique_pivot_count [npivots]
 *                                   what kh_confusion_row returns for pivot p built with ci = 1, no cx and
 *                                   counters saturating at pivot_cs (KH_KMC_DEFAULT_CS in the workflow) against the
 *                                   `set_counts 1` unions of the groups: k-mers in ascending canonical key order,
 *                                   1/len(M) then * count, one rounding each, no contraction
 *                                   (src/merge_lists.py:122-141).  Bit-exact: the order of the sum is part of the contract.
 *   distinct_per_seq [nseq], distinct_per_pivot [npivots]   distinct canonical k-mers of every text
 * Any output may be NULL.  KH_E_ARG: a group outside [0, ngroups), a group without genome, hist_len < 2, k outside
 * 1..64, cs == 0, pivot_cs == 0.
 *
 * Forms, the same numbers in each: k <= 12 and at most 64 groups presence bitmaps (kh_bmp.hip: the pivots are further
 * genomes of the bitmap build; their multiplicities are added up in tables of 4^k cells, and one kernel writes a
 * (membership mask, count) record per pivot k-mer in code order, which IS the dump order: nothing is sorted); otherwise,
 * and whenever the bitmaps do not fit (1023 genomes per group, 4096 bins and counters, a pivot of 2^32 positions, the
 * memory budget), builds, unions and the membership search on sets in device memory, whose keys the host sorts.
 * Switches as for kh_exp1_run: KHOICE_NO_BMP, KHOICE_NO_SKM, KHOICE_BMP_MAX_K, KHOICE_BMP_MAX_BYTES. */
int kh_exp4_run(kh_ctx *ctx, int nseq, const uint8_t *const *seqs, const uint64_t *lens, int on_device,
                const int *group_of, int ngroups,
                int npivots, const uint8_t *const *pivot_seqs, const uint64_t *pivot_lens,
                int k, uint32_t cs, uint32_t pivot_cs,
                uint64_t *within_hist, uint32_t hist_len,      /* [ngroups * hist_len] */
                double *rows, uint64_t *unique_pivot_count,    /* [npivots * ngroups], [npivots] */
                uint64_t *distinct_per_seq, uint64_t *distinct_per_pivot);

/* ---------------------------------------------------------------- fused experiment type 6
 * The device side of exp_type_6.smk:164-344 for one k and one read type: the rules of type 4 up to the last one, which
 * runs src/merge_lists.py with -r.  Three forms, tried in this order, the same outputs bit for bit:
 *   bitmap form  k <= 12 (KHOICE_BMP_MAX_K: up to 13; KHOICE_NO_BMP: never), at most 1024 groups of at most 1023
 *                genomes, and the bitmaps and the table within the budget (KHOICE_BMP_MAX_BYTES): presence bitmaps of
 *                the genomes, the groups' presence rows transposed into a table of one mask per canonical code, and
 *                per window of a read one direct-addressed load of its mask; the fold of kh_read_votes unchanged.
 *   index form   any k: the builds, unions and `set_counts 1` of the set form, ONE merged mask index (kh_index_build)
 *                over the groups' sets, and per window of a read one lookup in it (kh_read_votes_index without a
 *                check set); the index is freed before the call returns.  KHOICE_EXP6_INDEX=1 takes the form whenever
 *                it applies, =0 never; unset it is taken when windows * ngroups >= 0.53 * sum |sets| (windows: the
 *                k-mers of all reads; sets: the groups' unions) and sum |sets| >= 3.6e6, the measured break-even
 *                against the set form (profiles/exp6_index.json).  It declines when the index and the workspace of
 *                its union are above a quarter of the free memory (KHOICE_INDEX_MAX_BYTES lowers that budget).
 *   set form     builds, -cs{cs} unions and `set_counts 1` as in the set form of kh_exp4_run, then kh_read_votes for
 *                every pivot's reads against the unions of ALL groups (no check set: every k-mer of a read is in the
 *                database built from the same reads).  It answers wherever the other two do not apply.
 *   pivot_reads[p], pivot_read_off[p], pivot_nreads[p]   the reads of pivot p in the layout of kh_read_votes (host or
 *                                   device like seqs; the offsets always on the host)
 *   within_hist [ngroups * hist_len], distinct_per_seq [nseq]   as for kh_exp4_run; may be NULL
 *   tie_masks [sum(pivot_nreads) * nwords], unmatched [sum(pivot_nreads)]   pivot after pivot; unmatched may be NULL
 * Errors: those of kh_exp4_run's arguments and of kh_read_votes. */
int kh_exp6_run(kh_ctx *ctx, int nseq, const uint8_t *const *seqs, const uint64_t *lens, int on_device,
                const int *group_of, int ngroups,
                int npivots, const uint8_t *const *pivot_reads, const uint64_t *const *pivot_read_off,
                const uint64_t *pivot_nreads,
                int k, uint32_t cs, uint64_t *within_hist, uint32_t hist_len,
                uint64_t *tie_masks /* concatenated per pivot */, uint32_t *unmatched, uint64_t *distinct_per_seq);

/* ---------------------------------------------------------------- multi-GPU exchange (RCCL over xGMI)
 * Steps 7-8 of exp_type_1.smk:243-259 when the groups are sharded over several GPUs, one process
 * per GPU: every rank runs kh_exp1_run on its own groups asking for `across_set` (counter = number
 * of its groups holding the k-mer) and calls kh_across_exchange_histogram; the mixed key space is
 * cut into nranks slots, slices travel by grouped ncclSend / ncclRecv (full mesh), the owner sums
 * the counters (saturating at cs) and the histograms are all-reduced: every rank gets the global
 * step_8 histogram.  kh_comm_unique_id is called on one rank and its 128 bytes handed to the others
 * by whatever launched them (file, socket, MPI); RCCL is loaded on first use. */
#define KH_COMM_ID_BYTES 128
typedef struct kh_comm kh_comm;
int kh_comm_unique_id(char id[KH_COMM_ID_BYTES]);
int kh_comm_init(kh_ctx *ctx, int rank, int nranks, const char id[KH_COMM_ID_BYTES], kh_comm **out);
void kh_comm_destroy(kh_comm *comm);
int kh_across_exchange_histogram(kh_ctx *ctx, kh_comm *comm, const kh_set *local_across_set, uint32_t cs,
                                 uint64_t *hist, uint32_t hist_len);

/* host-side helpers exposed for tests (no device work) */
void kh_mix_host(int k, const uint64_t *key_words, uint64_t *out_words);
void kh_unmix_host(int k, const uint64_t *key_words, uint64_t *out_words);

/* ---------------------------------------------------------------- steps 7-8 across ranks, exchange of records
 * (workflow/rules/exp_type_1.smk:243-259 when the groups live on several GPUs; 17 <= k <= 32).
 * kh_skm_exchange_plan: the slot geometry all ranks must share, from numbers they agreed on (the largest rank's number
 *   of k-mer positions, the largest group of any rank: its genomes bring their copies of a locus into a slot together,
 *   which sizes the slot's region).
 * kh_skm_pack: this rank's genomes -> minimizer records tagged with the LOCAL group number tag_of[i] (0..31), identical
 *   records merged, packed by owner of their slot into CALLER-ALLOCATED device buffers: rec_out [nparts][part_cap] x 16
 *   bytes, mask_out [nparts][part_cap], count_out / off_out [nparts][slots_per_part] (records of a slot and where they
 *   start in their part); part_n[p] (host) = records for part p.  A rank without k-mers (nseq = 0, or every sequence
 *   shorter than k) gets zero counts, offsets and part_n.
 * kh_skm_phased_histogram: on the owner, the pieces received (one per source rank, device pointers) -> hist[c] = number of
 *   distinct k-mers of this rank's slots that occur in c groups of all ranks (c saturating at cs). */
int kh_skm_exchange_plan(kh_ctx *ctx, int k, uint64_t positions_max, uint32_t fan_max, int nparts, uint32_t *nslots,
                         uint32_t *slots_per_part, uint64_t *part_cap);
int kh_skm_pack(kh_ctx *ctx, int nseq, const uint8_t *const *seqs, const uint64_t *lens, int on_device, const int *tag_of,
                int k, uint32_t nslots, int nparts, uint64_t part_cap, void *rec_out, uint32_t *mask_out,
                uint32_t *count_out, uint32_t *off_out, uint64_t *part_n);
int kh_skm_phased_histogram(kh_ctx *ctx, int k, int npieces, const void *const *recs, const uint32_t *const *masks,
                            const uint32_t *const *counts, const uint32_t *const *offs, uint32_t nslots, uint32_t cs,
                            uint64_t *hist, uint32_t hist_len);

#ifdef __cplusplus
}
#endif
#endif /* KHOICE_HIP_H */
