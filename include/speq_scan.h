/*
 * speq_scan.h — C ABI of libspeq_scan.so, the MI355X-native SPeQ scan path.
 *
 * This is the drop-in boundary for the reference's hot path.
 * The reference has no FFI; its seam is the SeqAn3 library call pair
 *
 *   seqan3::fm_index{collection}            /root/reference/src/fm_indexer.cpp:36
 *   search(windows, fm_index, cfg)          /root/reference/src/fm_scanner.cpp:208 (+12 more sites)
 *
 * followed by the per-window tally `do_a_count` (fm_scanner.cpp:153-196, :426-471, :665-708, :916-962),
 * the per-thread reduction (fm_scanner.cpp:224-233 …) and the reference-uniqueness pass
 * `_async_count_unique_kmers_per_group` (fm_scanner.cpp:1476-1576).  The functions below replace that
 * seam AND the tally, so per-window hit lists never materialise: the GPU returns the counters directly.
 *
 * Conventions
 *  - Every function returns 0 on success, a negative SPEQ_E_* code on failure; the message of the last
 *    failure on the calling thread is returned by speq_last_error() (mirrors the reference's exceptions,
 *    e.g. std::logic_error at fm_scanner.cpp:69, which the C++ CLI re-raises).
 *  - Plain pointers and sizes only.  "d_" pointers are device (HBM) pointers of the device the handle was
 *    opened on; "stream" is a hipStream_t passed as void* (NULL = the default stream).
 *  - An index is immutable after build/load; a device replica may be used concurrently from many host
 *    threads (the reference copies the index per worker thread, fm_scanner.cpp:145 — we do not need to).
 *  - Product paths run on the GPU only.  There is no CPU fallback: a call that needs a device fails
 *    with SPEQ_E_DEVICE when none is present.
 */
#ifndef SPEQ_SCAN_H
#define SPEQ_SCAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPEQ_ABI_VERSION 8

enum {
    SPEQ_OK = 0,
    SPEQ_E_ARG = -1,      /* invalid argument (shape, range, null pointer) */
    SPEQ_E_IO = -2,       /* file could not be read / written / has a bad format */
    SPEQ_E_DEVICE = -3,   /* no GPU, HIP runtime failure, or kernel launch failure */
    SPEQ_E_GROUPS = -4,   /* groupings do not cover every reference record */
    SPEQ_E_NOMEM = -5,
    SPEQ_E_RETRY = -6     /* speq_scan_fastq_shard, cut = 1: the parallel cut does not fit this file; counters and
                             EM histogram are cleared, scan again with cut = 0 (every rank) */
};

/* Scan modes: fm_scanner.cpp:5-32 picks "local" (Phred-weighted) when --fixed-accuracy == 0. */
enum { SPEQ_MODE_GLOBAL = 0, SPEQ_MODE_LOCAL = 1 };

typedef struct speq_index speq_index;            /* host-side FM-index (immutable) */
typedef struct speq_device_index speq_device_index; /* replica of an index in one GPU's HBM */

typedef struct {
    uint32_t prefix_q;   /* length of the q-mer interval lookup table (0 = none, max 13) */
    uint32_t threads;    /* host threads for the build (0 = all) */
    uint32_t pair_steps; /* 1: add the 16 two-symbol occ planes (LF over two bases per gather pair) */
    uint32_t label_table;/* 1: add the per-SA-position {group, run distance} table (one-load classification);
                            2: auto (only when the collection has >= 4 M symbols) */
    uint32_t gpu_build;  /* 1: build the suffix array and planes on GPU `device` (prefix doubling on radix sorts);
                            0: host SA-IS. Both produce identical indexes. */
    int32_t device;      /* GPU ordinal for gpu_build */
    uint32_t triple_steps; /* 1: also add the 64 three-symbol occ planes (LF over three bases per gather pair;
                              10.7 bytes per text symbol); requires pair_steps; 2: auto (on while the planes fit
                              32-bit buffer offsets, ~400 M symbols) */
} speq_build_opts;

/* Per-scan parameters (reference: cmd_arguments in include/arg_parse.h:10-28). */
typedef struct {
    uint32_t k;              /* --kmer (reference default 70)                               */
    uint32_t phred_cutoff;   /* --phred-cutoff; a window passes iff min(Q) > cutoff (:162) */
    uint32_t paired;         /* 1: records 2i and 2i+1 are mates; ambiguity per pair (:709-729) */
    uint32_t mode;           /* SPEQ_MODE_GLOBAL (integer U[g]) or SPEQ_MODE_LOCAL (also fp64 W[g]) */
} speq_scan_params;

/* Counter vector layout (u64): [0] = T (passing windows, fm_scanner.cpp:164),
 *                              [1] = ambiguous reads/pairs (:183-190, :213),
 *                              [2 .. 2+G) = U[g] (windows unique to group g, :180).
 * Local mode additionally fills a fp64 vector W[G] (:454-455). */
#define SPEQ_COUNTS_LEN(G) ((size_t)(G) + 2u)

/* ---- library ---- */
const char* speq_last_error(void);
int speq_abi_version(void);
/* Number of visible GPUs (0 when none); never fails. */
int speq_device_count(void);

/* ---- index build / persistence (replaces seqan3::fm_index{…}, fm_indexer.cpp:8-52) ----
 * seq          : concatenated ASCII sequences of the R reference records (FASTA order)
 * rec_offsets  : R+1 offsets into seq
 * group_of_rec : group id of each record (file_to_map's group_scaffolds, file_to_map.cpp:20-119);
 *                n_group_entries may exceed R (extra entries are ignored like the zip at
 *                fm_scanner.cpp:1494) but every record r < R must have 0 <= group < n_groups.
 * The indexed collection is [fwd_0, rc_0, fwd_1, rc_1, …] as built at fm_indexer.cpp:25-33. */
int speq_index_build(const char* seq, const uint64_t* rec_offsets, uint32_t n_records,
                     const int32_t* group_of_rec, uint32_t n_group_entries, uint32_t n_groups,
                     const speq_build_opts* opts, speq_index** out);
/* user_header: opaque bytes stored in front of the index (the CLI stores the reference's
 * {ref path, ref mtime, groups mtime, names, group_scaffolds, counts}, fm_indexer.cpp:39-50). */
int speq_index_save(const speq_index* idx, const char* path, const void* user_header, uint64_t header_len);
/* Loads an index; *user_header (may be NULL) receives a malloc'ed copy of the stored header that the
 * caller frees with speq_free(). */
int speq_index_load(const char* path, speq_index** out, void** user_header, uint64_t* header_len);
/* Reads only the user header of an index file (for the staleness check at fm_indexer.cpp:68-97). */
int speq_index_read_header(const char* path, void** user_header, uint64_t* header_len);
void speq_index_free(speq_index* idx);
void speq_free(void* p);

typedef struct {
    uint64_t n;            /* FM text length (all texts + separators + terminator) */
    uint32_t n_texts;      /* 2R */
    uint32_t n_records;    /* R */
    uint32_t n_groups;     /* G */
    uint32_t prefix_q;
    uint32_t pair_steps;   /* 1 when the two-symbol occ planes are present */
    uint32_t label_table;  /* 1 when the per-position label table is present */
    uint64_t n_runs;       /* runs of equal group label along the suffix array */
    uint64_t device_bytes; /* bytes a device replica occupies in HBM */
    uint32_t triple_steps; /* 1 when the three-symbol occ planes are present */
} speq_index_info;
int speq_index_get_info(const speq_index* idx, speq_index_info* info);

/* Read-only views of the host arrays (for tests and tools; layout documented in DESIGN.md §3).
 * name: "text", "sa", "occ", "occ2", "occ3", "runs", "run_label", "lab", "prefix", "prefix_q1", "prefix_q2", "C",
 *       "text_start", "text_group". */
int speq_index_array(const speq_index* idx, const char* name, const void** ptr, uint64_t* bytes);

/* ---- device replica ---- */
/* Optional, before the index is even loaded (any thread): prepares GPU `device` for this process's first scan — its
 * context, the scan's GPU code (otherwise loaded at the first use of each kernel file, inside the first scan; the
 * GPU index builder's code is left to its first use) and `streams` (0-16) ready streams that speq_device_open and the FASTQ pipelines then take instead of creating
 * them (3-10 ms each). New in the MI355X build: the reference loads a host index (fm_scanner.cpp:45-58). */
int speq_device_warmup(int device, uint32_t streams);
int speq_device_open(const speq_index* idx, int device, speq_device_index** out);
int speq_device_close(speq_device_index* d);

/* ---- the hot path: scan reads already resident in HBM ----
 * Replaces search() + do_a_count() for every window of every read (fm_scanner.cpp:149-214 and the
 * paired/local variants).  Counters are ADDED to d_counts (u64[G+2]) and, in local mode, to d_weights
 * (f64[G]); the caller zeroes them.  d_seq/d_qual: ASCII bases and Phred+33 qualities, d_offsets:
 * n_reads+1 u64 offsets into both.  With params->paired the records are mate pairs (2i, 2i+1) and
 * n_reads must be even.  Asynchronous on `stream`. */
int speq_scan_reads_device(speq_device_index* d, const uint8_t* d_seq, const uint8_t* d_qual,
                           const uint64_t* d_offsets, uint64_t n_reads, const speq_scan_params* params,
                           uint64_t* d_counts, double* d_weights, void* stream);

/* Diagnostic twin of speq_scan_reads_device (not the hot path; bench.py's roofline model): the same scan and
 * results, run by an instrumented instantiation of the anchor-and-extend kernel that also counts the work it did.
 * stats (host, u64[SPEQ_AX_STATS_N], overwritten; synchronous): [0] loop iterations per wave, [1] anchor-bucket loads
 * (64 B each), [2] run iterations (lanes), [3]/[4] iterations in which a wave issued bucket/granule loads, [5] windows
 * classified by runs, [6] deferred windows, [7] deferred windows past the Bloom filter, [8] phase-2 bucket loads,
 * [9] phase-2 candidate verifications (ceil(k / 32) + 1 16-B granules each), [10] staged 16-base chunks (16 B of
 * bases + 16 B of qualities), [11] staged read segments, [12] single quality bytes loaded, [13] windows tallied by
 * runs, [14] 16-B granules loaded by runs, [15] lane refills (per wave), [16..19] phase-1 wave iterations
 * with 1-4, 5-16, 17-32, 33-64 busy lanes, [20..24] shader-clock cycles (s_memtime) summed over waves: in refills
 * (staging), phase-1 lookup iterations, phase-1 run iterations, phase 2 (deferred windows), and the whole loop,
 * [25] deferred-window passes (per wave), [26] cycles of the Bloom-filter part of phase 2, [27] phase-2 probe rounds
 * of the filter's survivors (per wave), [28] / [29] cycles of refills before their staging loads / in their staging
 * batches, [30] the longest wave's loop cycles (a maximum), [31] waves, [32..36] loop cycles summed over the waves of
 * blocks 0-255, 256-511, 512-767, 768-1023 and 1024 on, [37] probes of the substitution bitmap (tuning "ax_sproof"),
 * [38] windows over a mismatch dropped on its proof (not looked up, not deferred), [39] proofs whose continued run met
 * a second mismatch within k - 1 bases (the windows over both deferred), [40] 64-chunk stream instructions the
 * staging batches executed (per wave; [10] / 64 are needed). Fails with SPEQ_E_ARG when the scan does not
 * use that kernel, and, before anything is launched (counts, weights and stats untouched), when the replica has more
 * than 2048 groups: the instrumented kernel exists with the LDS tally only. */
#define SPEQ_AX_STATS_N 41
int speq_scan_reads_device_stats(speq_device_index* d, const uint8_t* d_seq, const uint8_t* d_qual,
                                 const uint64_t* d_offsets, uint64_t n_reads, const speq_scan_params* params,
                                 uint64_t* d_counts, double* d_weights, uint64_t* stats);

/* Host-buffer convenience used by the CLI: stages the reads to HBM in batches, runs the kernel and
 * returns the totals (counts: u64[G+2]; weights: f64[G] or NULL). Synchronous. */
int speq_scan_reads(speq_device_index* d, const uint8_t* seq, const uint8_t* qual, const uint64_t* offsets,
                    uint64_t n_reads, const speq_scan_params* params, uint64_t* counts, double* weights);

/* ---- per-unit report (a diagnostic pass beside the scan) ----
 * A unit is a read, or the pair (2i, 2i+1) when params->paired is set. For every unit: a fixed record and the set of
 * groups that at least one of its windows is unique to, as W = SPEQ_SET_WORDS(G) u64 words (bit g % 64 of word
 * g / 64). A unit is ambiguous iff its set holds two or more bits; the number of such units is counts[1] of a scan of
 * the same reads. Window filter and base conversion are the scan's; params->mode is ignored. Every passing window is
 * searched exactly (no per-k structure), so this is far slower than the scan: an opt-in pass, not the hot path.
 * The reference keeps none of this: its paired "fusion map" (fm_scanner.cpp:915-1033) is keyed by a copy of the set
 * that is always empty (:916). */
#define SPEQ_REPORT_MAX_K 1024
typedef struct {
    uint32_t passing;     /* passing windows of the unit; sum over units == counts[0] of a scan */
    uint32_t unique;      /* windows whose k-mer occurs in texts of exactly one group; sum == sum of U[g] */
    uint32_t shared;      /* passing windows whose k-mer occurs in texts of >= 2 groups;
                             sum == n_windows of the EM histogram */
    uint32_t first_group; /* group of the first unique window (mate 1 before mate 2, ascending start):
                             the reference's which_group, fm_scanner.cpp:183-190; 0xFFFFFFFF when none */
} speq_read_report;       /* 16 bytes */
#define SPEQ_SET_WORDS(G) (((size_t)(G) + 63u) / 64u)
/* Device buffers (d_reports 16-byte aligned), asynchronous on stream; overwrites n_units records and n_units * W set
 * words, nothing else. 1 <= k <= SPEQ_REPORT_MAX_K; reads of any length; n_reads == 0 launches nothing. */
int speq_report_reads_device(speq_device_index* d, const uint8_t* d_seq, const uint8_t* d_qual,
                             const uint64_t* d_offsets, uint64_t n_reads, const speq_scan_params* params,
                             speq_read_report* d_reports, uint64_t* d_sets, void* stream);
/* Host buffers, synchronous, staged in batches like speq_scan_reads. */
int speq_report_reads(speq_device_index* d, const uint8_t* seq, const uint8_t* qual, const uint64_t* offsets,
                      uint64_t n_reads, const speq_scan_params* params, speq_read_report* reports, uint64_t* sets);
/* ---- marker coverage (a diagnostic pass beside the scan) ----
 * A marker of group g, at scan length k: a distinct N-free k-mer of the indexed texts (fwd and rc of every record)
 * whose occurrences all lie in texts of g; a k-mer and its reverse complement are two markers. Its depth is the number
 * of passing read windows equal to it (window filter and base conversion are the scan's; params->paired and
 * params->mode are ignored). Per group: the markers, those of depth >= 1 (observed), the sum of depths (hits, equal to
 * U[g] of a scan of the same reads), the largest depth, and depth_hist[j] = markers of depth exactly j for j < 7 and of
 * depth >= 7 for j = 7. observed / markers is the breadth of coverage; a group that is really present shows a breadth
 * near 1 - exp(-hits / markers), while copies of a few k-mers (an amplicon, duplicates, a contaminating fragment)
 * give the same hits at a breadth near 0. Every passing window is searched exactly (no per-k structure), as in the
 * per-unit report: an opt-in pass, not the hot path. The handle holds 4 bytes per SA position on the replica's GPU;
 * the replica must outlive it. A marker's depth must stay below 2^31. The reference keeps none of this.
 *
 * The marker track says where along each record the covered markers lie. A locus (r, p) is a window
 * start p of fwd_r (text 2r), 0 <= p < nwin_r = max(L_r - k + 1, 0); it is a marker locus when its k-mer x is a marker
 * (then of the record's own group). Its depth folds the strands: depth(x) + depth(rc(x)), or depth(x) alone when x is
 * its own reverse complement (one k-mer, one marker, counted once). The depth belongs to the k-mer: a marker that lies
 * at several loci (a repeat inside a record, identical records of one group) gives each of them its full depth, so the
 * track's hits summed over a group are >= the group's hits above, and equal when every marker has one locus. Record r
 * has ceil(nwin_r / bin) bins, bin b covering the loci [b * bin, min((b + 1) * bin, nwin_r)); a record shorter than k
 * has none. Per bin: its marker loci, those of depth >= 1 (observed), the sum of their depths (hits) and the largest. */
#define SPEQ_MARKER_BINS 8
typedef struct {
    uint64_t markers, observed, hits, max_depth, depth_hist[SPEQ_MARKER_BINS];
} speq_marker_cov; /* 96 bytes */
typedef struct speq_markers speq_markers;
/* Fixes params->k (1 .. SPEQ_REPORT_MAX_K) and params->phred_cutoff, and marks the markers (one pass over the texts on
 * the replica's GPU; blocking). SPEQ_E_NOMEM when the depth array does not fit the free HBM. */
int speq_markers_create(speq_device_index* d, const speq_scan_params* params, speq_markers** out);
/* Adds the reads' windows to the depths. Device buffers, asynchronous on stream; writes nothing but the handle's array.
 * Reads of any length; n_reads == 0 launches nothing. */
int speq_markers_add_reads_device(speq_markers* m, const uint8_t* d_seq, const uint8_t* d_qual,
                                  const uint64_t* d_offsets, uint64_t n_reads, void* stream);
/* Host buffers, synchronous, staged in batches like speq_report_reads; nothing is copied back. */
int speq_markers_add_reads(speq_markers* m, const uint8_t* seq, const uint8_t* qual, const uint64_t* offsets,
                           uint64_t n_reads);
/* Waits for the adds of every stream of the device and folds the depths into out[G] (host, overwritten). The handle
 * stays usable: more adds and another finalize give the totals of everything added so far. */
int speq_markers_finalize(speq_markers* m, speq_marker_cov* out);
/* Test accessor: every marker (depth 0 included) by ascending SA position. *n_markers (may be NULL) receives their
 * number; lo / group / depth (any may be NULL) hold that many entries each: call once with null arrays for the size. */
int speq_markers_list(speq_markers* m, uint64_t* n_markers, uint32_t* lo, uint32_t* group, uint32_t* depth);
void speq_markers_free(speq_markers* m);
typedef struct {
    uint64_t markers, observed, hits, max_depth;
} speq_marker_bin; /* 32 bytes */
#define SPEQ_TRACK_MAX_BIN (1u << 20)
/* Host only: the bins per record as a prefix, first_bin[R + 1] for the index's R records (may be NULL for the size
 * alone); *n_bins (may be NULL) = first_bin[R]. 1 <= bin <= SPEQ_TRACK_MAX_BIN. The second form needs no replica:
 * the same layout from an index and a scan length (1 .. SPEQ_REPORT_MAX_K). */
int speq_markers_track_layout(const speq_markers* m, uint32_t bin, uint64_t* n_bins, uint64_t* first_bin);
int speq_index_track_layout(const speq_index* idx, uint32_t k, uint32_t bin, uint64_t* n_bins, uint64_t* first_bin);
/* Waits for the adds of every stream of the device (as speq_markers_finalize does), runs one pass over the forward
 * texts and overwrites out[n_bins] (host), record after record as the layout says. Reads the handle's depths and
 * changes nothing of it: the handle stays usable, more adds and another track give the totals so far, and
 * speq_markers_finalize returns the same records before and after. SPEQ_E_NOMEM when the bins do not fit the free HBM. */
int speq_markers_track(speq_markers* m, uint32_t bin, speq_marker_bin* out);

/* ---- read bootstrap: how far to trust a percentage (a diagnostic pass beside the scan) ----
 * The scan's counter vector under B Poisson(1) resamplings of the reads, in one pass. The resampling unit is the read,
 * or the pair (2i, 2i + 1) when params->paired is set: windows of one read are strongly correlated. Unit u, replicate
 * b = 1 .. B has the integer weight
 *   w = #{j in 0 .. 20 : h >= C_j},  h = mix(x + g b),  x = mix(seed + g (u + 1)),  g = 0x9e3779b97f4a7c15,
 *   mix = splitmix64's finaliser,  C_j = floor(2^64 e^-1 sum_{i <= j} 1 / i!)   (all mod 2^64; w <= 21),
 * and replicate 0 is the sample itself (every weight 1). u is the unit's position in the input, always passed
 * explicitly (first_unit + its position in the call): no handle keeps a running count, so the result depends on no
 * batch cut, block order, thread count or grid size. Per unit: P passing windows, c[g] windows unique to group g, amb =
 * 1 iff two or more c[g] are non-zero. counts is u64 [B + 1][G + 2], row b a counter vector in SPEQ_COUNTS_LEN layout:
 * [b][0] = sum_u w P_u, [b][1] = sum_u w amb_u, [b][2 + g] = sum_u w c_u[g]; row 0 equals a scan of the same reads.
 * With params->mode == SPEQ_MODE_LOCAL there is also weights, f64 [B + 1][G]: [b][g] = sum_u w (sum of the scan's Phred
 * weight over u's windows unique to g). Window filter and base conversion are the scan's. Every passing window is
 * searched exactly (no per-k structure), as in the per-unit report: an opt-in pass, not the hot path. The replica must
 * outlive the handle. The reference keeps none of this. */
#define SPEQ_BOOTSTRAP_MAX_REPLICATES 1024
typedef struct speq_bootstrap speq_bootstrap;
/* Fixes params (k in 1 .. SPEQ_REPORT_MAX_K, phred_cutoff, paired, mode), 1 .. SPEQ_BOOTSTRAP_MAX_REPLICATES replicates
 * and the seed; the accumulators live on the replica's GPU (blocking). */
int speq_bootstrap_create(speq_device_index* d, const speq_scan_params* params, uint32_t replicates, uint64_t seed,
                          speq_bootstrap** out);
/* Adds n_reads records (an even number for a paired handle) whose first unit has index first_unit. Device buffers,
 * asynchronous on stream; writes nothing but the handle's accumulators. n_reads == 0 launches nothing. */
int speq_bootstrap_add_reads_device(speq_bootstrap* b, const uint8_t* d_seq, const uint8_t* d_qual,
                                    const uint64_t* d_offsets, uint64_t n_reads, uint64_t first_unit, void* stream);
/* Host buffers, synchronous, staged in batches like speq_report_reads; first_unit counts units, not records. */
int speq_bootstrap_add_reads(speq_bootstrap* b, const uint8_t* seq, const uint8_t* qual, const uint64_t* offsets,
                             uint64_t n_reads, uint64_t first_unit);
/* Waits for the adds of every stream of the device; counts[(B + 1)(G + 2)] and, for a local handle, weights[(B + 1) G]
 * (NULL otherwise) are overwritten with the totals so far. The handle stays usable, like speq_markers_finalize. */
int speq_bootstrap_finalize(speq_bootstrap* b, uint64_t* counts, double* weights);
/* Any output may be NULL. *lds_path: 1 when the last add accumulated per block in LDS, 0 when it used device atomics
 * throughout (the accumulators did not fit); *units_added: units of every add so far. */
int speq_bootstrap_info(const speq_bootstrap* b, uint32_t* replicates, uint32_t* lds_path, uint64_t* units_added);
void speq_bootstrap_free(speq_bootstrap* b);
/* Host test accessor: the weight of (seed, unit, replicate) as the kernel computes it. */
uint32_t speq_bootstrap_weight(uint64_t seed, uint64_t unit, uint32_t replicate);
/* Host only: per group, the percentage of the sample and its spread over the replicates. Row b's percentage of group
 * g is unique_to_percent of that row: 100 ur / counts[b][0] / (u_ref[g] / tot_ref[g]) with ur = weights[b][g] when
 * weights is given, else counts[b][2 + g] * unique_scale (the CLI passes 1 / fixed_accuracy^k); 0 where tot_ref[g] ==
 * 0. estimate is row 0's. Replicates with counts[b][0] == 0 are left out; `used` counts the rest, n. Over their values
 * v in replicate order: mean = sum v / n, se = sqrt(sum (v - mean)^2 / (n - 1)) (0 when n < 2), plain sequential f64
 * sums; sorted ascending with t = floor(n (1 - level) / 2): lo = v[t], hi = v[n - 1 - t]. 0 < level < 1. n = 0:
 * everything but estimate is 0. */
typedef struct { double estimate, mean, se, lo, hi; uint64_t used; } speq_bootstrap_ci; /* 48 bytes */
int speq_bootstrap_summary(const uint64_t* counts, const double* weights, uint32_t replicates, uint32_t n_groups,
                           const uint64_t* u_ref, const uint64_t* tot_ref, double unique_scale, double level,
                           speq_bootstrap_ci* out /* [G] */);
/* The same statistics over a given percentage matrix, f64 [B + 1][G] (the EM-refined percentages of
 * speq_em_rows_refine): row b = 1 .. B is a replicate, left out where used_mask[b] == 0 (u8 [B + 1]; [0] is not read);
 * estimate is the vector `estimate`, or row 0 when it is NULL. */
int speq_bootstrap_summary_percent(const double* percent, const double* estimate, const uint8_t* used_mask,
                                   uint32_t replicates, uint32_t n_groups, double level,
                                   speq_bootstrap_ci* out /* [G] */);
/* One EM histogram per replicate, filled by the adds in the same pass. `em` must be finalized, of the
 * same replica and group count as b, and b must have had no reads added and no histogram attached; otherwise
 * SPEQ_E_ARG. Uploads em's interval -> row map and allocates the u64 [n_rows][B + 1] matrix (SPEQ_E_NOMEM when it does
 * not fit); blocking. em itself is not kept: it may be freed afterwards. From then on every add also adds, per unit u
 * and replicate b, w(u, b) * (u's multi-group windows whose interval em holds, per merged row); a multi-group window
 * whose interval em does not hold is counted in `missed`. The counts and weights of b are what they are without. */
struct speq_em;
int speq_bootstrap_attach_em(speq_bootstrap* b, const struct speq_em* em);
/* *n_rows: em's merged rows; *lds_rows: H, how many of them (the most frequent in the sample) a block accumulates in
 * LDS: min(n_rows, floor((64 KiB - 4 wave_bytes(k) - the counters' cells when they take the LDS path) / (8 (B + 1)))).
 * SPEQ_E_ARG without an attached histogram. */
int speq_bootstrap_em_info(const speq_bootstrap* b, uint64_t* n_rows, uint32_t* lds_rows);
/* Like speq_bootstrap_finalize (waits; repeatable): mult is u64 [B + 1][n_rows], row b the multiplicities of replicate
 * b in the order of speq_em_rows, so mult[0] equals em's row_mult when the reads are those of em's scan and *missed
 * (may be NULL) is 0. */
int speq_bootstrap_finalize_em(speq_bootstrap* b, uint64_t* mult, uint64_t* missed);

/* ---- duplicate reads: every distinct read (pair) counted once (a pass beside the scan) ----
 * A unit is a record, or the pair of records (2i, 2i + 1) of a paired handle. Its fingerprint is (F_0, F_1),
 *   F_s = sum over mates m in {0, 1} and positions i of that mate of mix(S_s + g (1 + c + 5 i + (m << 40)))  (mod 2^64),
 *   c = the scan's dna5 code of the base (A C G T/U in either case 0..3, every other byte 4; qualities do not enter),
 *   mix = splitmix64's finaliser, g = 0x9e3779b97f4a7c15, S_0 = 0x243f6a8885a308d3, S_1 = 0x13198a2e03707344;
 * an empty unit has (0, 0); a record must be shorter than 2^32. Two units are duplicates iff their fingerprints are
 * equal: that is the definition. Two distinct sequences collide with probability about 2^-128 per pair. Position and
 * mate are inside the term, so a prefix, a shifted read and swapped mates differ. rep[u] is the lowest unit index of
 * u's fingerprint, and u is kept iff rep[u] == u, whatever the batch cuts, streams or thread counts. The records of the
 * other units get '!' (Phred 0) over their qualities: a window passes only if every quality is above the unsigned
 * cutoff, so a scan of the masked reads equals, counter for counter, a scan of the reads with those units removed.
 * The handle holds 20 bytes per unit on the replica's GPU (24 after a finalize), in chunks of 65,536 units allocated
 * as the adds reach them; the replica must outlive it. Unit indices stay below 2^32 - 1. The reference keeps none of
 * this. */
#define SPEQ_DEDUP_BINS 8
typedef struct {
    uint64_t units;            /* N */
    uint64_t distinct;         /* classes of equal fingerprint */
    uint64_t max_multiplicity; /* units of the largest class */
    uint64_t reserved;         /* 0 */
    uint64_t mult_hist[SPEQ_DEDUP_BINS]; /* [j]: classes of exactly j + 1 units, j < 7; [7]: of 8 or more; sum = distinct */
} speq_dedup_stats; /* 96 bytes */
typedef struct speq_dedup speq_dedup;
struct speq_em;
int speq_dedup_create(speq_device_index* d, uint32_t paired, speq_dedup** out);
/* Fingerprints n_reads records (an even number for a paired handle) whose first unit has index first_unit. Device
 * buffers, asynchronous on stream; writes nothing but the handle's storage. Adds may come in any order, in any number of
 * calls and on several streams. SPEQ_E_ARG when a unit index would reach 2^32 - 1, SPEQ_E_NOMEM when a chunk does not
 * fit. n_reads == 0 launches nothing. */
int speq_dedup_add_reads_device(speq_dedup* h, const uint8_t* d_seq, const uint64_t* d_offsets, uint64_t n_reads,
                                uint64_t first_unit, void* stream);
/* Host buffers, synchronous, staged in batches like speq_report_reads; first_unit counts units, not records. */
int speq_dedup_add_reads(speq_dedup* h, const uint8_t* seq, const uint64_t* offsets, uint64_t n_reads,
                         uint64_t first_unit);
/* Waits for the device. The units added so far must be exactly 0 .. N - 1, each once: otherwise SPEQ_E_ARG, and the
 * handle stays usable (add what is missing and finalize again). Sorts the fingerprints, marks the representatives and
 * fills *out. More adds and another finalize cover everything added so far, like speq_markers_finalize. */
int speq_dedup_finalize(speq_dedup* h, speq_dedup_stats* out);
/* The three below need a finalize with no add after it and a unit range inside 0 .. N - 1; otherwise SPEQ_E_ARG. */
/* Test accessor: rep[first_unit .. first_unit + n_units) to the host. */
int speq_dedup_representatives(speq_dedup* h, uint64_t first_unit, uint64_t n_units, uint32_t* rep);
/* Writes '!' over the quality bytes of every record of a unit that is not kept, and nothing else; d_offsets holds
 * n_reads + 1 offsets, record r belongs to unit first_unit + r / (records per unit). Asynchronous on stream. */
int speq_dedup_mask_device(speq_dedup* h, uint8_t* d_qual, const uint64_t* d_offsets, uint64_t n_reads,
                           uint64_t first_unit, void* stream);
/* The scan of host reads with the duplicates masked: staged in batches like speq_report_reads, the mask goes over the
 * staged qualities (seq, qual and offsets are only read), then speq_em_scan_reads_device when em is given (a histogram
 * of the handle's replica, not finalized) and speq_scan_reads_device otherwise. The batches' counters are ADDED to
 * counts (u64 [G + 2]) and, in local mode, to weights (f64 [G]; NULL otherwise): the caller zeroes them. SPEQ_E_ARG
 * also when params->paired differs from the handle's. Synchronous. */
int speq_dedup_scan_reads(speq_dedup* h, struct speq_em* em, const uint8_t* seq, const uint8_t* qual,
                          const uint64_t* offsets, uint64_t n_reads, uint64_t first_unit,
                          const speq_scan_params* params, uint64_t* counts, double* weights);
void speq_dedup_free(speq_dedup* h);
/* Host only: the fingerprint of the unit (seq1, seq2) as the kernel computes it; seq2 NULL or len2 0 for a single-end
 * unit (an empty mate 2 adds nothing). */
void speq_dedup_fingerprint(const uint8_t* seq1, uint64_t len1, const uint8_t* seq2, uint64_t len2, uint64_t out[2]);

/* ---- reference-uniqueness pass (replaces _async_count_unique_kmers_per_group, fm_scanner.cpp:1476-1576)
 * For every window of every text (fwd and rc of each record): Tot_ref[g] += 1, and U_ref[g] += 1 iff
 * every occurrence lies in a text of group g.  Outputs are host arrays of G u64 (overwritten). */
int speq_ref_unique(speq_device_index* d, uint32_t k, uint64_t* u_ref, uint64_t* tot_ref);
/* Same on device buffers (added to d_u_ref/d_tot_ref), asynchronous. */
int speq_ref_unique_device(speq_device_index* d, uint32_t k, uint64_t* d_u_ref, uint64_t* d_tot_ref,
                           void* stream);

/* ---- multi-GPU: one all-reduce of the counter vector (replaces the future.get() sums, fm_scanner.cpp:224-233).
 * A communicator (void* comm) runs over one of two transports: RCCL (ncclAllReduce over xGMI; one rank per GPU) or
 * host sockets (loopback TCP: a reduce at rank 0 in rank order and a broadcast; ranks may share a GPU). Every
 * speq_allreduce_* / speq_em_allreduce call below takes either. ---- */
enum { SPEQ_COMM_AUTO = 0, SPEQ_COMM_RCCL = 1, SPEQ_COMM_HOST = 2 };
/* RCCL communicator from an id that rank 0 made with speq_comm_unique_id and handed to the others out of band
 * (bench.py: torch.distributed); binds to the calling thread's current GPU. */
int speq_comm_unique_id(void* id_out /* 128 bytes */);
int speq_comm_init(int nranks, int rank, const void* id /* 128 bytes */, void** comm_out);
/* Rendezvous + communicator in one call (the CLI's one-process-per-GPU mode). Rank 0 listens on 127.0.0.1 and
 * publishes {nonce, port} in the file rendezvous_path (replacing a stale one); the other ranks poll that file, connect
 * and present the nonce (a stale file of a dead run is skipped: its port refuses or its nonce does not match), all
 * within timeout_s. transport: SPEQ_COMM_RCCL, SPEQ_COMM_HOST, or SPEQ_COMM_AUTO = RCCL when every rank's `device`
 * is a different GPU (PCI bus id), else host sockets (RCCL refuses two ranks on one GPU). The RCCL communicator is
 * created on GPU `device` (set and restored around ncclCommInitRank); device may be -1 with SPEQ_COMM_HOST. */
int speq_comm_connect(int nranks, int rank, int device, const char* rendezvous_path, int transport, int timeout_s,
                      void** comm_out);
/* SPEQ_COMM_RCCL or SPEQ_COMM_HOST (the transport a communicator runs on); SPEQ_E_ARG for NULL. */
int speq_comm_transport(void* comm);
int speq_comm_destroy(void* comm);
int speq_allreduce_u64(void* comm, uint64_t* d_buf, uint64_t count, void* stream);
int speq_allreduce_f64(void* comm, double* d_buf, uint64_t count, void* stream);

/* ---- EM refinement (reference: fm_scanner.cpp:1069-1453 and the loops at :248-279) ----
 * The reference re-reads and re-searches all reads in every EM iteration. Here ONE scan records, for every passing
 * window whose occurrences span >= 2 groups, its SA interval (a window's EM weight depends only on the per-group
 * occurrence counts of its k-mer; the per-window factor temp_acc/qavg cancels), and every iteration is a sweep
 * over that histogram:
 *   speq_em_create -> speq_em_scan_reads[_device] (any number of batches; also returns the normal counters)
 *   -> speq_em_finalize -> speq_em_step per iteration.
 * The speq_index and the device replica must outlive the histogram. */
typedef struct speq_em speq_em;
int speq_em_create(const speq_index* idx, speq_device_index* d, speq_em** out);
int speq_em_scan_reads(speq_em* em, const uint8_t* seq, const uint8_t* qual, const uint64_t* offsets,
                       uint64_t n_reads, const speq_scan_params* params, uint64_t* counts, double* weights);
int speq_em_scan_reads_device(speq_em* em, const uint8_t* d_seq, const uint8_t* d_qual, const uint64_t* d_offsets,
                              uint64_t n_reads, const speq_scan_params* params, uint64_t* d_counts,
                              double* d_weights, void* stream);
/* Downloads the histogram and builds one row per distinct interval {multiplicity, (group, count)...}; rows of equal
 * content are then merged (multiplicities summed). `threads` is kept for the ABI: the rows are built on the
 * library's worker pool (at most 16 threads), as the EM steps are. */
int speq_em_finalize(speq_em* em, uint32_t threads);
/* Distinct intervals recorded, their (group, count) entries, and the windows (sum of multiplicities); before merging. */
int speq_em_info(const speq_em* em, uint64_t* n_intervals, uint64_t* n_entries, uint64_t* n_windows);
/* Test accessor: the finalized rows as CSR (after merging, so n_rows <= n_intervals and n_entries here counts the
 * merged rows' entries). Call with null arrays for the sizes, then with row_mult[n_rows], row_ptr[n_rows + 1],
 * col_group[n_entries], col_count[n_entries] (any may be null) for a copy: row r has multiplicity row_mult[r] and the
 * entries row_ptr[r] .. row_ptr[r + 1], groups ascending. Fails with SPEQ_E_ARG before speq_em_finalize. */
int speq_em_rows(const speq_em* em, uint64_t* n_rows, uint64_t* n_entries, uint64_t* row_mult, uint64_t* row_ptr,
                 uint32_t* col_group, uint32_t* col_count);
/* next[g] = sum over passing windows with hits of (c_g p_g / n_g) / sum_j (c_j p_j / n_j) (windows with a
 * non-positive sum skipped), given percent[G], group_counts[G] (the "(count)" of each groupings line) and
 * unique[G] (the U[g] counters of the same scan, i.e. its single-group windows). */
int speq_em_step(const speq_em* em, const double* percent, const int32_t* group_counts, const uint64_t* unique,
                 double* next);
/* Test accessor, call-twice like speq_em_rows: *n recorded intervals (speq_em_info's n_intervals), lo[n] their SA
 * interval starts ascending, row[n] the index in speq_em_rows' order of the merged row each went into. Fails with
 * SPEQ_E_ARG before speq_em_finalize. */
int speq_em_intervals(const speq_em* em, uint64_t* n, uint32_t* lo, uint32_t* row);
/* speq_em_step without a handle or a GPU, over rows as speq_em_rows returns them (row_ptr[n_rows + 1] ascending from
 * 0, groups below n_groups) with the multiplicities mult[n_rows] in row_mult's place: the same sweep, so with
 * mult = row_mult the same bits. */
int speq_em_rows_step(uint32_t n_groups, uint64_t n_rows, const uint64_t* row_ptr, const uint32_t* col_group,
                      const uint32_t* col_count, const uint64_t* mult, const double* percent,
                      const int32_t* group_counts, const uint64_t* unique, double* next);
/* The refinement loop of `speq scan` for every row b of a bootstrap's matrices (mult u64 [B + 1][n_rows] of
 * speq_bootstrap_finalize_em, counts u64 [B + 1][G + 2], weights f64 [B + 1][G] or NULL): unique_totals = weights[b],
 * or counts[b][2 ..] * unique_scale; total = counts[b][0]; percent = unique_to_percent(unique_totals, total, u_ref,
 * tot_ref); then, while the largest |change| of a step is above precision and fewer than max_iterations steps were
 * made: next = the step over mult[b] with unique = counts[b][2 ..], percent = unique_to_percent(unique_totals, total,
 * unique_totals, next). percent_out is f64 [B + 1][G], iterations_out u32 [B + 1] the steps made. A row with
 * counts[b][0] == 0 gets zeros and 0 steps. The rows are refined side by side on the library's worker pool (at most
 * 16 threads), each one's sweep adding its chunks in chunk order: the result does not depend on the thread count. */
int speq_em_rows_refine(uint32_t n_groups, uint64_t n_rows, const uint64_t* row_ptr, const uint32_t* col_group,
                        const uint32_t* col_count, uint32_t replicates, const uint64_t* mult, const uint64_t* counts,
                        const double* weights, double unique_scale, const uint64_t* u_ref, const uint64_t* tot_ref,
                        const int32_t* group_counts, double precision, uint32_t max_iterations, double* percent_out,
                        uint32_t* iterations_out);
void speq_em_free(speq_em* em);

/* ---- streaming scan: pinned host slots, H2D on a copy stream overlapped with the kernel ----
 * Replaces the reference's single-producer async_input_buffer feeding T-1 search workers
 * (fm_scanner.cpp:138-141, :219-222; paired :651-655). A pipeline owns n_slots pinned host buffers, each with a
 * device twin; a producer thread acquires a free slot, writes whole records into it (ASCII bases, Phred+33
 * qualities, offsets[0] = 0 .. offsets[n]), and submits it: the slot is copied to HBM on a copy stream while the
 * kernel of the previous slot runs on a compute stream. Any number of producer threads may acquire/submit
 * concurrently. Counters accumulate on the device; finish returns them (and resets them to zero).
 * em may be NULL; when given, the scan also records its EM histogram (the pipeline must use em's device). */
typedef struct speq_pipeline speq_pipeline;
typedef struct {
    uint8_t* seq;          /* capacity cap_bytes */
    uint8_t* qual;         /* capacity cap_bytes */
    uint64_t* offsets;     /* capacity cap_records + 1 */
    uint64_t cap_bytes;
    uint64_t cap_records;
    int32_t slot;          /* pass back to speq_pipeline_submit */
} speq_slot;
int speq_pipeline_create(speq_device_index* d, const speq_scan_params* params, speq_em* em, uint64_t slot_bytes,
                         uint64_t slot_records, uint32_t n_slots, speq_pipeline** out);
/* Blocks until a slot is free (its previous copy and kernel have completed). */
int speq_pipeline_acquire(speq_pipeline* pl, speq_slot* out);
/* Grows a slot's capacity (host and device) before it is filled; contents are not preserved. */
int speq_pipeline_reserve(speq_pipeline* pl, speq_slot* slot, uint64_t bytes, uint64_t records);
/* Enqueues the copy + scan of n_records records of an acquired slot (n_records may be 0: releases the slot). */
int speq_pipeline_submit(speq_pipeline* pl, int32_t slot, uint64_t n_records);
/* Waits for every submitted slot; counts u64[G+2] (and weights f64[G] in local mode) receive the totals since
 * the last finish. */
int speq_pipeline_finish(speq_pipeline* pl, uint64_t* counts, double* weights);
void speq_pipeline_free(speq_pipeline* pl);

/* Scan of FASTQ files (plain or gzip; paired when path2 != NULL: records i of both files are mates) through a
 * pipeline: one reader thread per file decompresses and cuts record-aligned blocks, `threads` parser threads fill
 * pinned slots. FASTQ grammar of the reference's reader (multi-line sequence/quality accepted; a FASTA file is
 * rejected: qualities are required). counts/weights as speq_scan_reads; stats may be NULL. */
typedef struct {
    uint64_t records;      /* records scanned (both mates) */
    uint64_t bases;
    uint64_t batches;      /* slots submitted */
    double seconds;        /* wall time of the call */
} speq_stream_stats;
int speq_scan_fastq(speq_device_index* d, const char* path1, const char* path2, const speq_scan_params* params,
                    speq_em* em, uint32_t threads, uint64_t* counts, double* weights, speq_stream_stats* stats);
/* Optional, ahead of speq_scan_fastq on GPU `device` with `threads` parsers (e.g. while the index loads): allocates
 * the stream's pinned and device slot buffers now (otherwise the parser threads' first slots allocate them: up to
 * 66 ms of page-locking at the start of a `speq scan` run); the next stream's slots of that device take them. */
int speq_stream_reserve(int device, uint32_t threads, uint32_t paired);
/* The same reader and parsers without a device (host only; for tests and tools): record and base counts, and an
 * order-independent digest = sum over records of mix64(FNV-1a-64 over (len, (base << 8 | qual) per position)). */
int speq_fastq_checksum(const char* path1, const char* path2, uint32_t threads, uint64_t* records, uint64_t* bases,
                        uint64_t* digest);

/* The per-unit report (speq_report_reads) of FASTQ file(s) as an order-independent summary: one entry per distinct
 * group set with the number of units that have it, sorted ascending by the set read as one integer (word W-1 most
 * significant), so the empty set comes first. Entries with two or more bits are the real fusion map. The blocks are
 * parsed on host threads and reported in any order; stats may be NULL. */
typedef struct speq_group_sets speq_group_sets;
int speq_report_fastq(speq_device_index* d, const char* path1, const char* path2, const speq_scan_params* params,
                      uint32_t threads, speq_group_sets** out, speq_stream_stats* stats);
uint64_t speq_group_sets_count(const speq_group_sets* s);  /* distinct sets, the empty set included */
int speq_group_sets_get(const speq_group_sets* s, uint64_t i, uint64_t* words /* W */, uint64_t* units);
/* Sums over all units (any output may be NULL). */
int speq_group_sets_totals(const speq_group_sets* s, uint64_t* units, uint64_t* passing, uint64_t* unique,
                           uint64_t* shared);
void speq_group_sets_free(speq_group_sets* s);

/* Marker coverage (speq_markers_*) of the whole of FASTQ file(s) (plain or gzip; both files' records when path2 != NULL) through a handle of its own:
 * blocks parsed on host threads and added in any order, one finalize at the end into out[G]. stats may be NULL. */
int speq_markers_fastq(speq_device_index* d, const char* path1, const char* path2, const speq_scan_params* params,
                       uint32_t threads, speq_marker_cov* out, speq_stream_stats* stats);
/* The same single pass over the file(s), and both answers from its handle: cov[G] as speq_markers_fastq gives (cov may
 * be NULL), and the marker track at width `bin` (speq_markers_track): first_bin[R + 1] (the caller's, R = the index's
 * records) and *out, *n_bins records allocated here and freed with speq_free (NULL when there is no bin). */
int speq_markers_track_fastq(speq_device_index* d, const char* path1, const char* path2, const speq_scan_params* params,
                             uint32_t threads, uint32_t bin, speq_marker_cov* cov, uint64_t* first_bin,
                             speq_marker_bin** out, uint64_t* n_bins, speq_stream_stats* stats);

/* The read bootstrap (speq_bootstrap_*) of the whole of FASTQ file(s) (plain or gzip; paired when path2 != NULL)
 * through a handle of its own: blocks parsed on host threads and added in any order, each with the index of its first
 * record in the file, so the result equals speq_bootstrap_add_reads of the same records with first_unit = 0 for any
 * `threads`. weights is NULL unless params->mode is local; stats may be NULL. */
int speq_bootstrap_fastq(speq_device_index* d, const char* path1, const char* path2, const speq_scan_params* params,
                         uint32_t replicates, uint64_t seed, uint32_t threads, uint64_t* counts, double* weights,
                         speq_stream_stats* stats);
/* The same with the finalized histogram em attached (speq_bootstrap_attach_em): also mult u64 [B + 1][n_rows] and
 * *missed (may be NULL) of speq_bootstrap_finalize_em; independent of `threads` as well. */
int speq_bootstrap_em_fastq(speq_device_index* d, const speq_em* em, const char* path1, const char* path2,
                            const speq_scan_params* params, uint32_t replicates, uint64_t seed, uint32_t threads,
                            uint64_t* counts, double* weights, uint64_t* mult, uint64_t* missed,
                            speq_stream_stats* stats);

/* The deduplicated scan (speq_dedup_*) of the whole of FASTQ file(s) (plain or gzip; paired when path2 != NULL) through
 * a handle of its own, in two passes of the sequential reader with host-parsed blocks, each block carrying the index of
 * its first record: pass 1 adds every block, one finalize fills *stats (may be NULL), pass 2 runs speq_dedup_scan_reads
 * on every block. counts (u64 [G + 2]) and, in local mode, weights (f64 [G]; NULL otherwise) are overwritten with the
 * totals; with em (may be NULL; not finalized) the scan also fills that histogram. The statistics and the counts do not
 * depend on `threads`. st (may be NULL) describes pass 2. */
int speq_dedup_fastq(speq_device_index* d, struct speq_em* em, const char* path1, const char* path2,
                     const speq_scan_params* params, uint32_t threads, speq_dedup_stats* stats, uint64_t* counts,
                     double* weights, speq_stream_stats* st);

/* ---- several GPUs in one process ----
 * Reads shard across the GPUs of a node, the index is replicated (one speq_device_index per GPU, opened from the
 * same speq_index), and the only exchange is a sum of the counters. The reference sums its per-thread vectors after
 * future.get() (fm_scanner.cpp:224-233, :1544-1557); here one host thread owns every replica, so the G + 2 counter
 * words of each replica are added on the host, and the EM histograms (n words per replica) are added on the first
 * replica's GPU (peer copy over xGMI + an add kernel). For one process per GPU use speq_allreduce_* (RCCL).
 * Replicas may share a GPU (logical shards; results are the same). */
/* speq_scan_fastq over n_devices replicas: record-aligned blocks are dealt to the replicas in turn. ems is NULL or
 * holds one histogram per replica (ems[i] created on ds[i]); fold them with speq_em_merge before speq_em_finalize. */
int speq_scan_fastq_multi(speq_device_index* const* ds, speq_em* const* ems, uint32_t n_devices, const char* path1,
                          const char* path2, const speq_scan_params* params, uint32_t threads, uint64_t* counts,
                          double* weights, speq_stream_stats* stats);
/* speq_ref_unique with replica i scanning the i-th equal slice of the reference windows (the .dat pass sharded the
 * same way as the reads; fm_scanner.cpp:1476-1560). */
int speq_ref_unique_multi(speq_device_index* const* ds, uint32_t n_devices, uint32_t k, uint64_t* u_ref,
                          uint64_t* tot_ref);
/* dst += src for two unfinalized EM histograms of replicas of one index (any GPUs of this process). src's device
 * arrays are released: afterwards src accepts only speq_em_free. */
int speq_em_merge(speq_em* dst, speq_em* src);

/* ---- one process per GPU (RANK / WORLD_SIZE of a launcher such as torchrun; `speq scan` runs this way when
 * WORLD_SIZE > 1). Every rank opens its own replica, scans ITS share of the input, and the exchange is RCCL:
 * speq_allreduce_u64/_f64 of the counters, speq_em_allreduce of the EM histogram. This replaces the reference's
 * future.get() sums (fm_scanner.cpp:224-233) across processes instead of threads. ---- */
/* speq_scan_fastq over shard `shard` of `n_shards`: the input is cut into record-aligned blocks exactly as on every
 * other rank and this rank scans the blocks b with b % n_shards == shard (counts, weights, em and stats cover those
 * only). cut: -1 = parallel cut, falling back to the sequential cutter on this rank alone (n_shards = 1 only);
 * 1 = parallel cut only, failing with SPEQ_E_RETRY (counters, weights, em cleared) when the file does not fit it —
 * the ranks then agree (an all-reduce of the flag) and all scan again with cut = 0 (sequential cutter). */
int speq_scan_fastq_shard(speq_device_index* d, speq_em* em, const char* path1, const char* path2,
                          const speq_scan_params* params, uint32_t threads, uint32_t shard, uint32_t n_shards, int cut,
                          uint64_t* counts, double* weights, speq_stream_stats* stats);
/* speq_fastq_checksum over one shard (same blocks as speq_scan_fastq_shard; cut 0 or 1, SPEQ_E_RETRY as there). */
int speq_fastq_checksum_shard(const char* path1, const char* path2, uint32_t threads, uint32_t shard,
                              uint32_t n_shards, int cut, uint64_t* records, uint64_t* bases, uint64_t* digest);
/* The .dat pass over shard `shard` of `n_shards` equal slices of the reference windows (host outputs, this
 * shard's partial sums; fm_scanner.cpp:1476-1560). */
int speq_ref_unique_shard(speq_device_index* d, uint32_t k, uint32_t shard, uint32_t n_shards, uint64_t* u_ref,
                          uint64_t* tot_ref);
/* Sums an unfinalized EM histogram over the ranks of comm (multiplicities added, interval ends by max: a position
 * that starts a multi-group interval on any rank starts the same interval everywhere), enqueued on stream and
 * synchronized. Every rank then holds the whole job's histogram (speq_em_finalize / speq_em_step as usual). */
int speq_em_allreduce(speq_em* em, void* comm, void* stream);
/* In-place sum over the ranks of comm of `count` u64 (is_f64 = 0) or f64 (is_f64 = 1) words in HOST memory (blocking;
 * RCCL communicators stage it through GPU `device`): the CLI's counters, weights, .dat sums, statistics and flags. */
int speq_allreduce_host(void* comm, int device, void* buf, uint64_t count, int is_f64);

/* ---- groupings file (speq::file_to_map, /root/reference/src/file_to_map.cpp:20-119) ----
 * Same grammar "Name(count): i, j-k, …"; parse errors of single tokens are collected (the reference prints
 * them to std::cerr) and returned by speq_groupings_errors(). A missing "(count)" fails with SPEQ_E_ARG
 * (std::invalid_argument from std::stoi at file_to_map.cpp:43). */
typedef struct speq_groupings speq_groupings;
int speq_groupings_parse(const char* path, speq_groupings** out);
uint32_t speq_groupings_n_groups(const speq_groupings* g);
const char* speq_groupings_name(const speq_groupings* g, uint32_t i);
int32_t speq_groupings_count(const speq_groupings* g, uint32_t i);
uint32_t speq_groupings_n_entries(const speq_groupings* g);
const int32_t* speq_groupings_scaffolds(const speq_groupings* g);
const char* speq_groupings_errors(const speq_groupings* g);
void speq_groupings_free(speq_groupings* g);

/* ---- launch tuning (performance only; results never depend on it) ----
 * "blocks_per_cu": cap resident 256-thread workgroups per CU (0 = no cap; the kernel's LDS is padded);
 *                  default by plane footprint: <= 16 MB none, <= 256 MB (Infinity Cache) 4, larger 3;
 * "grid_blocks"  : upper bound of the grid (default 16384 below 4 M symbols, else 8192);
 * "ilp"          : k-mer windows each lane searches concurrently, 1 or 2 (default 2 for indexes of < 4 M
 *                  symbols, else 1); "ilp_local" the same for Phred-weighted scans (default 1);
 * "prefix_level" : q-mer table used by scans: -1 (default) picks, per k, the longest of q, q-1, q-2 that leaves a
 *                  multiple of the widest LF step; 0..2 forces table q - level (results never change);
 * "sparse_prefix": 0 (default) dense q-mer tables; 1 a presence bitvector with ranks + the present intervals
 *                  (less memory, one more dependent load per window); -1 sparse when < 1/8 of the codes occur;
 * "fastq_gpu_parse": 1 (default) speq_scan_fastq parses blocks of simple four-line records on the GPU (raw text
 *                  to HBM); 0 parses every block on host threads. Results are identical;
 * "kmer_table"   : 1 (default) scans of k <= 31 look each N-free window up in the replica's k-mer interval table
 *                  for k (built by the first scan with that k, or by speq_device_prepare); 0 searches every window
 *                  with LF steps. Results are identical;
 * "kt_compact"   : 1 (default) 8-B-slot tables for k <= 23 (0: 16-B slots); "kt_load8": their load factor in percent
 *                  (default 35); "kt_slots": 16-B slots per distinct k-mer of the wide form (default 2). These apply to
 *                  tables built afterwards;
 * "ilp_kt"       : windows per lane of table scans, 1 or 2 (pipelined kernel), 4 (k_scan); 0 (default) = 1 for
 *                  compact tables (k <= 23), 2 for 16-B-slot tables;
 *                  "kt_pipeline": 1 (default) the software-pipelined table kernel k_scan_kt, 0 k_scan;
 *                  "blocks_per_cu_kt": blocks_per_cu of table scans (default 0: no cap);
 * "stream_lanes" : compute streams of a pipeline created afterwards (speq_pipeline_create, speq_scan_fastq, host
 *                  scans), 1..8 (default 3): consecutive batches are parsed and scanned on them in turn, so the
 *                  short launches of different batches overlap on the CUs;
 * anchor-and-extend scans (k <= 128): "ax_scan" 1 (default) / 0 (other kernels), "ax_load" anchor-table load factor in
 *                  percent for tables built afterwards, "grid_blocks_ax" grid cap, "blocks_per_cu_ax" resident blocks
 *                  per CU (0: as registers/LDS allow), "ax_generations" grid = 1..16 times the resident blocks
 *                  (default 1: one persistent generation), "ax_mproof" m-mer absence proofs of the windows around a
 *                  mismatch (1 default: known and unknown mismatches, 2: known ones only, 0: off; results are the
 *                  same), "ax_sproof" substitution-bitmap proofs of the windows over a known mismatch (1: on, 0: off,
 *                  2 default: on for the k whose structures have no m-mer filter; the bitmap of a k is built by
 *                  speq_device_prepare or the first scan that uses it; results are the same);
 *                  "last_kernel" (read only) the kernel of the last scan: 0 LF steps (k_scan), 1 k-mer table (k_scan),
 *                  2 pipelined k-mer table (k_scan_kt), 3 anchor-and-extend (k_scan_ax);
 *                  "last_variant" (read only) the template instantiation of the last launch of one of these kernels,
 *                  the reference-uniqueness pass included (-1 before the first): bits 0-1 family (0 k_scan,
 *                  1 k_scan_kt, 2 k_scan_ax), bits 2-3 mode (0 global, 1 local, 2 reference pass), bit 4 paired,
 *                  bit 5 the tally in LDS (G <= 2048; else global atomics), bit 6 EM histogram, bits 7-9 windows per
 *                  lane (k_scan 1, 2, 4; k_scan_kt 1, 2) or 64-bit words per k-mer (k_scan_ax 1..4), bit 10 k_scan
 *                  with a k-mer table, bit 11 compact table, bit 12 substitution-bitmap path, bit 13 the instrumented
 *                  twin. A test ledger (tests/variant_table.py) states which value every scan must report. */
int speq_device_set_tuning(speq_device_index* d, const char* key, int64_t value);
int speq_device_get_tuning(const speq_device_index* d, const char* key, int64_t* value);

/* ---- k-mer interval table (the q-mer table of the FM-index taken to q = k) ----
 * For a scan length k <= 31 the replica keeps a hash table of every distinct N-free k-mer of the reference texts
 * with its SA interval start and its classification (one group, or the interval width when its occurrences span
 * >= 2 groups), computed once per distinct k-mer by FM backward search; a scan then resolves each window with one
 * 64-B bucket load instead of a chain of LF steps (an absent k-mer does not occur). Built on the replica's GPU by
 * the first scan with k, or here ahead of time; blocking. Outputs may be NULL; all zero when tables are off
 * (tuning "kmer_table" = 0), k > 31, or the table would not fit the free HBM (those scans use LF steps). Replaces no reference call; the reference
 * searches each window from scratch (fm_scanner.cpp:208). */
int speq_device_prepare(speq_device_index* d, uint32_t k, uint64_t* distinct_kmers, uint64_t* table_bytes,
                        double* build_ms);

/* Test accessor: copies the substitution bitmap of k (bit x of word x / 64: no single-base substitution at text
 * position x in any of the k windows over x gives a k-mer of the texts) to `words` (host,
 * u64[n_words], n_words >= ceil(n / 64)); builds the structures of k and the bitmap when they are missing. Fails with
 * SPEQ_E_ARG when the anchor-and-extend scan does not take k. Blocking. */
int speq_device_sproof_bitmap(speq_device_index* d, uint32_t k, uint64_t* words, uint64_t n_words);

/* Test accessor: what replica d holds for k, building nothing. facts (host, u64[n_facts], n_facts >=
 * SPEQ_BUILD_FACTS): [0] the anchor structures of k: 0 not asked for yet, 1 built, 2 deferred because the free device
 * memory was short (the next scan tries again), 3 refused (k, the group count or a 32-bit buffer offset: never
 * retried); of a built table [1] buckets nb, [2] filter words nf, [3] m of the m-mer filter (0: none), [4] its words
 * nmf, [5] the substitution bitmap's byte offset s_off, [6] its words s_words (0: none), [7] 1 when the representatives
 * came from the suffix sort, [8] 1 when the EM-only arrays exist, [9] the distinct k-mers; [10] the plane families the
 * replica published (bit 0 one-symbol, bit 1 two-symbol, bit 2 three-symbol); [11] the k-mer table of k: 0 not asked
 * for yet, 1 wide, 2 compact, 3 none (too large for the free memory at the time: kept for the replica's life); [12]
 * text positions n, [13] texts. */
#define SPEQ_BUILD_FACTS 14
int speq_device_build_facts(speq_device_index* d, uint32_t k, uint64_t* facts, uint32_t n_facts);

/* Test accessor: one run of the GPU FASTQ parser (fastq_gpu.hip, the parser of speq_scan_fastq's raw blocks) on
 * `device`. raw (host) holds file 1's four-line text [0, len1) followed, when paired, by file 2's [len1, len1 + len2);
 * n_records is the record count per file. The text is copied into a 16-byte aligned device buffer of
 * align16(len1 + len2) + 16 bytes whose remainder is filled with pad_byte; the parser's scratch, the offsets and the
 * two output buffers (len1 + len2 bytes each) are filled with `poison` first, then the parser is launched as the
 * stream path launches it. Outputs (host): seq / qual, all len1 + len2 bytes of each, so the bytes at and after
 * offsets[n_slots] show what the parser left alone; offsets, u64[n_slots + 1] with n_slots = n_records * (paired ? 2
 * : 1), records interleaved (slot 2r + f) when paired; *err, the OR of the records' flags (1 header not '@', 2
 * separator line, 4 base / quality counts, 8 too few lines; a flagged record has length 0); *total_bases =
 * offsets[n_slots] as the stream statistics get it. n_records = 0 launches nothing (offsets[0] = 0). Blocking. */
int speq_fastq_parse_block(int device, const uint8_t* raw, uint64_t len1, uint64_t len2, uint64_t n_records,
                           uint32_t paired, uint8_t pad_byte, uint8_t poison, uint8_t* seq, uint8_t* qual,
                           uint64_t* offsets, uint32_t* err, uint64_t* total_bases);

/* ---- kernel timing (HIP events on the launch stream; bench/roofline support) ----
 * Returns the summed elapsed milliseconds of the scan kernels launched by speq_scan_reads_device on
 * this handle since the last reset, and the number of launches.  Enabled by speq_timing_enable(d, 1). */
int speq_timing_enable(speq_device_index* d, int on);
int speq_timing_read(speq_device_index* d, double* total_ms, uint64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* SPEQ_SCAN_H */
