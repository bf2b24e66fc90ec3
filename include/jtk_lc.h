/* jtk_lc.h -- C ABI of the MI355X-native local-clustering stage (drop-in for the rayon loop of
 * ban-m/jtk haplotyper/src/local_clustering/mod.rs:64-72).
 *
 * Everything here is plain C: pointers, sizes and POD structs; no torch / HIP types.  All buffers are
 * caller-owned HOST memory unless a function name ends in `_dev`; the library never keeps a pointer
 * after returning, never throws/unwinds across the boundary, and returns 0 or a negative jtk_status.
 * The reference has no FFI layer (it is one Rust process); each entry point below cites the Rust item
 * it replaces, and INTEGRATION.md shows the `extern "C"` block + shim a jtk maintainer would add.
 *
 * Sequence encoding at the boundary: ASCII upper-case ACGT (the reference rejects anything else at
 * entry, haplotyper/src/entry.rs:40-45).  Alignment ops are one byte per column, values of
 * `kiley::Op` in the order the reference uses them (haplotyper/src/misc.rs:167-172):
 *   0 = Match, 1 = Mismatch, 2 = Ins (read base, no template base), 3 = Del (template base, no read base).
 */
#ifndef JTK_LC_H
#define JTK_LC_H

#include <stddef.h>
#include <stdint.h>

/* The library is built with -fvisibility=hidden: the entry points below (and the diagnostic ones of jtk_lc_debug.h) are
 * its only dynamic symbols. */
#if defined(__GNUC__) || defined(__clang__)
#define JTK_LC_API __attribute__((visibility("default")))
#else
#define JTK_LC_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever a public struct changes size or an entry point gains a precondition; a host compares it with
 * jtk_lc_version() before the first call.  2: jtk_lc_timing_t grew by chain_lds_bytes[2] (round 3) and
 * jtk_lc_cluster_chunks_multi checks the contiguous read_first layout itself (see there). */
#define JTK_LC_ABI_VERSION 2

/* kiley::hmm::NUM_ROW = 8 + COPY_SIZE + DEL_SIZE (pseudo_mcmc.rs:7,172,447): rows 0-3 substitute to
 * ACGT, 4-7 insert ACGT before the position, 8-10 copy 1-3 bp, 11-13 delete 1-3 bp. */
#define JTK_NUM_ROW 14
#define JTK_COPY_SIZE 3
#define JTK_DEL_SIZE 3
#define JTK_GAINS_MAX_HOMOP 8

enum jtk_op { JTK_OP_MATCH = 0, JTK_OP_MISMATCH = 1, JTK_OP_INS = 2, JTK_OP_DEL = 3 };

/* likelihood_gains.rs:194-199 (declaration order). */
enum jtk_diff_type { JTK_DIFF_SUBST = 0, JTK_DIFF_DEL = 1, JTK_DIFF_INS = 2 };

typedef enum jtk_status {
    JTK_OK = 0,
    JTK_ERR_INVALID_ARG = -1,     /* null pointer, inconsistent offsets, non-ACGT base, bad op code    */
    JTK_ERR_NO_DEVICE = -2,       /* no usable MI355X / HIP runtime failure (message via last_error)   */
    JTK_ERR_UNSUPPORTED = -3,     /* band radius > 255 (any read count is taken); jtk_lc_align_reads:  */
                                  /* a read farther from its template than max_dist, or > 32,000 bases */
                                  /* (jtk_lc_align_reads_mode: or a band > JTK_ALIGN_MODE_MAX_BAND)    */
    JTK_ERR_ALLOC = -4,           /* hipMalloc / host allocation failed                                */
    JTK_ERR_OPS_MISMATCH = -5,    /* ops do not consume exactly the template and the read              */
    JTK_ERR_CHUNK_FAILED = -6,    /* >=1 chunk hit a condition on which the reference panics; see      */
                                  /* chunk_status[] (e.g. WeightedError::AllWeightsZero, misc.rs:335)  */
    JTK_ERR_INTERNAL = -7
} jtk_status;

/* definitions/src/lib.rs:101-126 (same field order; model_tune.rs:36-63 maps it 1:1 onto
 * kiley::hmm::PairHiddenMarkovModel).  mat_emit[4*ref + read]; ins_emit[4*prev_read_base + read] with
 * prev = 4 for the first read base (own reading of kiley's 20-entry table). */
typedef struct jtk_hmm {
    double mat_mat, mat_ins, mat_del;
    double ins_mat, ins_ins, ins_del;
    double del_mat, del_ins, del_del;
    double mat_emit[16];
    double ins_emit[20];
} jtk_hmm_t;

/* likelihood_gains.rs:41-47 / :55-61. */
typedef struct jtk_gain_profile {
    double gain;
    double prob;
} jtk_gain_profile_t;

typedef struct jtk_gains {
    uint32_t max_homopolymer_len; /* 3 for estimate_gain_default (likelihood_gains.rs:189) */
    uint32_t reserved;
    jtk_gain_profile_t subst[JTK_GAINS_MAX_HOMOP];
    jtk_gain_profile_t deletions[JTK_GAINS_MAX_HOMOP];
    jtk_gain_profile_t insertions[JTK_GAINS_MAX_HOMOP];
} jtk_gains_t;

/* What local_clustering_selected computes once per call and passes by reference into every
 * clustering_on_pileup (mod.rs:57-62): the model on both strands, the calibrated gains, the haploid
 * coverage and the read type (only its band fraction matters here, definitions/src/lib.rs:173-175). */
typedef struct jtk_lc_params {
    jtk_hmm_t forward;
    jtk_hmm_t reverse;
    jtk_gains_t gains;
    double haploid_coverage;
    double band_frac; /* 0.03 ONT, 0.01 CCS, 0.05 CLR/None; band_width = ceil(len*frac), radius = band_width/2 */
} jtk_lc_params_t;

/* One pile-up = one call of clustering_on_pileup (mod.rs:86-123). Reads are already in the order fixed
 * by pileup_nodes (mod.rs:45-51); jtk_lc_pileup_sort_keys below gives the sort key. */
typedef struct jtk_lc_chunk {
    uint64_t chunk_id;   /* seeds the per-chunk RNG: Xoshiro256StarStar::seed_from_u64(id * 3490) (mod.rs:97) */
    uint32_t copy_num;   /* Chunk.copy_num (definitions/src/lib.rs:403-415) */
    uint32_t n_reads;
    uint64_t tmpl_off;   /* into tmpl_bases */
    uint64_t tmpl_len;
    uint64_t read_first; /* index of this chunk's first read in read_off / ops_off / strand */
} jtk_lc_chunk_t;

/* Per-chunk result record. */
typedef struct jtk_lc_result {
    double score;         /* Chunk.score (mod.rs:78)        */
    uint32_t cluster_num; /* Chunk.cluster_num (mod.rs:79)   */
    int32_t status;       /* 0, or the jtk_status this chunk failed with */
    uint32_t polish_rounds;
    uint32_t n_variants;  /* D: number of selected variant columns (filter_profiles) */
} jtk_lc_result_t;

/* ---- the drop-in entry point ------------------------------------------------------------------
 * Replaces `pileups.into_par_iter()...map(clustering_on_pileup)` (mod.rs:64-72) for a batch of chunks:
 * consensus polishing (mod.rs:105-106), variant search (pseudo_mcmc.rs:109-138), clustering
 * (pseudo_mcmc.rs:213-274, 77-107) and the per-node write-back data of update_by_clusterings
 * (mod.rs:244-260).  Chunks with copy_num >= 8 take clustering_recursive's split branch (mod.rs:138-189):
 * a 4-way clustering, then per group a consensus polish and a clustering with the group's share of the
 * copies, merged as mod.rs:161-187 does; post_stride must be >= the largest copy_num of the batch.
 *
 * label[r]        : Node.cluster of read r (before normalize_local_clustering).
 * log_post        : row r has post_stride doubles; the first result[c].cluster_num are Node.posterior
 *                   (log posterior, rows logsumexp to 0), the rest are written as 0.
 * cons_out        : polished consensus of chunk c at cons_off[c] .. cons_off[c+1]; the caller provides
 *                   capacity cons_cap bytes in total (>= sum(tmpl_len) + 64*n_chunks is always enough:
 *                   the library fails the chunk rather than overrun).
 * ops_out         : re-threaded per-base ops of read r at ops_out_off[r] .. ops_out_off[r+1], capacity
 *                   ops_cap bytes (sum(ops_len) + 8*polish edits; same overrun rule).
 * device          : HIP device ordinal (one process drives one GPU; multi-GPU = one process per GPU).
 */
JTK_LC_API int jtk_lc_cluster_chunks(const jtk_lc_params_t *params, size_t n_chunks, const jtk_lc_chunk_t *chunks,
                          const uint8_t *tmpl_bases, const uint8_t *read_bases, const uint64_t *read_off,
                          const uint8_t *ops, const uint64_t *ops_off, const uint8_t *strand,
                          uint32_t *label, double *log_post, uint32_t post_stride, jtk_lc_result_t *result,
                          uint8_t *cons_out, uint64_t *cons_off, uint64_t cons_cap, uint8_t *ops_out,
                          uint64_t *ops_out_off, uint64_t ops_cap, int device);

/* The same call over several GPUs of one node from one host process (SURVEY 8b's `device_mask`, as a list): chunks are
 * dealt to `devices` by longest-processing-time-first over a cost model (pair-HMM cells + Metropolis steps per candidate k;
 * the partition bench.py / jtk_amd.sharding use between ranks), each share is gathered into its own batch and runs as on a
 * single device (sliced, overlapped), and the outputs are scattered back into the caller's order, laid out as above.  Chunks are independent (one RNG stream per chunk id), so results do not depend on
 * the device list; the path has no exchange step and no collective runs.  A device may be listed more than once.
 * Precondition (checked here since ABI 2, as the single-device call always did when it built its session): the chunks' reads
 * are laid out back to back in chunk order (chunks[0].read_first == 0, chunks[c + 1].read_first == chunks[c].read_first +
 * chunks[c].n_reads) -- JTK_ERR_INVALID_ARG otherwise. */
JTK_LC_API int jtk_lc_cluster_chunks_multi(const jtk_lc_params_t *params, size_t n_chunks, const jtk_lc_chunk_t *chunks,
                                const uint8_t *tmpl_bases, const uint8_t *read_bases, const uint64_t *read_off,
                                const uint8_t *ops, const uint64_t *ops_off, const uint8_t *strand,
                                uint32_t *label, double *log_post, uint32_t post_stride, jtk_lc_result_t *result,
                                uint8_t *cons_out, uint64_t *cons_off, uint64_t cons_cap, uint8_t *ops_out,
                                uint64_t *ops_out_off, uint64_t ops_cap, const int *devices, size_t n_devices);

/* Same, but the template is an already polished consensus and ops are already re-threaded: skips
 * polish_until_converge_antidiagonal.  This is `pseudo_mcmc::clustering` (pseudo_mcmc.rs:77-107) batched;
 * a Rust host that keeps real kiley polishing calls this one and inherits exactness downstream.
 * cons_out/ops_out are not produced. */
JTK_LC_API int jtk_lc_cluster_polished(const jtk_lc_params_t *params, size_t n_chunks, const jtk_lc_chunk_t *chunks,
                            const uint8_t *tmpl_bases, const uint8_t *read_bases, const uint64_t *read_off,
                            const uint8_t *ops, const uint64_t *ops_off, const uint8_t *strand,
                            uint32_t *label, double *log_post, uint32_t post_stride,
                            jtk_lc_result_t *result, int device);

/* ---- the polishing step on its own -------------------------------------------------------------------
 * kiley `polish_until_converge_antidiagonal(template, seqs, ops, strands, &HMMPolishConfig::new(radius, take_num,
 * ignore_edge))` for a batch of independent windows (one jtk_lc_chunk_t each; copy_num is ignored): the call
 * `consensus::polish_seg` makes on 2 kbp windows of contigs (haplotyper/src/consensus/mod.rs:476-483 with
 * (radius / 2, max_coverage, 0)) and the one this stage makes per pile-up (local_clustering/mod.rs:105-106 with
 * (band / 2, N, 3)).  Only the first take_num reads of a window vote in a round (0 = all); every read's ops are
 * re-threaded.  radius 0 derives the radius from the window length and params->band_frac as mod.rs:96 does.
 * result[c].polish_rounds / .status are filled; cons_out / ops_out as in jtk_lc_cluster_chunks. */
JTK_LC_API int jtk_lc_polish_chunks(const jtk_lc_params_t *params, size_t n_chunks, const jtk_lc_chunk_t *chunks,
                         const uint8_t *tmpl_bases, const uint8_t *read_bases, const uint64_t *read_off,
                         const uint8_t *ops, const uint64_t *ops_off, const uint8_t *strand, uint32_t radius,
                         uint32_t take_num, uint32_t ignore_edge, uint8_t *cons_out, uint64_t *cons_off, uint64_t cons_cap,
                         uint8_t *ops_out, uint64_t *ops_out_off, uint64_t ops_cap, jtk_lc_result_t *result, int device);

/* ---- making the ops: global read-to-template alignment -------------------------------------------------
 * edlib Global / Alignment as the reference calls it (`global_align`, haplotyper/src/consensus/mod.rs:424-435, around the
 * polish of `polish_seg` :437-443, :490-494; per node in `PolishChunk::consensus_chunk`, polish_chunks.rs:114-120): the
 * unit-cost alignment ops of every read of every chunk against that chunk's template, which the entry points above take as
 * input.  Among the optimal alignments the one of DESIGN.md section 4 is returned (walk from the end; diagonal, then Del,
 * then Ins); parity with edlib's own tie-breaking is not pinned.  chunks / tmpl_bases / read_bases / read_off as in
 * jtk_lc_polish_chunks; copy_num and chunk_id are ignored.
 * ops_out     : ops of read r at ops_out_off[r] .. ops_out_off[r+1], capacity ops_cap bytes (sum(tmpl_len + read_len) over
 *               the reads is always enough; JTK_ERR_INVALID_ARG rather than an overrun when it is too small).
 * dist_out[r] : the edit distance of read r.
 * max_dist    : 0 = unbounded (sequences up to 32,000 bases each are taken).  A read farther from its template than
 *               max_dist, or longer than that cap, gets read_status[r] = JTK_ERR_UNSUPPORTED, dist_out[r] = UINT32_MAX and
 *               an empty op slot; the call then returns JTK_ERR_CHUNK_FAILED and every other read is aligned. */
JTK_LC_API int jtk_lc_align_reads(size_t n_chunks, const jtk_lc_chunk_t *chunks, const uint8_t *tmpl_bases,
                       const uint8_t *read_bases, const uint64_t *read_off, uint32_t max_dist,
                       uint8_t *ops_out, uint64_t *ops_out_off, uint64_t ops_cap,
                       uint32_t *dist_out, int32_t *read_status, int device);

/* ---- the same with one sequence's ends free: edlib Infix / Prefix with AlignTask::Alignment -------------------
 * What the reference calls wherever it places one sequence inside a slightly longer window of another: `semiglobal`
 * (haplotyper/src/encode/mod.rs:227-246, the tips of every encoded node), the chunk laid into a read window
 * (encode/deletion_fill.rs:544-554), dense_encoding.rs:728-757, determine_chunks.rs:520-538, and `align_infix` /
 * `align_leading` / `align_trailing` (consensus/mod.rs:563-614), with which `fix_alignment` re-anchors every read after a
 * round of window polishing (`polish`, :300-371).  One sequence of a pair is whole (edlib's query) and is consumed
 * entirely; the other is free (edlib's target), `free_seq` says which, and only its stretch [start, end) is consumed:
 *   JTK_ALIGN_INFIX  : both ends of the free sequence are free; the distance is the smallest over all its substrings.
 *   JTK_ALIGN_PREFIX : its start is pinned to 0, its end is free; the smallest over all its prefixes.
 *   JTK_ALIGN_GLOBAL : jtk_lc_align_reads (same ops and distances); free_seq is ignored, start = 0, end = tmpl_len.
 * Among equally good placements the smallest end is returned, and for it the path of DESIGN.md section 4 (walk from the end
 * cell; diagonal, then Del, then Ins -- in either orientation; infix: the walk stops at the first cell on the free
 * boundary, which gives start).  Parity with edlib's own choice among equally good placements and paths is not pinned.
 * The op meanings do not change with free_seq: Del consumes a template base, Ins a read base.  An empty whole sequence
 * gives distance 0, no ops and start = end = 0; an empty free sequence gives whole-length x Ins (the read is whole) or
 * x Del (the template is whole) and start = end = 0.
 * Batch layout, validation, ops_out / ops_cap, dist_out, read_status, the per-read failure rule and max_dist are those of
 * jtk_lc_align_reads; start_out[r] / end_out[r] are 0 for a failed read.  Limits (JTK_ERR_UNSUPPORTED for the read, the rest
 * of the batch is aligned): 32,000 bases per sequence, and JTK_ALIGN_MODE_MAX_BAND diagonals in the band that certifies
 * the largest distance the call allows -- min(max_dist, whole length), see DESIGN.md section 4 for the band -- which is
 * decided per read before anything is launched (the kernel keeps 3 bytes of LDS per diagonal).  With max_dist = 0 that is
 * every pair with tmpl_len + read_len < 32,768; longer pairs need a max_dist.
 * mode / free_seq outside the enums: JTK_ERR_INVALID_ARG. */
enum jtk_align_mode { JTK_ALIGN_GLOBAL = 0, JTK_ALIGN_INFIX = 1, JTK_ALIGN_PREFIX = 2 };
enum jtk_align_free { JTK_ALIGN_FREE_TEMPLATE = 0, JTK_ALIGN_FREE_READ = 1 };
#define JTK_ALIGN_MODE_MAX_BAND 32768
JTK_LC_API int jtk_lc_align_reads_mode(size_t n_chunks, const jtk_lc_chunk_t *chunks, const uint8_t *tmpl_bases,
                            const uint8_t *read_bases, const uint64_t *read_off, int mode, int free_seq, uint32_t max_dist,
                            uint8_t *ops_out, uint64_t *ops_out_off, uint64_t ops_cap,
                            uint32_t *dist_out, uint32_t *start_out, uint32_t *end_out, int32_t *read_status, int device);

/* ---- resident-batch form of the same call ----------------------------------------------------------
 * jtk_lc_cluster_chunks == session_create + session_run(0) + session_fetch + session_destroy.
 * A session uploads the batch once (inputs stay resident in HBM, all device workspaces are allocated
 * up front), so repeated runs measure the device path without PCIe; bench.py times session_run.
 * The reference enters this stage up to ~6 times per pipeline run on overlapping chunk sets
 * (cli/src/pipeline.rs:158,164-168), which is what a resident session serves. */
typedef struct jtk_lc_session jtk_lc_session_t;
JTK_LC_API int jtk_lc_session_create(const jtk_lc_params_t *params, size_t n_chunks, const jtk_lc_chunk_t *chunks,
                          const uint8_t *tmpl_bases, const uint8_t *read_bases, const uint64_t *read_off,
                          const uint8_t *ops, const uint64_t *ops_off, const uint8_t *strand,
                          uint32_t post_stride, int device, jtk_lc_session_t **out);
/* One pass of the hot path over the resident batch; skip_polish != 0 gives jtk_lc_cluster_polished
 * semantics.  Returns after the device has finished; results stay on the device until fetched. */
JTK_LC_API int jtk_lc_session_run(jtk_lc_session_t *s, int skip_polish);
/* Copies the last run's results out (any pointer may be NULL to skip that output). */
JTK_LC_API int jtk_lc_session_fetch(jtk_lc_session_t *s, uint32_t *label, double *log_post, jtk_lc_result_t *result,
                         uint8_t *cons_out, uint64_t *cons_off, uint64_t cons_cap, uint8_t *ops_out,
                         uint64_t *ops_out_off, uint64_t ops_cap);
JTK_LC_API int jtk_lc_session_destroy(jtk_lc_session_t *s);
/* The reference's trace! rows (log level Trace) of ONE chunk's clustering, after a jtk_lc_session_run: '\n'-terminated rows, in the
 * order the reference logs them -- TOTAL, CAND per candidate column (pseudo_mcmc.rs:467-472), PICK per picked column (:539),
 * DUMP per selected column (:122-127), RANGE (:236), and per candidate cluster count the two LK rows (:250, :256) and, where the
 * count was accepted, COUNTS (:262).  (Not written: the per-column PVALUE / RAWCOUNT / FILTER rows of the filter, REMOVE, VARS.)
 * The chunk's pick and its chain run once more on the device, in instantiations that record what the rows need (the product
 * kernels carry none of it); labels, posteriors and scores come out as they were.  *len = bytes of text (no terminator);
 * JTK_ERR_INVALID_ARG with *len set when cap is too small; JTK_ERR_UNSUPPORTED for a session that holds a chunk of copy number
 * >= 8 (clustering_recursive, mod.rs:125-189); a chunk of copy number < 2 logs nothing (pseudo_mcmc.rs:86-88). */
JTK_LC_API int jtk_lc_session_trace(jtk_lc_session_t *s, size_t chunk, char *text, size_t cap, size_t *len);

/* ---- stage pieces, exported because the reference exposes them too ------------------------------ */

/* `pseudo_mcmc::modification_table` (pseudo_mcmc.rs:45-68) for one pile-up: for read r, table[r] has
 * JTK_NUM_ROW*(tmpl_len+1) doubles = kiley modification_table_antidiagonal(...) MINUS lk[r]
 * (pseudo_mcmc.rs:62-64); lk[r] is the read's log-likelihood under the unedited template. */
JTK_LC_API int jtk_lc_modification_table(const jtk_lc_params_t *params, const uint8_t *tmpl, uint64_t tmpl_len,
                              uint32_t n_reads, const uint8_t *read_bases, const uint64_t *read_off,
                              const uint8_t *ops, const uint64_t *ops_off, const uint8_t *strand,
                              double *table, double *lk, int device);

/* `pseudo_mcmc::cluster_filtered_variants` + the re-assignment / posterior tail of `clustering`
 * (pseudo_mcmc.rs:213-274, 98-105) on caller-supplied feature matrices (the entry the reference's
 * sandbox/src/bin/benchmark_mcmc.rs:111-114 drives).  Chunk c: variants[var_off[c] ..] is n_reads x dim
 * row-major, variant_type[vt_off..] is dim x (homop_len, jtk_diff_type) pairs of uint32. */
typedef struct jtk_lc_feature_chunk {
    uint64_t chunk_id;
    uint32_t copy_num;
    uint32_t n_reads;
    uint32_t dim;
    uint32_t reserved;
    uint64_t var_off;  /* in doubles */
    uint64_t vt_off;   /* in (uint32,uint32) pairs */
    uint64_t read_first;
    double local_coverage; /* ClusteringConfig.local_coverage (mod.rs:108-112) */
} jtk_lc_feature_chunk_t;

JTK_LC_API int jtk_lc_cluster_features(const jtk_lc_params_t *params, size_t n_chunks,
                            const jtk_lc_feature_chunk_t *chunks, const double *variants,
                            const uint32_t *variant_type, uint32_t *label, double *log_post,
                            uint32_t post_stride, jtk_lc_result_t *result, int device);

/* ---- host-side helpers (no GPU needed) ------------------------------------------------------------ */

/* ---- stage preamble: gains calibration ------------------------------------------------------------
 * Replaces `estimate_gain(hmm, seed, seq_len, band, homop_len)` (likelihood_gains.rs:162-184); the stage
 * calls it through `estimate_gain_default` = (hmm, 309423, 100, 10, 3) (likelihood_gains.rs:186-192,
 * local_clustering/mod.rs:60).  Per (type, homopolymer length) profile: 100 simulated variant pairs x 100
 * simulated reads, every read scored against both members of its pair with the banded pair-HMM
 * (likelihood_antidiagonal_bootstrap); the sampling runs on the host, the bootstrap alignments and the
 * likelihoods on the device.  `out` is what jtk_lc_params_t.gains expects. */
JTK_LC_API int jtk_lc_estimate_gains(const jtk_hmm_t *forward, const jtk_hmm_t *reverse, uint64_t seed, uint32_t seq_len,
                          uint32_t band, uint32_t homop_len, jtk_gains_t *out, int device);

/* `estimate_minimum_gain(&hmm)` (likelihood_gains.rs:6-39), the scale of correct_clustering's protection rule
 * (phmm_likelihood_correction.rs:118: min_gain = estimate_minimum_gain(&hmm) * PROTECT_FACTOR).  sample_num templates of
 * `len` random bases, each with one base deleted (kiley introduce_errors(.., 0, 1, 0)); per template the median over seq_num
 * simulated reads of lk(read | template) - lk(read | template minus the base) with the banded bootstrap likelihood; the
 * third smallest median, at least 1.  The reference's constants: seed 23908, 1000, 500, 100, band 25.  Sampling on the
 * host, alignments and likelihoods on the device (the machinery of jtk_lc_estimate_gains; own specification of kiley). */
JTK_LC_API int jtk_lc_estimate_minimum_gain(const jtk_hmm_t *forward, const jtk_hmm_t *reverse, uint64_t seed, uint32_t sample_num,
                                 uint32_t seq_num, uint32_t len, uint32_t band, double *out, int device);

/* ---- stage preamble: model refit ----------------------------------------------------------------------
 * Replaces `estimate_model_parameters_on_both_strands` (haplotyper/src/model_tune.rs:119-152; entered through
 * `update_models_on_both_strands`, local_clustering/mod.rs:58) on the training pile-ups the host has selected
 * (model_tune.rs:99-118: coverage within 2 of the median, sorted by chunk id, the first TRAIN_UNIT_SIZE = 5):
 * `rounds` (TRAIN_ROUND = 10) times [ polish every pile-up with HMMPolishConfig::new(band / 2, N, 0), then one
 * Baum-Welch step over all of them with the largest band's radius ].  params->forward / reverse are the starting model
 * (DataSet.model_param), params->band_frac the read type's; the refitted models are what jtk_lc_params_t.forward /
 * .reverse then carry.  kiley's fit is not part of the reference tree: the step is this build's own specification
 * (expected transition / emission counts of the banded pair-HMM, rows renormalised). */
JTK_LC_API int jtk_lc_fit_model(const jtk_lc_params_t *params, size_t n_chunks, const jtk_lc_chunk_t *chunks,
                     const uint8_t *tmpl_bases, const uint8_t *read_bases, const uint64_t *read_off,
                     const uint8_t *ops, const uint64_t *ops_off, const uint8_t *strand, uint32_t rounds,
                     jtk_hmm_t *forward_out, jtk_hmm_t *reverse_out, int device);

/* ---- the first consumer of the stage's posteriors: cross-chunk correction ------------------------------------
 * Replaces `AlignmentCorrection::correct_clustering_selected` (haplotyper/src/phmm_likelihood_correction.rs:32-97): per
 * selected chunk with more than one cluster, a read-by-read similarity matrix from a 3-state affine-gap alignment of the
 * neighbouring nodes' posteriors (`alignment` :466-479, `align_swg` :482-531, `sim` :534-550; on the device), then spectral
 * clustering on the host (graph Laplacian :385-402, eigenvectors below 0.2 :405-464, 20 x misc::kmeans :295-302), the
 * adjusted Rand index against the previous labels (:220-240), suppression of the lowest 5 % (:100-105) unless the chunk's
 * local-clustering score protects it (:108-129).
 * The data set reaches the call flattened: read r owns nodes node_off[r] .. node_off[r+1] (in read order), node e has
 * post_len log-posteriors at posteriors[post_off].  chunks[] is DataSet.selected_chunks (cluster_num is updated in place).
 * min_gain is `estimate_minimum_gain(&hmm) * PROTECT_FACTOR` (:118): a simulation through kiley that the caller runs.
 * Output: cluster_out[e] = Node.cluster after the call, touched[e] = 1 where the reference rewrites the node; its posterior
 * then is -10000 everywhere except 0 at the new cluster, with the chunk's NEW cluster_num entries (:88-93).
 * Returns JTK_ERR_CHUNK_FAILED where the reference panics (a pile-up smaller than 4 x copy_num :348+:361, no eigenvalue
 * below the threshold :455, posterior lengths that differ from cluster_num :547, ...); nothing is written then. */
typedef struct jtk_cc_node {
    uint64_t chunk;      /* Node.chunk                 (definitions/src/lib.rs:672-683) */
    uint64_t cluster;    /* Node.cluster                */
    uint32_t is_forward; /* Node.is_forward             */
    uint32_t post_len;   /* Node.posterior.len()        */
    uint64_t post_off;   /* into `posteriors`           */
} jtk_cc_node_t;
typedef struct jtk_cc_chunk {
    uint64_t id;          /* Chunk.id                   (definitions/src/lib.rs:403-415) */
    uint32_t cluster_num; /* Chunk.cluster_num (in / out) */
    uint32_t copy_num;    /* Chunk.copy_num             */
    double score;         /* Chunk.score                */
} jtk_cc_chunk_t;
JTK_LC_API int jtk_lc_correct_clustering(size_t n_reads, const uint64_t *read_id, const uint64_t *node_off, const jtk_cc_node_t *nodes,
                              const double *posteriors, size_t n_chunks, jtk_cc_chunk_t *chunks, size_t n_selected,
                              const uint64_t *selection, double haploid_coverage, double min_gain, uint64_t *cluster_out,
                              uint8_t *touched, int device);

/* ---- the step in front of the correction: squish erroneous clusters ---------------------------------------------
 * Replaces `SquishErroneousClusters::squish_erroneous_clusters` (haplotyper/src/squish_erroneous_clusters.rs:44-60), which
 * both call sites of correct_clustering run first on the same DataSet (cli/src/pipeline.rs:174-175,
 * haplotyper/src/dense_encoding.rs:62-64).  On the flattened data set of jtk_lc_correct_clustering:
 *   - a node is biased when Node::is_biased(0.2) holds (definitions/src/lib.rs:703-709);
 *   - every position pair i < j of biased nodes of a read adds 1 to the chunk pair (min id, max id) (:80-90; a chunk twice in
 *     a read gives (u, u)); pairs with count_thr < count whose two chunks have 1 < cluster_num survive (:96-97);
 *   - per surviving pair, the adjusted Rand index (misc.rs:22-46, in 64-bit integers and one division) of the reads' minimum
 *     clusters on the two chunks, one observation per read that has biased nodes of both (:213-252);
 *   - classify (:254-365): chunks are labelled stiff or not by 10 x (one sweep + 1,000 Metropolis proposals) on the pair
 *     graph, Xoshiro256PlusPlus::seed_from_u64(3093240);
 *   - class per chunk of chunks[] (:137-165): JTK_REL_STIFF if labelled stiff or 2 < copy_num, else JTK_REL_SUSPICIOUS if a
 *     pair in which it is the SMALLER id names a stiff chunk, else JTK_REL_ISOLATED.
 * Pair order.  The reference's pair list comes out of a HashMap under par_iter: its order, and with it classify's node
 * numbering, sweep order and summation order, differs from run to run.  This build fixes one admissible order: pairs
 * ascending by (u1, u2).  It is the order of the optional pair list below.
 * Output: class_out[c] per chunk; chunks[c].cluster_num = 1 where suspicious; cluster_out[e] = Node.cluster after the call,
 * touched[e] = 1 where the reference rewrites the node (a node of a suspicious chunk: cluster 0), whose posterior then is one
 * entry, 0.0 (:55-58).  With all of pair_u1 / pair_u2 / pair_ari / pair_count given (any NULL skips all four) the surviving pairs
 * are returned, pair_count being the number of observations (what classify weighs); JTK_ERR_INVALID_ARG with *n_pairs set
 * when pair_cap is too small.
 * Returns JTK_ERR_CHUNK_FAILED where the reference panics (a pair above count_thr whose retain indexes a chunk id that is not
 * in chunks[], :97), and JTK_ERR_UNSUPPORTED when a read that enters the table of a surviving pair has a biased node of either
 * chunk with cluster >= 64 (the table is 64 x 64 counters; the reference sizes its table by the largest label and has no such
 * limit) or a read has more than 65535 nodes.  Nothing is written on failure. */
typedef struct jtk_squish_config {
    double ari_thr, match_score, mismatch_score;
    uint64_t count_thr;
} jtk_squish_config_t;
/* SquishConfig::default(): 0.5, 4, -1, 10 (squish_erroneous_clusters.rs:29-38) */
enum jtk_rel_class { JTK_REL_STIFF = 0, JTK_REL_ISOLATED = 1, JTK_REL_SUSPICIOUS = 2 };
JTK_LC_API int jtk_lc_squish_clusters(size_t n_reads, const uint64_t *node_off, const jtk_cc_node_t *nodes, const double *posteriors,
                           size_t n_chunks, jtk_cc_chunk_t *chunks, const jtk_squish_config_t *cfg, uint8_t *class_out,
                           uint64_t *cluster_out, uint8_t *touched, uint64_t *pair_u1, uint64_t *pair_u2, double *pair_ari,
                           uint64_t *pair_count, size_t pair_cap, size_t *n_pairs, int device);
/* Host only, no GPU: classify (:254-365) on a pair list in the order GIVEN.  ids[] = the chunk ids in first-appearance order
 * over the list (u1 then u2), stiff[i] = 1 where ids[i] is labelled stiff.  JTK_ERR_INVALID_ARG with *n_ids set when id_cap
 * is too small. */
JTK_LC_API int jtk_lc_squish_classify(size_t n_pairs, const uint64_t *u1, const uint64_t *u2, const double *ari, const uint64_t *count,
                           const jtk_squish_config_t *cfg, uint64_t *ids, uint8_t *stiff, size_t id_cap, size_t *n_ids);

/* ---- the step after the stage: purge diverged clusters, and the two functions it rests on ---------------------------
 * `ds.purge(&purge_config)` runs right after local_clustering, twice (cli/src/pipeline.rs:164-165; purge_diverged.rs:42-48):
 * purge_diverged_nodes (:238-322), then re_cluster (:189-236), which estimates copy numbers over the assembly graph (not part
 * of this library) and calls local_clustering_selected on the purged chunks (jtk_lc_cluster_chunks).  It rests on
 * `determine_chunks::calc_sim_thr` (determine_chunks.rs:796-823) and `estimate_error_rate::estimate_error_rate`
 * (estimate_error_rate.rs:37-133), which correct_deletion (encode/deletion_fill.rs:141-144), jtk.rs:251-253 and
 * determine_chunks.rs:113,157,164 call too: they have entry points of their own.  purge_largeindel is not covered.
 * The data set is flattened as for jtk_lc_correct_clustering (n_reads, node_off, nodes in encoded_reads order, chunks), plus
 * what Node::recover (definitions/src/lib.rs:773-813) reads: node e's sequence at seq_bases[seq_off[e] .. seq_off[e+1]) and its
 * per-base ops at ops[ops_off[e] .. ops_off[e+1]) (codes as above; 0 and 1 both stand for a cigar Match column, whether it
 * shows '|' or 'X' is decided by the bases; the ops_out of jtk_lc_cluster_chunks can be passed as it is), and chunk c's
 * sequence (c indexes chunks[]) at tmpl_bases[tmpl_off[c] .. tmpl_off[c+1]).  Bases are compared after ASCII upper-casing; no
 * base is refused.  Chunk ids must not repeat in chunks[] (JTK_ERR_INVALID_ARG); a sequence, op list or template of 2^31
 * bytes or more is JTK_ERR_UNSUPPORTED.
 *
 * jtk_lc_node_errors: per node, err_len[e] = the number of alignment columns and err_num[e] = those that are not '|'; the
 * node's error rate is err_num / err_len as one f64 division (determine_chunks.rs:796-803 == estimate_error_rate.rs:68-70).
 * status[e]: 0, or, decided by the first op in order that fails,
 *   JTK_ERR_OPS_MISMATCH  an op steps past the end of the node's sequence or of the template (the reference's slice panics;
 *                         ops that consume LESS than a sequence are accepted: recover does not check),
 *   JTK_ERR_INVALID_ARG   an op code above 3,
 *   JTK_ERR_CHUNK_FAILED  a node without columns (0 / 0) or of a chunk id that is not in chunks[] (chunks[&node.chunk]);
 * err_num = err_len = 0 for such a node.  Returns JTK_ERR_CHUNK_FAILED if any node failed; every node is written. */
JTK_LC_API int jtk_lc_node_errors(size_t n_reads, const uint64_t *node_off, const jtk_cc_node_t *nodes, size_t n_chunks,
                       const jtk_cc_chunk_t *chunks, const uint8_t *seq_bases, const uint64_t *seq_off, const uint8_t *ops,
                       const uint64_t *ops_off, const uint8_t *tmpl_bases, const uint64_t *tmpl_off, uint32_t *err_num,
                       uint32_t *err_len, int32_t *status, int device);
/* calc_sim_thr (determine_chunks.rs:806-823): the value at index min(floor(n_nodes x quantile), n_nodes - 1) of the ascending
 * error rates err_num[e] / err_len[e].  JTK_ERR_INVALID_ARG for a quantile outside [0, 1], n_nodes = 0 or an err_len of 0. */
JTK_LC_API int jtk_lc_error_quantile(size_t n_nodes, const uint32_t *err_num, const uint32_t *err_len, double quantile, double *out,
                          int device);
/* estimate_error_rate (estimate_error_rate.rs:37-133) on the nodes' error counts: one rate per read (read_err[n_reads], by
 * position in the flattened data set; a read without nodes gets the 0 / 0 of :101 as the NaN 0x7ff8000000000000) and one per
 * (chunk, cluster): chunk c's clusters at chunk_err[chunk_err_off[c] .. chunk_err_off[c+1]), chunk_err_off[n_chunks + 1] being
 * the prefix sum of cluster_num (the caller gives chunk_err_cap doubles; sum(cluster_num) are needed), the square root of the
 * median squared residual, and the number of passes of the loop :78-108.  Every sum runs in the reference's order (chunk rates:
 * reads in order, their nodes in order; the regulariser :32: chunks ascending by id), so the outputs and the pass count are
 * the reference's bit for bit.  fallback is every read's first rate (:55-58).
 * JTK_ERR_CHUNK_FAILED: a node's cluster is not below its chunk's cluster_num or its chunk is not in chunks[] (:49-50 index
 * out of bounds), or 100,000 passes without convergence (the reference would not return).  JTK_ERR_INVALID_ARG: no nodes (the
 * median of nothing, :123-126), an err_len of 0, chunk_err_cap too small.  Nothing is written on failure. */
JTK_LC_API int jtk_lc_estimate_error_rate(size_t n_reads, const uint64_t *node_off, const jtk_cc_node_t *nodes, const uint32_t *err_num,
                               const uint32_t *err_len, size_t n_chunks, const jtk_cc_chunk_t *chunks, double fallback,
                               double *read_err, double *chunk_err, uint64_t *chunk_err_off, size_t chunk_err_cap,
                               double *median_of_sqrt_err, uint32_t *n_iter, int device);
/* purge_diverged_nodes (purge_diverged.rs:238-322) with get_diverged_clusters (:299-309) on one upload: the node errors, their
 * 0.5 quantile as the fallback (:301), the fit, then diverged[slot] = thr < chunk_err[slot] (THR = 0.1, :40); a chunk whose
 * clusters are ALL diverged keeps them all (:241-249).  n_post = the length of the data set's posterior array (only the nodes'
 * post_off / post_len are read).  Output, to be applied by the caller:
 *   diverged[], chunk_err_off[]  flat as in jtk_lc_estimate_error_rate (slot_cap entries given, sum(cluster_num) needed)
 *   chunks[c].cluster_num        reduced by the chunk's number of flags (:261-265)
 *   keep[e]                      0 where the node's (chunk, cluster) is flagged: the node is removed (:271-272)
 *   cluster_out[e]               Node.cluster minus the flagged clusters below it (:312-316)
 *   touched[e]                   1 for a kept node of a chunk with a flag: remove_diverged rewrites it (:273-278)
 *   post_keep[n_post]            0 for the posterior entries remove_diverged drops (:318-321), 1 everywhere else
 *   purged[], *n_purged          the chunk ids with a flag, ascending (:291-295; purged_cap entries given, n_chunks suffice)
 *   read_err, chunk_err, median_of_sqrt_err   the fit, each optional (NULL skips it)
 * The caller then drops the reads left without nodes (:283) and rebuilds every read's gaps and edges from its nodes
 * (encode::nodes_to_encoded_read, :284-290).
 * JTK_ERR_CHUNK_FAILED: a node fails in jtk_lc_node_errors, the fit fails, or a kept node of a chunk with a flag carries a
 * posterior longer than the chunk's cluster_num (:320 indexes past cluster_info).  JTK_ERR_INVALID_ARG: no nodes
 * (calc_sim_thr indexes an empty list), slot_cap or purged_cap too small.  Nothing is written on failure, chunks[] included. */
JTK_LC_API int jtk_lc_purge_diverged(size_t n_reads, const uint64_t *node_off, const jtk_cc_node_t *nodes, size_t n_post, size_t n_chunks,
                          jtk_cc_chunk_t *chunks, const uint8_t *seq_bases, const uint64_t *seq_off, const uint8_t *ops,
                          const uint64_t *ops_off, const uint8_t *tmpl_bases, const uint64_t *tmpl_off, double thr, uint8_t *diverged,
                          uint64_t *chunk_err_off, size_t slot_cap, uint8_t *keep, uint64_t *cluster_out, uint8_t *touched,
                          uint8_t *post_keep, uint64_t *purged, size_t purged_cap, size_t *n_purged, double *read_err,
                          double *chunk_err, double *median_of_sqrt_err, int device);

/* ---- correct_deletion's candidate search: the skeleton pile-up -------------------------------------------------------
 * `ds.correct_deletion(..)` runs three times per pipeline run (cli/src/pipeline.rs:149,166,168).  In each of its up to 3 x 12
 * rounds `correct_deletion_error` (encode/deletion_fill.rs:301-337) calls get_pileup (deletion_fill.rs:642-698) for every live
 * read: the read's node skeleton against EVERY read's skeleton -- check_alignment_by_chunkmatch (:611-637),
 * pairwise_alignment_gotoh (:738-827), the verdict of `alignment` (:707-725), the walk into per-slot insertion lists -- then
 * mean_cov and ins_thr (:312-314) and check_insertion_head / _tail (:883-981), whose candidates try_encoding_head / _tail test
 * against the sequence.  This call returns those candidates, all integers, bit for bit.  What follows a candidate stays the
 * caller's: the failed-trial filter (:318,:328), remove_slippy_alignment, remove_overlapping_encoding; encode_node
 * (:451-566) is jtk_lc_encode_nodes below.
 *
 * Read r's nodes are nodes[node_off[r] .. node_off[r+1]) in read order.  The query set is every read, the target included;
 * `target` (NULL = every read) selects the reads that get output -- the reference's `is_alive` filter.  A read without nodes
 * or with target[r] == 0 keeps zero coverage, ins_thr 0 and no candidate.
 *   coverage[node_off[r] + r + slot]   Pileup.coverage of slot 0 ..= n of read r (slot n stays 0)
 *   ins_thr[r]                         min(mean_cov / 5, 2), mean_cov = sum(coverage) / (n + 1)
 *   cands[cand_off[r] .. cand_off[r+1]) sorted by (slot, side, chunk, cluster, is_forward): the keys whose entry count in the
 *                                      slot's head (side 0) or tail (side 1) list is >= ins_thr and which carry an offset;
 *                                      position = the value the reference's HashMap holds afterwards.  A head position is
 *                                      written signed: a negative one is what wraps to a huge usize in the reference, and
 *                                      `start_position < seq.len()` (:381) rejects it.
 * The reference's arm `position == pileups.len() - 1` (:669) reads the length of the shadowing iterator, i.e. what REMAINS:
 * it fires where 2 position + 1 == n, and at position == n the subtraction wraps (release build) and the general arm runs.
 * That is restated as it stands.
 * JTK_ERR_UNSUPPORTED: a read with more than 65,535 nodes.  JTK_ERR_INVALID_ARG with *n_cands = the need: cand_cap is too
 * small.  Nothing else is written on failure. */
typedef struct jtk_fill_node {      /* what ReadSkelton::from_rich_nodes reads of a Node (deletion_fill.rs:1003-1030) */
    uint64_t chunk, cluster;        /* Node.chunk, Node.cluster */
    uint32_t is_forward;            /* Node.is_forward */
    uint32_t query_len;             /* Node.query_length() */
    uint64_t position;              /* Node.position_from_start */
} jtk_fill_node_t;
typedef struct jtk_fill_cand {
    uint32_t read, slot;            /* slot idx of get_pileup's vector, 0 ..= n_nodes(read) */
    uint32_t side;                  /* 0 = check_insertion_head, 1 = check_insertion_tail */
    uint32_t is_forward;
    uint64_t chunk, cluster;        /* the LightNode key */
    uint32_t count, reserved;       /* entries of that key in the slot's list (what `threshold <= *num` saw) */
    int64_t  position;              /* the value the HashMap holds afterwards: start_position (head) / end_position (tail) */
} jtk_fill_cand_t;
JTK_LC_API int jtk_lc_fill_candidates(size_t n_reads, const uint64_t *node_off, const jtk_fill_node_t *nodes,
        const uint8_t *target /* NULL = every read; else 1 = compute this read (the reference's `is_alive` filter) */,
        uint32_t *coverage /* node_off[n_reads] + n_reads entries; read r's slots start at node_off[r] + r */,
        uint32_t *ins_thr /* n_reads */, uint64_t *cand_off /* n_reads + 1 */, jtk_fill_cand_t *cands, size_t cand_cap,
        size_t *n_cands, int device);

/* ---- banded affine-gap alignment along a guide path --------------------------------------------------------------
 * What the reference gets from kiley::bialignment::guided (`global_guided`, `infix_guided`): an alignment that already
 * exists (an edlib alignment of jtk_lc_align_reads*, an earlier pass of this call) is refined under affine gap scores inside
 * a band of `radius` cells around its path.  Call sites: encode/deletion_fill.rs:526,553-554 (infix, radius = band, scores
 * (2, -6, -5, -1)), determine_chunks.rs:538, consensus/mod.rs:560,1231-1233,1259-1261 (global); dense_encoding.rs:757 (global)
 * is jtk_lc_encode_edges below.
 * kiley is not part of the reference tree: the aligner follows THIS build's specification, DESIGN.md section 4 ("Guided
 * alignment"), and parity with kiley's band shape and its choice among equally good alignments is NOT pinned.  In short:
 * the guide is walked from (0, 0) (ops that do not fit are skipped, a short guide goes on diagonally, then by Del, then by
 * Ins); row i of the band holds the columns within `radius` of the path's columns in that row; three states M, D, I per cell,
 * a gap of length L costs gap_open + (L - 1) gap_ext; ties go to the first of M, D, I, in the end cell and at every step
 * back.  mode = JTK_ALIGN_INFIX frees both ends of x: M(i, 0) = 0 in every row the band reaches, the end is the best
 * (i, |y|), the smallest i on a tie, and the walk back stops the first time it is in M at column 0.
 * A pair indexes two base buffers and one op buffer, so that many pairs can share a sequence:
 *   x      the sequence whose ends may be free; Del (3) consumes an x base
 *   y      the sequence that is consumed whole; Ins (2) consumes a y base
 * Output per pair: score_out, the stretch [start_out, end_out) of x that was aligned (global: 0, x_len), status, and the ops at
 * ops_out[ops_out_off[p] .. ops_out_off[p+1]) (capacity ops_cap bytes; sum(x_len + y_len) is always enough).  The ops of
 * either mode consume both sequences whole -- infix: start x Del, the path, (x_len - end) x Del -- Match and Mismatch are
 * told apart, and the score leaves the free runs out.  Empty sequences are valid input.
 * JTK_ERR_INVALID_ARG: a base that is not ACGT, a guide op above 3, a mode other than GLOBAL / INFIX, scores outside
 * gap_open <= gap_ext <= 0, mismatch <= 0 <= match, or one above JTK_GUIDED_MAX_SCORE in magnitude (the table is 32-bit).
 * Limits, per pair (status[p] = JTK_ERR_UNSUPPORTED, no ops, the rest of the batch is aligned and the call returns
 * JTK_ERR_CHUNK_FAILED): 32,000 bases per sequence, and JTK_GUIDED_MAX_WIDTH cells in one row of the band (2 radius + 1 plus
 * the columns the path itself spans in that row). */
#define JTK_GUIDED_MAX_WIDTH 4096
#define JTK_GUIDED_MAX_SCORE 1024
typedef struct jtk_guided_pair {
    uint64_t x_off, y_off;          /* first base in x_bases / y_bases */
    uint64_t guide_off;             /* first op in guide_ops */
    uint32_t x_len, y_len, guide_len;
    uint32_t radius;
} jtk_guided_pair_t;
JTK_LC_API int jtk_lc_align_guided(size_t n_pairs, const jtk_guided_pair_t *pairs, const uint8_t *x_bases, const uint8_t *y_bases,
                        const uint8_t *guide_ops, int mode, int match, int mismatch, int gap_open, int gap_ext,
                        uint8_t *ops_out, uint64_t *ops_out_off, uint64_t ops_cap, int32_t *score_out, uint32_t *start_out,
                        uint32_t *end_out, int32_t *status, int device);

/* ---- correct_deletion's trial of a candidate: encode_node, batched ------------------------------------------------------
 * `encode_node` with `fine_mapping` and `fit_query_by_edlib` (encode/deletion_fill.rs:451-566) for a batch of trials, as it
 * stands.  Trial t lays the consensus cons_bases[cons_off .. + cons_len) of a (chunk, cluster) into the window
 * read_bases[read_off + start .. read_off + end) of a raw read (reverse-complemented when is_forward == 0, upper-cased), and
 * then the chunk's own sequence chunk_bases[chunk_off .. + chunk_len) onto what is left of the window:
 *   1. sim_thr < (cons_len -. (end - start)) / cons_len in f64 (:461-465, saturating subtraction): verdict 1, nothing else runs;
 *   2. the edlib infix alignment of the consensus into the window (jtk_lc_align_reads_mode), padded at both ends with ops
 *      that consume the window (:546-550); band = max(ceil(window_len * sim_thr * 0.3), 10) (:552);
 *   3. two passes of jtk_lc_align_guided's infix aligner, x = window, y = consensus, scores (2, -6, -5, -1) (:553-554);
 *   4. Ins and Del swapped, the window-consuming runs at both ends trimmed (:556-564): trim_head, trim_tail, and the query
 *      = window[trim_head .. window_len - trim_tail);
 *   5. mat_num, ops_len and edge_identity's four counts with EDGE_LEN = 100 (:501-503, :568-592);
 *   6. the third pass, infix, x = the chunk's sequence, y = the query, the same band (:526): its score and ops are the node's;
 *   7. verdict 0 when 1 - sim_thr < mat_num / ops_len && 0.5 < min(head_match / head_len, tail_match / tail_len), else 2
 *      (:504-505; f64: a 0 / 0 identity is NaN and rejects, and f64::min hands back the other operand where one edge is NaN).
 *      The reference runs 6 only for verdict 0; here it runs for every trial that passed 1 and the host applies 7 afterwards.
 * The guided passes follow this build's specification (see jtk_lc_align_guided): parity with kiley is NOT pinned.
 * result[t]: status (0; JTK_ERR_UNSUPPORTED where the infix alignment or a guided pass refuses the trial -- verdict is then 2 and
 * the call returns JTK_ERR_CHUNK_FAILED after finishing the rest), verdict, trim_head, trim_tail, position_from_start = start +
 * (is_forward ? trim_head : trim_tail) (:477-480), query_len, band, score and the counts; the third pass's ops at
 * ops_out[ops_out_off[t] .. ops_out_off[t+1]) (sum(chunk_len + end - start) bytes are always enough).  The caller runs
 * kiley_op_to_ops on them, takes `seq` from the window and keeps max_by_key(score) over a slot's accepted trials.
 * JTK_ERR_INVALID_ARG: start >= end (the reference asserts), an empty consensus or chunk sequence, a base that is not ACGT after
 * upper-casing. */
typedef struct jtk_encode_trial {
    uint64_t read_off;              /* the read's first base in read_bases */
    uint32_t start, end;            /* the window, in bases of the read */
    uint32_t is_forward;
    uint32_t cons_len;
    uint64_t cons_off;              /* into cons_bases */
    uint64_t chunk_off;             /* into chunk_bases: Chunk.seq() */
    uint32_t chunk_len;
    uint32_t reserved;
    double sim_thr;                 /* error_rate_bound (:400, :442) */
} jtk_encode_trial_t;
enum jtk_encode_verdict { JTK_ENCODE_ACCEPTED = 0, JTK_ENCODE_LOWER_BOUND = 1, JTK_ENCODE_REJECTED = 2 };
typedef struct jtk_encode_result {
    int32_t status;
    uint32_t verdict;
    uint32_t trim_head, trim_tail;
    uint64_t position_from_start;
    uint32_t query_len, band;
    int32_t score;
    uint32_t mat_num, ops_len;      /* of the fitted ops (step 5) */
    uint32_t head_match, head_len, tail_match, tail_len;
    uint32_t reserved;
} jtk_encode_result_t;
JTK_LC_API int jtk_lc_encode_nodes(size_t n_trials, const jtk_encode_trial_t *trials, const uint8_t *read_bases,
                        const uint8_t *cons_bases, const uint8_t *chunk_bases, jtk_encode_result_t *result, uint8_t *ops_out,
                        uint64_t *ops_out_off, uint64_t ops_cap, int device);

/* ---- dense_encoding's trial of an edge or a tip: encode_edge, batched ---------------------------------------------------
 * `encode_edge` with `tune_position` (dense_encoding.rs:627-759), which `fill_edges_by_new_chunks` (:202-293) calls for every
 * read and every gap or tip on a polyploid edge, for a batch of trials, as it stands.  Trial t lays the contig
 * contig_bases[contig_off .. + contig_len) -- merge_chunks' concatenation of the edge's new chunks (:595-609), whose chunk k
 * ends at break_points[break_first + k] -- onto the window read_bases[read_off + start .. read_off + end) of a raw read
 * (reverse-complemented when is_forward == 0, upper-cased) and cuts the alignment at the break points into one node per chunk:
 *   1. the infix alignment of the contig into the window, the window free (jtk_lc_align_reads_mode; :731): [seq_start, seq_end)
 *      of the oriented window, to which the window is truncated.  In the read's coordinates that is (start + seq_start,
 *      start + seq_end) forward and (end - seq_end, end - seq_start) reverse (:741-744);
 *   2. the infix alignment of the truncated window into the contig, the contig free (:746-755): [ctg_start, ctg_end) and the guide;
 *   3. one global pass of jtk_lc_align_guided's aligner, x = contig[ctg_start .. ctg_end), y = the truncated window, `radius`
 *      (read_type.band_width(contig_len)), scores (2, -6, -5, -1) (:756-757): `score`;
 *   4. the cut (:640-692).  The op stream is (ctg_start - the break point below it) Dels, the pass's ops without their leading Ins
 *      run (head_ins, where ypos starts), (contig_len - ctg_end) Dels.  first_chunk = the first k with ctg_start < break point k
 *      (n_chunks when there is none); the chunks below it are not reached.  The op that brings xpos to break point k closes chunk
 *      k; the Ins behind it belong to chunk k + 1, and what follows the last chunk's closing op is dropped.  Per closed chunk:
 *      ops_len, mat_num = the Matches among them, query_len = the ops that are no Del, query_off = seq_start + ypos - query_len
 *      (the node's seq inside the ORIENTED window), position_from_start = start + query_off forward, (end - seq_start) - ypos
 *      reverse (:674-677), and the ops themselves, virtual Dels included;
 *   5. verdict 0 when 1 - sim_thr < mat_num / ops_len in f64 (:671), else 2; 3 for a chunk that is not reached (all else 0).
 * Trial t's chunk k is nodes[node_off[t] + k] and its ops ops_out[ops_out_off[node_off[t] + k] .. ops_out_off[node_off[t] + k + 1])
 * (ops_out_off holds node_off[n_trials] + 1 entries), in chunk order.  The caller takes `seq` from the oriented window, runs
 * kiley_op_to_ops on the ops, and reverses a reverse trial's accepted nodes (:693-695).
 * This build's own decisions: both infix alignments and the guided pass follow DESIGN.md section 4 -- parity with edlib's choice
 * among equal placements and with kiley is NOT pinned.  A truncated window of length 0 (the reference would hand edlib an empty
 * sequence) or ctg_start == contig_len gives status 0 and every chunk not reached; with the empty window no pass runs and
 * ctg_start = ctg_end = score = 0.  There is no limit on n_chunks other than memory.
 * Limits, per trial (status = JTK_ERR_UNSUPPORTED where an infix alignment or the guided pass refuses it: every chunk not
 * reached, no ops, the rest of the batch is answered and the call returns JTK_ERR_CHUNK_FAILED): 32,000 bases per sequence,
 * contig_len + window length < 32,768 (the infix alignments run without a distance bound), JTK_GUIDED_MAX_WIDTH cells in a row
 * of the band.
 * JTK_ERR_INVALID_ARG, before a device is looked for: start >= end (the reference asserts), n_chunks == 0, an empty contig,
 * break points that do not ascend strictly from above 0 or do not end at contig_len, node_off that is not the prefix sum of
 * n_chunks, a base that is not ACGT (the window's after upper-casing), ops_cap below sum(contig_len + end - start) -- which
 * always holds the batch's ops, and is asked for whatever they come to, so that the answer does not depend on the data. */
typedef struct jtk_edge_trial {
    uint64_t read_off;              /* the read's first base in read_bases */
    uint32_t start, end;            /* the window, in bases of the read */
    uint32_t is_forward;
    uint32_t radius;                /* read_type.band_width(contig_len) (:637) */
    uint64_t contig_off;            /* into contig_bases */
    uint32_t contig_len;
    uint32_t n_chunks;
    uint64_t break_first;           /* into break_points: n_chunks strictly ascending ends, the last == contig_len */
    double sim_thr;                 /* read_type.sim_thr() (:658) */
} jtk_edge_trial_t;
enum jtk_edge_verdict { JTK_EDGE_ACCEPTED = 0, JTK_EDGE_REJECTED = 2, JTK_EDGE_NOT_REACHED = 3 };
typedef struct jtk_edge_result {
    int32_t status;
    int32_t score;                  /* of the guided pass */
    uint32_t seq_start, seq_end;    /* inside the oriented window, end exclusive */
    uint32_t ctg_start, ctg_end;    /* end exclusive */
    uint32_t first_chunk;           /* n_chunks when no chunk is reached */
    uint32_t head_ins;              /* remove_leading_insertions (:655) */
} jtk_edge_result_t;
typedef struct jtk_edge_node {
    uint32_t verdict;               /* enum jtk_edge_verdict */
    uint32_t mat_num, ops_len;      /* alignment_identity's two integers (:622-625) */
    uint32_t query_off, query_len;  /* the node's seq inside the oriented window */
    uint32_t reserved;
    uint64_t position_from_start;
} jtk_edge_node_t;
JTK_LC_API int jtk_lc_encode_edges(size_t n_trials, const jtk_edge_trial_t *trials, const uint8_t *read_bases,
                        const uint8_t *contig_bases, const uint32_t *break_points, const uint64_t *node_off,
                        jtk_edge_result_t *result, jtk_edge_node_t *nodes, uint8_t *ops_out, uint64_t *ops_out_off,
                        uint64_t ops_cap, int device);

/* ---- correct_deletion's list surgery: node statistics and the settle step --------------------------------------------------
 * What `correct_deletion_error` does to a read's nodes once the trials are in (encode/deletion_fill.rs:349-361), what
 * `re_encode_read` (determine_chunks.rs:548-562) and dense_encoding.rs do after their own appends, and the per-node numbers
 * `purge_large_deletion_nodes` (purge_diverged.rs:73-88) reads.  Read r's nodes are nodes[node_off[r] .. node_off[r+1]) in the
 * order the caller holds them (new nodes appended); node e's cigar is given per base, ops[ops_off[e] .. ops_off[e+1]), Match and
 * Mismatch both standing for a cigar Match.
 * stats[e], for every node of every mode:
 *   total    the ops; indel = the Ins and Del among them (remove_overlapping_encoding's identity is 1.0 - indel / total in f64)
 *   score    (Match + Mismatch) - (Ins + Del): remove_slippy_alignment::score (encode/mod.rs:289-297)
 *   del_size misc::max_region (misc.rs:345-358) over the run-length cigar with -l for a Match run and 2 l for an Ins or Del run,
 *            divided by 2 toward zero (purge_diverged.rs:75-80).  On the per-base ops that is the largest sum of a non-empty
 *            range of (-1, +2) weights where the node has an indel, and -(total) / 2 where it has none (one Match run).
 * mode JTK_SETTLE_STATS_ONLY stops there (keep = 1, order = 0 .. n - 1, n_kept = n).  The other two run, per read:
 *   (a) a stable sort by (chunk, position_from_start) -- JTK_SETTLE_BY_CHUNK_POS, deletion_fill.rs:354 -- or by chunk alone --
 *       JTK_SETTLE_BY_CHUNK, determine_chunks.rs:555, encode/mod.rs:134;
 *   (b) remove_slippy_alignment (encode/mod.rs:288-313): `prev` gives way to a node of the same chunk and direction that is not
 *       disjoint from it (prev.position + prev.query_len < node.position is disjoint) and scores higher; a node that scores
 *       no higher is dropped;
 *   (c) a stable sort by position_from_start;  (d) remove_slippy_alignment again;
 *   (e) remove_overlapping_encoding (encode/mod.rs:248-286): of the first adjacent pair in which one node strictly contains the
 *       other (a.start <= b.start && b.end < a.end, end = start + query_len) the one of lower identity goes, the later one on
 *       a tie, until no such pair is left.
 * order[node_off[r] + k], k < n_kept[r]: the index inside read r of the k-th surviving node; the entries behind them are
 * UINT32_MAX.  keep[e] = 1 for a survivor.  The caller rebuilds the read from them (encode::nodes_to_encoded_read).
 * A read without nodes has n_kept 0 (the reference never settles one).  A read with a node that has no ops, or whose ops take a
 * number of read bases (Match, Mismatch, Ins) other than query_len, gets read_status[r] = JTK_ERR_UNSUPPORTED, or
 * JTK_ERR_INVALID_ARG for an op above 3: its nodes are left as they came (keep 1, order 0 .. n - 1), the other reads finish and
 * the call returns JTK_ERR_CHUNK_FAILED.  JTK_ERR_INVALID_ARG: offsets that do not start at 0 or decrease, an unknown mode, a
 * null pointer.  JTK_ERR_UNSUPPORTED: 2^32 - 1 nodes or more, a node of 2^31 ops or more. */
enum jtk_settle_mode { JTK_SETTLE_STATS_ONLY = 0, JTK_SETTLE_BY_CHUNK_POS = 1, JTK_SETTLE_BY_CHUNK = 2 };
typedef struct jtk_settle_node {
    uint64_t chunk;                 /* Node.chunk */
    uint64_t position_from_start;   /* Node.position_from_start */
    uint32_t is_forward;            /* Node.is_forward */
    uint32_t query_len;             /* Node.query_length() */
} jtk_settle_node_t;
typedef struct jtk_node_stats {
    int32_t score;
    uint32_t total;
    uint32_t indel;
    int64_t del_size;
} jtk_node_stats_t;
JTK_LC_API int jtk_lc_settle_nodes(size_t n_reads, const uint64_t *node_off, const jtk_settle_node_t *nodes, const uint8_t *ops,
                        const uint64_t *ops_off, int mode, jtk_node_stats_t *stats, uint32_t *n_kept, uint32_t *order,
                        uint8_t *keep, int32_t *read_status, int device);

/* ---- repeat masking: canonical k-mer counts over the raw reads -------------------------------------------------------------
 * `ds.mask_repeat` (repeat_masking.rs:135-158, the first thing cli/src/pipeline.rs:146 does to a data set) and its read-side
 * counterpart, get_repetitive_kmer (:109-134) and RepeatAnnot::repetitiveness (:90-105).  Sequences are given as everywhere
 * else, back to back with n + 1 offsets, but ANY byte is taken: the reference's tables code A C G T as 0 1 2 3 (forward) and
 * 3 2 1 0 (complement) in either case and EVERY OTHER BYTE AS 0 IN BOTH, so a run of N counts as the k-mer of a run of A, and
 * the reverse strand of a window that holds such a byte is not the complement of its forward strand.  The k-mer of a window is
 * min(forward, reverse): the forward strand has base i at bits 2i, the reverse strand the last base's complement at bits 0..1
 * (KMers, to_idx: :39-85, :196-208); a sequence shorter than k has none.  1 <= k <= 31 (pipeline.rs:83 asserts k < 32).
 *
 * jtk_lc_mask_repeats: every read is upper-cased (letters only), the k-mers of all reads are counted, and create_mask
 * (:255-285) chooses: with M the distinct k-mers counted more than once, percentile = floor(M as f64 * (1.0 - freq)) and
 * below_min = those of them counted <= min_count, the mask is all M of them where percentile < below_min (takes_all = 1,
 * thr = 0); otherwise thr = the count at index percentile of the M counts in ascending order and the mask is the k-mers counted
 * MORE than thr times.  A base j of a read then becomes lower case iff a masked k-mer starts in [j - k + 1, j] (mask_repeats,
 * :287-325).  masked receives the reads (it may be `bases` itself); mask_kmers the mask, ascending, if mask_cap holds it
 * (NULL with mask_cap = 0: the list is not asked for).  report: the bases, the k-mers (windows), the distinct k-mers, those counted once, the
 * mask's size, the lower-case bases (the reference's MASKREPEAT debug rows), thr and takes_all.
 * JTK_ERR_CHUNK_FAILED where the reference's counts[percentile] panics -- M = 0 (no reads, no k-mer, none counted twice), or
 * freq so small that 1.0 - freq == 1.0: the report's counts are filled in (thr, takes_all, n_masked_kmers, n_lower are 0) and
 * masked holds the upper-cased reads.  JTK_ERR_INVALID_ARG with report->n_masked_kmers = the need, and everything else valid,
 * when mask_cap is too small (the convention of jtk_lc_fill_candidates).
 *
 * jtk_lc_repetitive_kmers: the k-mers of every window of the reads AS GIVEN whose k bytes are all ASCII lower case (a lower-case
 * letter that is no base codes as 0), ascending and unique; *n_kmers = their number, also where cap is too small
 * (JTK_ERR_INVALID_ARG, nothing written to kmers).
 *
 * jtk_lc_repetitiveness: for every sequence, rep_num = the sum, over the k-mers of `kmers` that occur in it more than once,
 * of their occurrences, and rep_den = max(len, k) - k + 1 (1 for a sequence shorter than k); the reference's f64 is
 * rep_num / rep_den.  kmers must be ascending and unique (checked on the device: JTK_ERR_INVALID_ARG).
 *
 * All three, before a device is looked for: JTK_ERR_INVALID_ARG for a null pointer, offsets that do not start at 0 or decrease,
 * k = 0, freq NaN or outside [0, 1]; JTK_ERR_UNSUPPORTED for k >= 32, 2^32 bases or sequences or more (a count must fit the
 * reference's u32), and where the index of a sequence does not fit above the k-mer in 64 bits.  JTK_ERR_ALLOC, with the size in
 * the message, for a work area (the keys twice, the sort's block, the runs) above 80 % of the device's free memory. */
typedef struct jtk_mask_report {
    uint64_t n_bases, n_kmers, n_distinct, n_singleton, n_masked_kmers, n_lower;
    uint32_t thr, takes_all;
} jtk_mask_report_t;
JTK_LC_API int jtk_lc_mask_repeats(size_t n_reads, const uint8_t *bases, const uint64_t *read_off, uint32_t k, double freq,
                        uint32_t min_count, uint8_t *masked, uint64_t *mask_kmers, uint64_t mask_cap, jtk_mask_report_t *report,
                        int device);
JTK_LC_API int jtk_lc_repetitive_kmers(size_t n_reads, const uint8_t *bases, const uint64_t *read_off, uint32_t k, uint64_t *kmers,
                        uint64_t cap, uint64_t *n_kmers, int device);
JTK_LC_API int jtk_lc_repetitiveness(size_t n_seqs, const uint8_t *bases, const uint64_t *seq_off, uint32_t k, const uint64_t *kmers,
                        uint64_t n_kmers, uint32_t *rep_num, uint32_t *rep_den, int device);

/* ---- mapping: minimizer seeding and chaining of reads onto chunks -----------------------------------------------------------
 * What the reference gets from an external minimap2 process (encode/mod.rs:41-64 and :315-355, minimap2.rs; determine_chunks.rs
 * through `self.encode` and `remove_overlapping_chunks`): WHERE in a read a chunk lies.  minimap2 is not part of the reference
 * tree: the mapper follows THIS build's specification, DESIGN.md section 4 ("Seeding and chaining"), and parity with minimap2's
 * choice of seeds and chains is NOT pinned.  In short: canonical k-mers (bases upper-cased on the fly; one that holds a byte that
 * is no base, or equals its own reverse complement, is invalid), an invertible hash of the 2k bits, minimizers over windows of w
 * k-mer positions with EVERY position that attains a window's minimum kept, an index of the targets' minimizers in which a hash
 * that occurs more than max_occ times is not used, hits with diag = q' - tpos on the oriented query, clusters by single linkage
 * along the diagonal (a gap above max_gap, or another target or strand, starts a new one), and a placement for every cluster
 * with at least min_seeds distinct target positions.  skip_self: query i against target i yields nothing (minimap2's -X).
 * A placement is a seed cluster, not an alignment: jtk_lc_encode_nodes decides whether the chunk is there.
 *
 * jtk_lc_map_reads: placements in the order (query, target, reverse after forward, diag_lo).  JTK_ERR_INVALID_ARG with
 * *n_placements = the need and nothing else written when cap is too small (the convention of jtk_lc_fill_candidates).
 * jtk_lc_sketch: the minimizers alone, ascending by (seq, pos); hash, seq, pos, strand are parallel arrays of cap entries;
 * JTK_ERR_INVALID_ARG with *n = the need when cap is too small.
 *
 * Both, before a device is looked for: JTK_ERR_INVALID_ARG for a null pointer, offsets that do not start at 0 or decrease,
 * k = 0, w = 0 or min_seeds = 0; JTK_ERR_UNSUPPORTED for k >= 32, w > 64, a target above 65,535 bases, a query above 4,000,000
 * bases (jtk_lc_sketch: a sequence of 2^31 bases or more), more than 2^25 targets, 2^32 bases or sequences or more on either
 * side.  After the hits are counted: JTK_ERR_UNSUPPORTED for 2^32 hits or more, JTK_ERR_ALLOC, with the size in the message,
 * for a hit buffer above 80 % of the device's free memory. */
typedef struct jtk_map_params { uint32_t k, w, max_occ, max_gap, min_seeds, skip_self; } jtk_map_params_t;
typedef struct jtk_map_placement {
    uint32_t query, target, is_forward, n_seeds;
    uint32_t qstart, qend;          /* forward-strand query coordinates, as a PAF line has them */
    uint32_t oq_start, oq_end;      /* on the oriented query */
    uint32_t tstart, tend;
    int32_t  diag_lo, diag_hi;
} jtk_map_placement_t;
JTK_LC_API int jtk_lc_map_reads(size_t n_targets, const uint8_t *target_bases, const uint64_t *target_off, size_t n_queries,
                        const uint8_t *query_bases, const uint64_t *query_off, const jtk_map_params_t *params,
                        jtk_map_placement_t *out, uint64_t cap, uint64_t *n_placements, int device);
JTK_LC_API int jtk_lc_sketch(size_t n_seqs, const uint8_t *bases, const uint64_t *seq_off, uint32_t k, uint32_t w, uint64_t *hash,
                        uint32_t *seq, uint32_t *pos, uint8_t *strand, uint64_t cap, uint64_t *n, int device);

/* ---- consensus polishing that votes with banded edit distances -----------------------------------------------------------
 * What the reference gets from kiley::bialignment::guided::polish_until_converge / polish_until_converge_with:
 * `take_consensus_sequence` (encode/deletion_fill.rs:260-285, whose output is the cons_bases of jtk_lc_encode_nodes),
 * `polish_chunk` (polish_chunks.rs:64-65), the refresh of `polish_seg` (consensus/mod.rs:442,470-472), determine_chunks.rs:439
 * and dense_encoding.rs:575-577.  kiley is not part of the reference tree: the polish follows THIS build's specification,
 * DESIGN.md section 4 ("Guided polishing"), and parity with kiley's polish is NOT pinned.  In short, per pile-up and round t:
 * every read is aligned to the template at unit costs inside the band of jtk_lc_align_guided around its current ops (walk back:
 * diagonal, then Del, then Ins; these ops replace the read's); the first take_num reads (0 = all) vote with the 14-row table of
 * jtk_lc_modification_table's layout, T[p][row] = the banded distance of the read to the edited template, gain = the sum over
 * the voters of dist - T; the scan of jtk_lc_polish_chunks applies the first best row of a position where its gain is >= 1 and
 * no voter finds the entry outside its band; edits are applied, every read's ops re-threaded, and the next round begins.  A
 * round that applies nothing is the last; so is round max_rounds (0 = 20), after which the reads are aligned once more, so
 * that the ops and distances returned always belong to the consensus returned.
 * chunks / tmpl_bases / read_bases / read_off / ops / ops_off, cons_out / ops_out and their capacities, and the read-layout
 * precondition are those of jtk_lc_polish_chunks; copy_num, chunk_id and strands play no part.  radius[c] is pile-up c's band
 * radius; dist_out[r] the edit distance of read r inside its band; result[c].status and .polish_rounds are filled (rounds
 * count the one that applied nothing).  A pile-up without reads returns its template after one round; one with
 * 2 ignore_edge >= tmpl_len is not scanned (one round) and only has its reads aligned.
 * JTK_ERR_INVALID_ARG, before a device is looked for: a base that is not ACGT, an op above 3, a radius of 0, a null pointer.
 * Limits, per pile-up (result[c].status = JTK_ERR_UNSUPPORTED, empty consensus and ops, dist_out = UINT32_MAX, the rest of the
 * batch is polished and the call returns JTK_ERR_CHUNK_FAILED): 32,000 bases per sequence and JTK_GUIDED_MAX_WIDTH cells in
 * one row of a band; a consensus that outgrows tmpl_len + 64 + tmpl_len / 8 bases fails its pile-up the same way with
 * JTK_ERR_CHUNK_FAILED. */
JTK_LC_API int jtk_lc_polish_guided(size_t n_chunks, const jtk_lc_chunk_t *chunks, const uint8_t *tmpl_bases,
                         const uint8_t *read_bases, const uint64_t *read_off, const uint8_t *ops, const uint64_t *ops_off,
                         const uint32_t *radius /* per chunk */, uint32_t take_num, uint32_t ignore_edge, uint32_t max_rounds,
                         uint8_t *cons_out, uint64_t *cons_off, uint64_t cons_cap, uint8_t *ops_out, uint64_t *ops_out_off,
                         uint64_t ops_cap, uint32_t *dist_out /* per read */, jtk_lc_result_t *result, int device);

/* Sort key of pileup_nodes (mod.rs:47-50): number of alignment columns that are not '|' in
 * Node::recover (definitions/src/lib.rs:773-813) for run-length cigar ops given per base. */
JTK_LC_API int jtk_lc_pileup_sort_key(const uint8_t *tmpl, uint64_t tmpl_len, const uint8_t *read, uint64_t read_len,
                           const uint8_t *ops, uint64_t ops_len, uint64_t *key_out);

/* normalize_local_clustering for one pile-up (normalize.rs:21-50): relabels by descending cluster size
 * (ties: larger old index first) and permutes each posterior row in place. */
JTK_LC_API int jtk_lc_normalize_pileup(uint32_t n_reads, uint32_t cluster_num, uint32_t *label, double *log_post,
                            uint32_t post_stride);

/* Device workspaces of finished calls are kept for the next call of similar shape (up to JTK_LC_POOL_GB per device,
 * default 32; 0 disables the pool): mapping tens of GB for a 2500-chunk batch costs seconds otherwise.  This returns
 * them to the driver. */
JTK_LC_API int jtk_lc_trim_cache(int device);

JTK_LC_API const char *jtk_lc_strerror(int status);
/* Thread-local text of the last failure on this thread (HIP error strings etc.); "" if none.  The pointer is valid until
 * this thread's next call into the library: copy the text before calling anything else. */
JTK_LC_API const char *jtk_lc_last_error(void);
JTK_LC_API int jtk_lc_version(void);
/* 1 if a gfx950 device `device` is present and the kernels for it are loaded. */
JTK_LC_API int jtk_lc_device_ok(int device);

/* Timing of the last jtk_lc_cluster_* call on this thread, measured with HIP events on the library's
 * own stream: total device milliseconds and the milliseconds + launch count of each kernel family
 * (index = enum jtk_kernel_id).  Used by bench.py for the live roofline number.
 * The figures come from event pairs on the session's stream.  Sessions that share a lane (more sessions on a device than
 * its hardware queues pay for streams: INTEGRATION.md section 4) share that stream, and a family's figure then includes
 * whatever kernels of the lane's other sessions ran in between; kernel_ms[JTK_K_MCMC] is the merged chain launch that
 * carried the session's chunks, plus the wait for the sessions it was gathered with.
 * A session that shared a merged chain launch with lane-mates does not wait for the launch's end but for its own chunks
 * ("Leaving a merged chain launch"), and HIP gives no elapsed time for an event that has not completed.
 * For such a pass total_ms and kernel_ms[JTK_K_MCMC] are host-clock figures: from the start of the call, and from the return of
 * the chain launch, to the moment the session saw its chunks done.  Every other figure stays an event pair, and a pass that
 * ended with its launch's event (a lane to itself, or the fallback) is timed by events throughout, as before. */
enum jtk_kernel_id { JTK_K_PHMM = 0, JTK_K_POLISH = 1, JTK_K_FILTER = 2, JTK_K_MCMC = 3, JTK_K_COUNT = 4 };
typedef struct jtk_lc_timing {
    double total_ms;
    double h2d_ms, d2h_ms;
    double kernel_ms[JTK_K_COUNT];
    uint32_t kernel_launches[JTK_K_COUNT];
    uint32_t chain_lds_bytes[2]; /* LDS work area per chain workgroup of the two launch classes (0: class not used); class 0
                                  * stays <= 80 KiB (two workgroups per CU), class 1 <= 160 KiB */
} jtk_lc_timing_t;
JTK_LC_API int jtk_lc_last_timing(jtk_lc_timing_t *out);

#ifdef __cplusplus
}
#endif
#endif /* JTK_LC_H */
