/* jtk_lc_debug.h -- diagnostic entry points of libjtk_lc.so.  NOT part of the drop-in boundary (include/jtk_lc.h): nothing a
 * jtk host needs is declared here.  They exist so that a test can look at an intermediate the boundary does not return
 * (tests/test_gpu_correction.py compares the device-filled similarity matrix of phmm_likelihood_correction.rs:272-285 bit for
 * bit with the oracle's).  Same library, same build: there is no separate test build of the product. */
#ifndef JTK_LC_DEBUG_H
#define JTK_LC_DEBUG_H

#include "jtk_lc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Keep (on != 0) the raw similarity matrix of the first corrected chunk of the following jtk_lc_correct_clustering calls on
 * this thread. */
JTK_LC_API void jtk_lc_debug_cc_keep_sims(int on);
/* Copy up to `cap` doubles of the kept matrix into `out`; returns its size. */
JTK_LC_API size_t jtk_lc_debug_cc_first_sims(double *out, size_t cap);
/* While the switch above is on, the raw matrix (before filter_similarity) of EVERY corrected chunk of the last call is kept, in
 * the order the chunks are corrected (selected_chunks order) and across all device batches of the call: their number, and a copy
 * of up to `cap` doubles of matrix `job` (returns its size, 0 for a job that does not exist).  Nothing is kept while it is off. */
JTK_LC_API size_t jtk_lc_debug_cc_sims_count(void);
JTK_LC_API size_t jtk_lc_debug_cc_sims(size_t job, double *out, size_t cap);

/* Where the chain kernel's time went, per chunk of a session that has run: cycles[c] = shader-clock cycles the chunk's consumer
 * wave spent in the kernel (0 for a chunk without a variant column), events[c] = proposals of its table-driven chains that could
 * not be stepped over (accepted moves, rounding residues, draws inside the guard bands).  A chain launch lasts as long as its
 * slowest chunk: this is how bench.py names it.  Either pointer may be null. */
JTK_LC_API int jtk_lc_debug_chain_profile(jtk_lc_session_t *s, uint64_t *cycles, uint32_t *events);

/* HIP-event times of this thread's last jtk_lc_node_errors / jtk_lc_estimate_error_rate / jtk_lc_purge_diverged call, 4 doubles:
 * the upload of the sequences (allocation included) in ms, the column-walk kernel in ms, the whole call on its stream in ms
 * (upload to the last copy back), and the passes of the fit. */
JTK_LC_API void jtk_lc_debug_purge_timing(double *out);

/* The aligner of jtk_lc_fill_candidates by itself: for pair p = (pair_target[p], pair_query[p]) of reads given as for that call,
 * dir[p] = 1 forward, 0 reverse, -1 where check_alignment_by_chunkmatch rejects the pair or the target has no node (score and
 * pass are then 0 and the pair has no ops); score[p] = pairwise_alignment_gotoh's; pass[p] = `alignment` returns Some; and the
 * compressed ops at ops[ops_off[p] .. ops_off[p+1]) in alignment order, each len << 2 | code with code 0 = Match, 1 = Ins,
 * 2 = Del.  JTK_ERR_INVALID_ARG with *n_ops = the need when ops_cap is too small. */
JTK_LC_API int jtk_lc_debug_fill_pairs(size_t n_reads, const uint64_t *node_off, const jtk_fill_node_t *nodes, size_t n_pairs,
                                       const uint32_t *pair_target, const uint32_t *pair_query, int32_t *dir, int32_t *score, uint8_t *pass,
                                       uint64_t *ops_off, uint32_t *ops, size_t ops_cap, size_t *n_ops, int device);
/* Of this thread's last jtk_lc_fill_candidates call, 4 doubles: the pairs aligned, the insertion records, the HIP-event time of
 * the whole call on its stream in ms (upload to the last copy back) and of the pair kernels in ms. */
JTK_LC_API void jtk_lc_debug_fill_timing(double *out);

/* Of this thread's last jtk_lc_settle_nodes call, 4 doubles: the reads, the reads whose work area lay in global memory (more
 * nodes than the LDS slot of a wave holds), the HIP-event time of the kernel in ms, and of the whole call on its stream in ms
 * (upload to the last copy back). */
JTK_LC_API void jtk_lc_debug_settle_timing(double *out);

/* Of this thread's last jtk_lc_mask_repeats call, 4 doubles, HIP-event times in ms: the emit kernel; the sort of the keys; the
 * counting and the selections up to the mask (with the one wait for the host in it); the apply kernel. */
JTK_LC_API void jtk_lc_debug_mask_timing(double *out);

/* Of this thread's last jtk_lc_map_reads call, 10 doubles: HIP-event times in ms of the two sketches, of the index (sort, run
 * lengths, scan), of the hits (count, scan, the wait for the host, fill), of the ordering sort, of the chaining (flags, scan,
 * reduction, the distinct target positions) and of the compaction (with its wait and the copy back); then two counts, the
 * minimizers of targets and queries together and the hits; then the ms of the two sketch kernels alone (the sketch phase also
 * holds the upload of the sequences and the wait for the minimizers' number), and a 0. */
JTK_LC_API void jtk_lc_debug_map_timing(double *out);

/* The work-area budget of jtk_lc_align_guided / jtk_lc_encode_nodes on this thread, in bytes (traceback cells and row tables
 * per slice of the batch; 0 = the default, 4 GiB): a small value makes a small batch run in several slices.  A pair that
 * alone needs more still runs, in a slice of its own. */
JTK_LC_API void jtk_lc_debug_guided_scratch_cap(uint64_t bytes);
/* Of this thread's last jtk_lc_align_guided call, 4 doubles: the pairs, the cells filled, the HIP-event time of its kernels in
 * ms, and the slices it ran in. */
JTK_LC_API void jtk_lc_debug_guided_timing(double *out);
/* Of this thread's last jtk_lc_encode_nodes call, 8 doubles: the trials that passed the lower-bound filter, the HIP-event time
 * in ms of the three guided passes [1..3] and the cells they filled [4..6], and the host clock of the infix alignment in ms. */
JTK_LC_API void jtk_lc_debug_encode_timing(double *out);
/* Of this thread's last jtk_lc_encode_edges call, 8 doubles: the trials, the HIP-event time in ms of the guided pass [1], the
 * cells it filled [2] and its slices [3], the host clock in ms of the two infix alignments [4], [5], and the HIP-event time in ms
 * of the cut and pack kernels [6]. */
JTK_LC_API void jtk_lc_debug_edges_timing(double *out);

/* One round's fill of jtk_lc_polish_guided for a single pile-up, nothing applied: dist_out[r] = the banded edit distance of
 * read r along its ops, and table_out[r * table_stride + p * 14 + row] = T[p][row] of DESIGN.md section 4 ("Guided polishing")
 * for p = 0 .. tmpl_len, UINT32_MAX for a dead entry; table_stride >= (tmpl_len + 1) * 14.  Unlike the polish it takes a radius
 * of 0 (the band is the guide's path). */
JTK_LC_API int jtk_lc_debug_guided_table(const uint8_t *tmpl, uint32_t tmpl_len, uint32_t n_reads, const uint8_t *read_bases,
                                         const uint64_t *read_off, const uint8_t *ops, const uint64_t *ops_off, uint32_t radius,
                                         uint32_t *dist_out, uint32_t *table_out, uint64_t table_stride, int device);
/* Of this thread's last jtk_lc_polish_guided call, 8 doubles: pile-ups, reads, rounds the host enqueued, band cells filled
 * forward (all passes), the HIP-event time of the rounds' kernels in ms, the slices of the work area, the bytes of work area
 * that all reads together take by the host's bound (F cells, row tables, rings), and the band cells of the voting reads'
 * fills (whose table reads F rows p .. p + 3 at every position p). */
JTK_LC_API void jtk_lc_debug_gpolish_timing(double *out);

/* Keep (on != 0) what the device batches of the following jtk_lc_estimate_gains / jtk_lc_estimate_minimum_gain calls on this thread
 * held: while the switch is on, the last such call keeps, per batch and in batch order, the template and read bytes with their
 * offsets, the ops and their lengths exactly as edit_ops_kernel wrote them (JTK_LC_DEBUG_GAINS_OPS_STRIDE bytes per pair, before the
 * host packs them) and the likelihood of every (template, read) pair.  Pair g of a batch scores read g against template
 * g / (pairs / templates).  A call that fails keeps the batches it finished.  Nothing is kept while it is off, and switching it
 * off drops what was kept. */
#define JTK_LC_DEBUG_GAINS_OPS_STRIDE 512
JTK_LC_API void jtk_lc_debug_gains_keep(int on);
JTK_LC_API size_t jtk_lc_debug_gains_batches(void);
/* sizes[0..3] of batch `batch`: its templates, template bytes, pairs and read bytes; JTK_ERR_INVALID_ARG for a batch that does not
 * exist */
JTK_LC_API int jtk_lc_debug_gains_batch_sizes(size_t batch, uint64_t *sizes);
/* Copy one batch out; a null pointer skips its part.  tmpl_off holds templates + 1 entries, read_off pairs + 1, ops pairs x
 * JTK_LC_DEBUG_GAINS_OPS_STRIDE bytes, ops_len and lk pairs entries. */
JTK_LC_API int jtk_lc_debug_gains_batch(size_t batch, uint8_t *tmpl, uint64_t *tmpl_off, uint8_t *reads, uint64_t *read_off,
                                        uint8_t *ops, uint32_t *ops_len, double *lk);

/* The lane of a session ("Lanes and the merged chain launch"): sessions of one lane share a stream and
 * gather their chain kernels into one launch.  Whether two sessions meet in a launch is otherwise a race between their host
 * threads; these three make it a test's choice and let the test read back what was launched.
 *
 * jtk_lc_debug_session_lane: the index of the session's lane in its device's table (JTK_ERR_INVALID_ARG for a null session).
 *
 * jtk_lc_debug_lane_hold(device, lane, 1) holds the lane: until the matching (device, lane, 0) every session that reaches its
 * chain point pends, none launches.  On release a pending session launches everything pending in arrival order, at most 8
 * sessions per launch.  Holds count; a lane that does not exist and a release without a hold are JTK_ERR_INVALID_ARG.  Sessions
 * that enter no gather (polish-only ones, the sub-sessions of the split branch) do not wait for a hold.
 *
 * jtk_lc_debug_lane_state: in_pass = sessions between the start of a pass and their chain point (holds not counted), holds,
 * pending = sessions at their chain point waiting for the launch, launch_calls = launches the lane has made so far (one call
 * carries up to 8 sessions), and the n_records = min(launch_calls, JTK_LC_DEBUG_LANE_RECORDS) most recent of them, oldest first.
 * Per chain class (0: work areas up to 80 KiB, 1: above) a call makes one merged launch with a segment for every carried
 * session that has chunks of the class: segments[j] of them (0 = no launch), chunks[j] workgroups in all, seg_chunks[j][i] in
 * segment i.  Read it while the lane is held or idle. */
#define JTK_LC_DEBUG_LANE_RECORDS 8
typedef struct jtk_lc_debug_lane_launch {
    uint32_t members;
    uint32_t segments[2];
    uint32_t chunks[2];
    uint32_t seg_chunks[2][8];
} jtk_lc_debug_lane_launch_t;
typedef struct jtk_lc_debug_lane_state {
    uint32_t in_pass, holds, pending, n_records;
    uint64_t launch_calls;
    jtk_lc_debug_lane_launch_t records[JTK_LC_DEBUG_LANE_RECORDS];
} jtk_lc_debug_lane_state_t;
JTK_LC_API int jtk_lc_debug_session_lane(jtk_lc_session_t *s);
JTK_LC_API int jtk_lc_debug_lane_hold(int device, int lane, int hold);
JTK_LC_API int jtk_lc_debug_lane_state(int device, int lane, jtk_lc_debug_lane_state_t *out);

/* The polish rounds of a lane ("Lanes and the merged round launch"): lane-mates that are in their polish
 * phase at the same time put their rounds into one launch per kernel.  A session parks at its lane's round gather wherever it
 * would queue a round -- the opening of its pass (reset + band preparation), then every polish round -- and the launch is made
 * once every session of the lane that is in its polish phase is parked.  Sessions that do not take part (pair items, wide reads,
 * per-read tables, jtk_lc_polish_chunks, the sub-sessions of the split branch, JTK_LC_MERGE_ROUNDS=0) never park and never
 * appear in the records.
 *
 * jtk_lc_debug_round_hold(device, lane, 1) holds the lane's round gather: until the matching (device, lane, 0) every arriving
 * session pends and nothing launches; after the release the launch is made as soon as every session in its polish phase is
 * parked, in arrival order, at most 8 sessions per call.  (device, lane, 2) is a step: the sessions parked at that moment get
 * their launch, whoever else is in its polish phase, and the hold stays -- so a test can put sessions of different rounds into
 * one launch.  Holds count.  A hold of the chain gather (jtk_lc_debug_lane_hold) does not stall rounds, and this one does not
 * stall chains of sessions that have left their polish phase.
 *
 * jtk_lc_debug_round_state: in_rounds = sessions in their polish phase, parked = those waiting for a launch, holds, launch_calls
 * = round launches the lane has made (one that carried a single session counts), and the n_records most recent, oldest first.  A record is
 * read back from the segment table the kernels were given: members = its segments (1 and merged = 0: a session on its own,
 * a table of one), and per member round[i] (JTK_LC_DEBUG_ROUND_OPEN: the opening), chunks[i], and phmm_items[i], its reads in
 * phmm_kernel's item space (0 at the opening). */
#define JTK_LC_DEBUG_ROUND_RECORDS 64
#define JTK_LC_DEBUG_ROUND_OPEN 0xffffffffu
typedef struct jtk_lc_debug_round_launch {
    uint32_t members, merged;
    uint32_t round[8];
    uint32_t chunks[8];
    uint32_t phmm_items[8];
} jtk_lc_debug_round_launch_t;
typedef struct jtk_lc_debug_round_state {
    uint32_t in_rounds, holds, parked, n_records;
    uint64_t launch_calls;
    jtk_lc_debug_round_launch_t records[JTK_LC_DEBUG_ROUND_RECORDS];
} jtk_lc_debug_round_state_t;
JTK_LC_API int jtk_lc_debug_round_hold(int device, int lane, int hold);
JTK_LC_API int jtk_lc_debug_round_state(int device, int lane, jtk_lc_debug_round_state_t *out);

/* How a session's passes ended ("Leaving a merged chain launch"): a session whose chains went out in a
 * merged launch of several lane-mates waits for a word that the chain kernels write when ITS chunks are done, with the launch's
 * end event as the fallback, and goes on while the launch still runs.  Host bookkeeping only; one record per pass
 * (jtk_lc_session_run), the last JTK_LC_DEBUG_PASS_RECORDS kept.
 *
 *   pass           the session's pass count, from 1
 *   how            JTK_LC_DEBUG_LEFT_BY_EVENT: waited for its launch's end event (every pass that shared no launch, and the
 *                  fallback); JTK_LC_DEBUG_LEFT_BY_WORD: left through its word; 0: the pass has not reached that point
 *   event_pending  hipEventQuery of the launch's end event said "not ready" at the moment the session left
 *   members        sessions the chain launch carried (1: its own launch)
 *   still_waiting  of those, the ones that had not left yet when this one did (0: the launch ended with this session)
 *   round_stream / next_round_stream
 *                  which of the lane's two streams (0: the first, 1: the side stream) carried this pass's rounds, and which
 *                  carries the session's fetch and next rounds after it left
 *   stamp_*        order stamps from one process-wide counter (larger = later; 0 = has not happened): the session left its
 *                  launch; jtk_lc_session_run returned; a jtk_lc_session_fetch after this pass returned; and, of THIS pass's
 *                  own rounds, the host saw round 0 complete (which the opening of the pass precedes on its stream).
 * jtk_lc_debug_session_passes copies the records of the last min(passes, cap, JTK_LC_DEBUG_PASS_RECORDS) passes, oldest first,
 * and returns their number (negative: a jtk_status). */
#define JTK_LC_DEBUG_PASS_RECORDS 4
#define JTK_LC_DEBUG_LEFT_BY_WORD 1
#define JTK_LC_DEBUG_LEFT_BY_EVENT 2
typedef struct jtk_lc_debug_pass {
    uint64_t pass;
    uint32_t how, event_pending, members, still_waiting, round_stream, next_round_stream;
    uint64_t stamp_left, stamp_returned, stamp_fetched, stamp_round0;
} jtk_lc_debug_pass_t;
JTK_LC_API int jtk_lc_debug_session_passes(jtk_lc_session_t *s, jtk_lc_debug_pass_t *out, size_t cap);

/* The variant filter of a clustering pass by itself ("The filter seam"): homop_kernel, chunk_tables_kernel,
 * the column filter and the pick, through the launch functions and on the batch layout of a session, from planted input
 * instead of a pair-HMM pass.  `chunks` / `tmpl_bases` / `strand` as for jtk_lc_session_create (copy_num <= 7); the reads have
 * no bases.  Read g of a chunk with template length L brings, back to back in read order,
 *   mode JTK_LC_DEBUG_FILTER_TABLE:      values: 14 (L + 1) doubles, its table minus its likelihood; exps and lk are not read.
 *                                        Runs the table filter (column_filter_kernel, pick_kernel<true>).
 *   mode JTK_LC_DEBUG_FILTER_ROWS_FUSED: values: 16 (L + 1) doubles of row sums, exps: L + 1 exponents, lk[g].  Runs the fused
 *                                        filter (column_filter_fused_kernel, pick_kernel<false>); JTK_ERR_INVALID_ARG for a
 *                                        chunk of more than 65,535 reads, as a session never takes it for one.
 *   mode JTK_LC_DEBUG_FILTER_ROWS_TABLE: the same input; finalize_kernel as a session's last pass calls it, then the table filter.
 * Out, per chunk c: cand[14 * tmpl_off_c + 14 * c ..] = the 14 (L + 1) scores of its columns, -1 for a column that is no
 * candidate (tmpl_off_c = the sum of the earlier chunks' L); dim[c]; pos[21 c ..] the picked columns in column order and
 * vtype[42 c ..] their (homopolymer length, difference type) pairs; feat[21 * read_first_c ..] = n_reads x dim[c] features, row
 * major; trace[66 c ..] = the pick again by pick_trace_kernel: candidates, picks, then the picked candidates' list indices in
 * pick order (zeros for a chunk of copy number < 2, which has no pick).  Arguments are checked, and refused, before a device is
 * looked for. */
#define JTK_LC_DEBUG_FILTER_TABLE 0
#define JTK_LC_DEBUG_FILTER_ROWS_FUSED 1
#define JTK_LC_DEBUG_FILTER_ROWS_TABLE 2
#define JTK_LC_DEBUG_FILTER_TRACE_WORDS 66
JTK_LC_API int jtk_lc_debug_filter(const jtk_lc_params_t *params, size_t n_chunks, const jtk_lc_chunk_t *chunks,
                                   const uint8_t *tmpl_bases, const uint8_t *strand, int mode, const double *values,
                                   const int32_t *exps, const double *lk, double *cand, uint32_t *dim, uint32_t *pos,
                                   uint32_t *vtype, double *feat, uint32_t *trace, int device);

#ifdef __cplusplus
}
#endif
#endif /* JTK_LC_DEBUG_H */
