// device_common.h -- shared declarations of the HIP kernels (gfx950 only) and the session that drives them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "batch_types.h"
#include "jtk_lc.h"
#include "jtk_math.h"

// ---- kernel launchers (definitions in the .hip files) ----
size_t phmm_lds_bytes(uint32_t max_tmpl, uint32_t max_read);
// Work queues (phmm, phmm_pair, phmm_wide, phmm_counts): `work_counter` is a device ticket counter that is never reset (no fill
// blit in front of a launch).  A wave takes tickets until one is past the launch's last item, so a launch advances the counter
// by exactly n_items + n_waves; `ticket_base` (host) is the counter's value when the launch starts and is advanced by the launcher.
// The forward scratch of the lane-ring pair-HMM kernels: stripes of (template + read + guard) x 1 KiB, one per RESIDENT wave.
// The set is shared by every session of a device (session_internal.h: StripePool): however many batches are in flight, no more
// waves than the device holds are ever inside a sweep, so a wave takes a free stripe when it starts and gives it back when it
// ends (owner[]: 0 = free).  Release / acquire at agent scope on the hand-over: a stripe may move between XCDs, whose L2s are
// not coherent with each other -- nothing depends on where a wave runs.
struct StripeSet {
    double *mem;
    uint64_t stride;  // doubles per stripe
    uint32_t *owner;
    uint32_t n;       // stripes (>= the waves the device can hold: nobody ever waits for long)
};
#ifdef __HIPCC__
__device__ __forceinline__ uint32_t jtk_stripe_acquire(const StripeSet &ss) {
    uint32_t got = 0;
    if (threadIdx.x == 0) {
        // start anywhere (the cycle counter differs between waves and launches), probe linearly; holders never wait for anything,
        // so a full table only means a short wait
        uint32_t h = (uint32_t)((__builtin_readcyclecounter() * 0x9E3779B97F4A7C15ull) >> 40) % ss.n;
        for (uint32_t tries = 0;; tries++) {
            uint32_t expected = 0;
            if (__hip_atomic_compare_exchange_strong(&ss.owner[h], &expected, 1u, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT))
                break;
            if (++h == ss.n) h = 0;
            if ((tries & 255u) == 255u) __builtin_amdgcn_s_sleep(16);
        }
        got = h;
    }
    got = (uint32_t)__builtin_amdgcn_readfirstlane((int)got);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // every lane: what the previous holder wrote is not read stale
    return got;
}
__device__ __forceinline__ void jtk_stripe_release(const StripeSet &ss, uint32_t stripe) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");  // every lane's stores to the stripe are out of this XCD's L2 first
    if (threadIdx.x == 0) __hip_atomic_store(&ss.owner[stripe], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
#endif
// phmm_pair.hip: the same sweep for band radius <= JTK_PAIR_MAX_RADIUS, two reads of a chunk per wave.  items[q] = index of
// the first read of the pair, bit 31 set when the item is a single read; phmm_kernel is then told to skip those chunks.
size_t phmm_pair_lds_bytes(uint32_t max_tmpl, uint32_t max_read);
void launch_phmm_pair(hipStream_t s, uint32_t n_items, const uint32_t *items, const ReadMeta *reads, const ChunkMeta *chunks,
                      const ChunkState *state, DevBufs bufs, const uint8_t *ey, const uint64_t *delta, const HmmDev *hmm2,
                      StripeSet stripes, uint32_t n_waves, uint32_t *work_counter, uint32_t *ticket_base,
                      double *raw, int *rawG, double *lk, uint32_t max_tmpl, uint32_t max_read, int only_active);
void launch_finalize(hipStream_t s, uint32_t n_reads, const ReadMeta *reads, const ChunkMeta *chunks,
                     const ChunkState *state, const HmmDev *hmm2, double *raw, const int *rawG, const double *lk,
                     uint32_t max_tmpl, int only_active, int converged_in = -1);  // in place: a read's table takes the place of
                                                                                   // its row sums; converged_in >= 0: only the
                                                                                   // chunks that converged in that polish round
// phmm_wide.hip: the reads of chunks whose band radius exceeds JTK_MAX_RADIUS (phmm_kernel skips them)
size_t phmm_wide_lds_bytes(uint32_t max_tmpl, uint32_t max_read, uint32_t max_radius);
uint64_t phmm_wide_scratch_doubles(uint32_t max_tmpl, uint32_t max_read, uint32_t max_radius);
void launch_phmm_wide(hipStream_t s, uint32_t n_reads, const ReadMeta *reads, const ChunkMeta *chunks,
                      const ChunkState *state, DevBufs bufs, const uint8_t *ey, const uint64_t *delta, const HmmDev *hmm2,
                      double *scratch, uint64_t scratch_stride, uint32_t n_waves, uint32_t *work_counter, uint32_t *ticket_base,
                      double *raw, int *rawG, double *lk, uint32_t max_tmpl, uint32_t max_read, int only_active,
                      uint32_t max_radius);
// expected transition / emission counts of every read of a batch (E-step of the model refit); 45 doubles per read
size_t phmm_counts_lds_bytes(uint32_t max_tmpl, uint32_t max_read, uint32_t max_radius);
uint64_t phmm_counts_scratch_doubles(uint32_t max_tmpl, uint32_t max_read, uint32_t max_radius);
void launch_phmm_counts(hipStream_t s, uint32_t n_reads, const ReadMeta *reads, const ChunkMeta *chunks,
                        const ChunkState *state, DevBufs bufs, const uint8_t *ey, const uint64_t *delta, const HmmDev *hmm2,
                        double *scratch, uint64_t scratch_stride, uint32_t n_waves, uint32_t *work_counter, uint32_t *ticket_base,
                        double *counts, double *lk, uint32_t max_tmpl, uint32_t max_read, uint32_t max_radius);
// io_kernels.hip: the raw reads / ops of a batch recoded on the device (flags: bit 1 = non-ACGT base, bit 2 = op code > 3), and
// the variable-length results packed for the copy back (lengths first, then consensus as ASCII + ops at prefix-summed offsets)
void launch_encode_reads(hipStream_t s, uint32_t n_reads, const ReadMeta *reads, const uint8_t *raw_bases,
                         const uint64_t *raw_base_off, const uint8_t *raw_ops, const uint64_t *raw_ops_off, uint8_t *ey,
                         uint8_t *ops, uint32_t *flags);
void launch_out_len(hipStream_t s, uint32_t n_reads, uint32_t n_chunks, const ReadMeta *reads, const ChunkState *state,
                    DevBufs bufs, uint32_t *ops_len_out, uint32_t *cons_len_out);
void launch_gather(hipStream_t s, uint32_t n_reads, uint32_t n_chunks, const ReadMeta *reads, const ChunkMeta *chunks,
                   const ChunkState *state, DevBufs bufs, const uint64_t *ops_out_off, const uint64_t *cons_off,
                   uint8_t *ops_out, uint8_t *cons_out);
// polish_kernels.hip
#define JTK_NACTIVE_SLOTS (JTK_POLISH_MAX_ROUNDS + 3)  // one "chunks still active" counter per polish round of a pass
// a session's mapped pinned page: the round counters' mirror, then the word the chain kernels report a finished segment in
#define JTK_PINNED_CHAIN_WORD JTK_NACTIVE_SLOTS
#define JTK_PINNED_WORDS (JTK_NACTIVE_SLOTS + 1)
// The kernels of a polish round take the rounds of up to JTK_ROUND_MAX_SEGMENTS sessions in one launch (the sessions of a
// lane, session_lanes.h: RoundGather); a session on its own is a table of one segment -- there is one kernel per step.  A
// segment is one session's round: its pointers, its own flags, and which step of its pass it is at -- the opening (`open`:
// reset_pass + band_prep of every read) or polish round `round` (phmm, sum_final, select_edits, rethread, commit, band_prep
// of the active chunks; a final pass ends after select_edits).  Lane-mates need not be at the same step.  Every kernel takes
// the table by value plus its own prefix of first blocks / items (a segment that has no part in the kernel has no width),
// finds its segment by a scalar scan of the prefix and works on that segment's pointers with a rebased index: for every
// session the same arithmetic on the same buffers in the same order, whoever shares the launch.  Nothing waits for anything.
#define JTK_ROUND_MAX_SEGMENTS 8
struct RoundSegment {
    uint32_t n_chunks, n_reads;
    const ReadMeta *reads;
    const ChunkMeta *chunks;
    ChunkState *state;
    const ChunkState *state0;
    DevBufs bufs;
    const uint8_t *ey;
    uint64_t *delta;
    const HmmDev *hmm2;
    double *raw;
    int *rawG;
    double *lk;
    double *total;
    Edit *edits;
    uint32_t *new_len;
    uint32_t *n_active;       // the session's JTK_NACTIVE_SLOTS counters; round r's is n_active[r]
    uint32_t *n_active_host;  // their pinned mirror as the device addresses it (or null)
    uint32_t max_tmpl, max_read, n_waves;
    uint32_t open, round;     // the pass's opening, or polish round `round`
    uint32_t ignore_edge, skip_le_radius;
    int only_active, final_pass;
};
struct RoundSegTable {
    RoundSegment seg[JTK_ROUND_MAX_SEGMENTS];
    uint32_t n;
};
// what a launch carried, read back from the table the kernels were given (the lane's round ledger)
struct RoundLaunchInfo {
    uint32_t segments;                           // of the table
    uint32_t round[JTK_ROUND_MAX_SEGMENTS];      // 0xffffffff: the opening
    uint32_t chunks[JTK_ROUND_MAX_SEGMENTS];
    uint32_t phmm_items[JTK_ROUND_MAX_SEGMENTS]; // the segment's width in phmm_kernel's item space
};
// a kernel's own prefix: first[i] = the first block (or item) of segment i, first[JTK_ROUND_MAX_SEGMENTS] = their number;
// entries past the table's last segment hold that number too, so the scan needs no segment count
struct RoundFirst {
    uint32_t first[JTK_ROUND_MAX_SEGMENTS + 1];
};
template <class Width>
inline uint32_t round_prefix(const RoundSegTable &t, RoundFirst &f, Width &&width) {
    uint32_t at = 0;
    for (uint32_t i = 0; i <= JTK_ROUND_MAX_SEGMENTS; i++) {
        f.first[i] = at;
        if (i < t.n) at += width(t.seg[i]);
    }
    return at;
}
#ifdef __HIPCC__
// idx < first[JTK_ROUND_MAX_SEGMENTS]: the segment that holds it (a segment without width is never found).  Everything here
// is uniform and comes from the kernel-argument segment: scalar loads and compares.
__device__ __forceinline__ uint32_t round_segment_of(const RoundFirst &f, uint32_t idx) {
    uint32_t i = 0;
#pragma unroll
    for (uint32_t j = 1; j < JTK_ROUND_MAX_SEGMENTS; j++)
        if (idx >= f.first[j]) i = j;
    return i;
}
#endif
void round_table_info(const RoundSegTable &t, RoundLaunchInfo *info);
void launch_reset_pass(hipStream_t s, const RoundSegTable &t);
void launch_band_prep(hipStream_t s, const RoundSegTable &t);
// `work_counter` / `ticket_base`: a never-reset ticket counter and its host mirror (above) -- the lane's for a launch through
// the lane's gather, the session's own otherwise; `stripes`: a set whose stripes are long enough for every segment; n_waves: of
// the largest segment (at most the set's stripes)
void launch_phmm(hipStream_t s, const RoundSegTable &t, StripeSet stripes, uint32_t n_waves, uint32_t *work_counter,
                 uint32_t *ticket_base);
// the column totals of a polish round straight from the row sums (finalize's arithmetic + the ordered sum, no table written)
void launch_sum_final(hipStream_t s, const RoundSegTable &t);
void launch_polish_round(hipStream_t s, const RoundSegTable &t);  // select_edits, rethread, commit (after launch_sum_final)
// filter_kernels.hip: the variant search of a clustering pass, and one chunk's pick once more with its trace arrays
void launch_filter(hipStream_t s, uint32_t n_chunks, const ReadMeta *reads, const ChunkMeta *chunks,
                   ChunkState *state, DevBufs bufs, const jtk_lc_params_t *params, const double *table,
                   uint16_t *homop, const uint64_t *homop_off, double *aux, const uint64_t *aux_off, double *cand,
                   uint32_t *list, uint8_t *sel, double *feat, uint32_t *vtype, uint32_t *pos, uint32_t max_tmpl,
                   const HmmDev *hmm2, const int *rawG, const double *lk, int fused);
void launch_pick_trace(hipStream_t s, uint32_t ci, const ReadMeta *reads, const ChunkMeta *chunks, ChunkState *state,
                       const jtk_lc_params_t *params, const double *table, const uint16_t *homop, const uint64_t *homop_off,
                       const double *cand, uint32_t *list, uint8_t *sel, double *feat, uint32_t *vtype, uint32_t *pos,
                       const HmmDev *hmm2, const int *rawG, const double *lk, int fused, uint32_t *tr, uint32_t *tr_count);
// mcmc_kernels.hip (with the chain_*.h headers it alone includes; the sizes: chain_layout.h): the chain.  Its work area lives in LDS (launch_mcmc, sized per launch by mcmc_lds_bytes) or, for pile-ups
// beyond that, in global memory (launch_mcmc_huge, mcmc_ws_bytes); launch_mcmc_trace runs one chunk again with its records
size_t mcmc_trace_doubles(uint32_t n_reads);
int launch_mcmc_trace(hipStream_t s, const ChunkMeta *chunks, ChunkState *state, const jtk_lc_params_t *params, const double *feat,
                      const uint32_t *vtype, uint32_t *label, double *post, uint32_t post_stride, double *lg, const uint64_t *lg_off,
                      uint32_t n, uint32_t d, uint32_t k, const uint32_t *order, unsigned char *ws, const uint64_t *ws_off,
                      double *trace);
size_t mcmc_lds_bytes(uint32_t lds_n, uint32_t lds_d, uint32_t lds_k);
size_t mcmc_ws_bytes(uint32_t n, uint32_t d, uint32_t k);
int launch_mcmc_huge(hipStream_t s, uint32_t n_chunks, const ChunkMeta *chunks, ChunkState *state, const jtk_lc_params_t *params,
                     const double *feat, const uint32_t *vtype, const uint64_t *vt_off, uint32_t vt_stride_mode, uint32_t *label,
                     double *post, uint32_t post_stride, double *lg, const uint64_t *lg_off, uint32_t max_n, uint32_t max_d,
                     uint32_t max_k, const uint64_t *rng_resume, const uint32_t *order, unsigned char *ws, const uint64_t *ws_off);
int launch_mcmc(hipStream_t s, uint32_t n_chunks, const ChunkMeta *chunks, ChunkState *state,
                const jtk_lc_params_t *params, const double *feat, const uint32_t *vtype, const uint64_t *vt_off,
                uint32_t vt_stride_mode, uint32_t *label, double *post, uint32_t post_stride, double *lg,
                const uint64_t *lg_off, uint32_t lds_n, uint32_t lds_d, uint32_t lds_k, const uint64_t *rng_resume,
                const uint32_t *order, uint32_t *split, hipStream_t side, hipEvent_t ev_fork, hipEvent_t ev_join);
// One chain launch for several sessions (the sessions of a lane, session_lanes.h): a segment is what launch_mcmc takes for one
// session; the kernels get the segments as a by-value table and a workgroup finds its own by its index.  n_seg = 1 is
// launch_mcmc.  Every segment has a split scratch and no rng_resume (anything else launches alone, through launch_mcmc).
#define JTK_MCMC_MAX_SEGMENTS 8
struct McmcSegment {
    uint32_t n_chunks;
    const ChunkMeta *chunks;
    ChunkState *state;
    const jtk_lc_params_t *params;
    const double *feat;
    const uint32_t *vtype;
    const uint64_t *vt_off;
    uint32_t vt_stride_mode;
    uint32_t *label;
    double *post;
    uint32_t post_stride;
    double *lg;
    const uint64_t *lg_off;
    uint32_t lds_n, lds_d, lds_k;
    const uint64_t *rng_resume;
    const uint32_t *order;
    uint32_t *split;
    // The segment's own completion, or null.  `done`: a device counter that is never reset; every workgroup the launch makes
    // for the segment adds one when it ends -- mcmc_chain_workgroups(segment) of them, the ones past the device-side list
    // length included -- and the one that brings it to done_target (the host's count of everything launched for the segment so
    // far) stores done_pass to *done_word, mapped pinned memory as the device addresses it.  No kernel waits for any of it.
    uint32_t *done = nullptr, *done_word = nullptr;
    uint32_t done_target = 0, done_pass = 0;
};
// the workgroups launch_mcmc_merged makes for a segment: one per chunk in the general kernel and, where the segment has a
// split scratch and no rng_resume, one per chunk in the light kernel as well
inline uint32_t mcmc_chain_workgroups(const McmcSegment &x) { return (x.split && !x.rng_resume ? 2u : 1u) * x.n_chunks; }
int launch_mcmc_merged(hipStream_t s, int n_seg, const McmcSegment *seg, hipStream_t side, hipEvent_t ev_fork, hipEvent_t ev_join);
