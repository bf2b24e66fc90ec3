// session_internal.h -- what the host translation units that drive a resident batch share: the session object, its pooled
// device blocks and the steps of a stage call (session.hip defines them; session_split.hip, session_stages.hip,
// session_refit.hip and session_features.hip build the other entry points of include/jtk_lc.h on them; session_trace.hip
// reads a finished session).  The plain records are batch_types.h's; every offset, launch class and wave count of a batch
// is worked out by session_plan.h, which has no HIP in it.
#pragma once
#include <atomic>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "batch_types.h"
#include "device_common.h"
#include "host_common.h"
#include "jtk_lc_debug.h"
#include "session_lanes.h"

#define JTK_POOL_DEVICES 16

// A device block of the session's block pool (session.hip: BlockPool): it goes back to the pool with its owner.
struct DevPtr {
    void *p = nullptr;
    size_t cap = 0;
    int dev = -1;
    ~DevPtr();  // session.hip, beside the pool
    template <typename T>
    T *as() const {
        return reinterpret_cast<T *>(p);
    }
};

// The forward scratch of phmm_kernel / phmm_pair_kernel (device_common.h: StripeSet): one set of stripes per device, shared by
// every session on it -- four slices in flight used to hold four sets of 3,072 x 4.1 MB, of which the device's resident waves
// could only ever use one set's worth.  A session that needs longer stripes than the current set has replaces it (sessions
// that still run keep theirs through the shared_ptr).
struct StripePool {
    DevPtr mem, owner;
    uint64_t stride = 0;  // doubles
    uint32_t n = 0;
    StripeSet set() const {
        return StripeSet{mem.as<double>(), stride, owner.as<uint32_t>(), n};
    }
};

// a model as the kernels read it
inline HmmDev hmm_to_dev(const jtk_hmm_t &h) {
    HmmDev d;
    const double a[9] = {h.mat_mat, h.mat_ins, h.mat_del, h.ins_mat, h.ins_ins, h.ins_del, h.del_mat, h.del_ins, h.del_del};
    memcpy(d.a, a, sizeof a);
    memcpy(d.eM, h.mat_emit, sizeof d.eM);
    memcpy(d.eI, h.ins_emit, sizeof d.eI);
    return d;
}

struct KernelTimer {
    hipEvent_t a = nullptr, b = nullptr;
    int kind = 0;
    // set: the pair belongs to a merged round launch and is shared by the sessions it carried (a family's time then includes
    // the lane-mates'); the last holder destroys the events
    std::shared_ptr<void> shared;
};
void timers_clear(std::vector<KernelTimer> &timers);  // session.hip: destroys the events a session owns alone

// A merged chain launch that carried more than one session of a lane with two streams (session.hip: launch_lane_chains), held
// by its members until their passes are over and by the lane (session_lanes.h: LaneFlight, the stream rule).  Who may leave it
// through its word is lane_member_may_leave: a member for which anything is queued behind the merged kernels --
// mcmc_kernel_huge for its chunks of the global-memory class -- may not; it waits for the event behind its own last kernel
// and keeps its streams.
struct ChainFlight : LaneFlight {
    hipEvent_t end = nullptr;  // behind everything the launch put on its streams
    ~ChainFlight() override {
        if (end) (void)hipEventDestroy(end);
    }
};

// result of one clustering_recursive call (ClusteringDevResult, mod.rs:124)
struct SplitResult {
    std::vector<uint32_t> asn;
    std::vector<double> post;  // n x k log-posteriors
    uint32_t k = 0;
    double score = 0.0;
    int status = 0;
};

struct jtk_lc_session {
    int device = 0;
    // The streams are the session's lane's (session_lanes.h; session.hip: take_lane), shared with the lane's other sessions:
    // `lane` is its index in the device's table, `gather` the lane's chain launches, ev_done what the session records behind
    // its own work to wait for THAT and not for the stream (session_wait).  lane < 0 (session_features.hip): the session made
    // `stream` itself and destroys it.
    hipStream_t stream = nullptr;
    int lane = -1;
    LaneGather<jtk_lc_session> *gather = nullptr;
    // the lane's round gather (session_lanes.h: RoundGather) and what the session asks of it when it parks there: the opening of
    // its pass, or polish round `round` with its own flags
    RoundGather<jtk_lc_session> *rounds = nullptr;
    struct RoundRequest {
        int open = 0, round = 0, only_active = 0, final_pass = 0;
    } round_request;
    std::string round_error;   // the text of a failed round launch that carried this session (written under the gather's mutex)
    hipEvent_t ev_done = nullptr;
    jtk_lc_params_t params;
    uint32_t n_chunks = 0, n_reads = 0, post_stride = 1;
    uint32_t max_tmpl = 0, max_read = 0, max_n = 0, max_copy = 0, n_waves = 0;
    ChainClass chain_class[3];  // the chain kernel's launches (by LDS need), as ranges of d_order; [2]: the pile-ups whose
                                // work area lives in global memory (mcmc_kernel_huge: more than JTK_MAX_PILEUP reads, or more
                                // than a CU's LDS)
    DevPtr d_chain_ws, d_chain_ws_off;
    uint32_t n_pair_items = 0, n_pair_waves = 0;  // phmm_pair_kernel: chunks with band radius <= JTK_PAIR_MAX_RADIUS
    DevPtr d_pair_items;
    std::shared_ptr<StripePool> stripes;  // the device's forward scratch (shared)
    bool features_only = false;
    std::vector<ChunkMeta> h_chunks;
    std::vector<ReadMeta> h_reads;
    std::vector<ChunkState> h_state0;  // initial state (re-uploaded at every run)
    std::vector<uint64_t> h_in_tmpl_off;
    // device memory
    DevPtr d_params, d_hmm2, d_chunks, d_reads, d_state, d_tmpl0, d_tmpl1, d_ops0, d_ops1, d_opslen0, d_opslen1,
        d_ey, d_delta, d_raw, d_rawG, d_lk, d_total, d_edits, d_newlen, d_counter, d_nactive,
        d_homop, d_homop_off, d_aux, d_aux_off, d_cand, d_list, d_sel, d_feat, d_vtype, d_pos, d_label, d_post,
        d_lg, d_lg_off, d_vt_off, d_tmpl_init, d_ops_init, d_opslen_init, d_order;
    size_t tmpl_bytes = 0, ops_bytes = 0;
    DevBufs bufs;
    std::vector<KernelTimer> timers;
    // clustering_recursive (mod.rs:125-189)
    uint32_t ignore_edge = 3;            // HMMPolishConfig ignore_edge: 3 for a chunk (mod.rs:105), 0 for a sub-problem (:153)
    bool has_split = false;              // some chunk has copy_num >= UPPER_COPY_NUM
    std::vector<uint32_t> h_copy0;       // Chunk.copy_num as given (ChunkMeta.copy_num is what one clustering() call sees)
    std::vector<uint8_t> h_read_bases, h_strand;  // kept on the host only when has_split
    std::vector<uint64_t> h_read_off;
    std::vector<SplitResult> split;      // per chunk; .k == 0: not a split chunk
    DevPtr d_rng;                        // 4 x u64 per chunk: where each chunk's RNG stream resumes (sub-problems only)
    bool resume_rng = false;
    bool polish_only = false;            // jtk_lc_polish_chunks: no variant search, no clustering
    bool ran = false, ran_fused = false; // a clustering pass has run (jtk_lc_session_trace needs its device state); with the fused filter?
    // reads whose band is wider than one wavefront (radius > JTK_MAX_RADIUS) take phmm_wide_kernel
    uint32_t n_wide_reads = 0, max_wide_radius = 0, n_wide_waves = 0;
    uint64_t wide_stride = 0;
    DevPtr d_wide_scratch, d_wide_counter;
    DevPtr d_state0;                     // pristine per-chunk state: a pass begins with a device-side copy of it
    // the variable-length outputs of a fetch, packed on the device (io_kernels.hip): lengths per read / chunk, their prefix sums,
    // the re-threaded ops and the consensus as the caller gets them; allocated by the first fetch that asks for them
    DevPtr d_out_len, d_out_off, d_out_ops, d_out_cons;
    // host mirrors of the never-reset device ticket counters of the work queues (device_common.h): d_counter[0] phmm_kernel,
    // d_counter[1] phmm_pair_kernel, d_wide_counter[0] phmm_wide_kernel
    uint32_t tk_phmm = 0, tk_pair = 0, tk_wide = 0;
    uint32_t *h_nactive = nullptr;       // pinned + mapped: the per-round "chunks still active" counters, written by commit_kernel
    uint32_t *h_nactive_dev = nullptr;   // the same memory as the device addresses it
    hipEvent_t ev_round[2] = {nullptr, nullptr};
    // the chain launch: light / general chunk lists made on the device (mcmc_kernels.hip), the general kernel on the lane's
    // second stream (null: the session does not use one)
    DevPtr d_chain_split;
    hipStream_t side = nullptr;
    hipEvent_t ev_chain[2] = {nullptr, nullptr};
    // Leaving a merged launch (session_lanes.h): d_counter[2] counts the session's chain workgroups and is never reset,
    // chain_done is the host's side of it, word JTK_PINNED_CHAIN_WORD of the pinned page is where the last workgroup reports.
    // `flight`: the merged launch the session left through its word, until the next pass; whatever frees the session's buffers
    // waits for its end event first (session_chain_settled).
    ChainDone chain_done;
    std::shared_ptr<ChainFlight> flight;
    bool may_leave = false;  // this pass, through its word (session_lanes.h: lane_member_may_leave)
    std::mutex pass_log_mutex;  // the ledger of the last passes (include/jtk_lc_debug.h), read by another thread
    uint64_t n_passes = 0;
    jtk_lc_debug_pass_t pass_log[JTK_LC_DEBUG_PASS_RECORDS] = {};
    ~jtk_lc_session();  // session.hip: waits for its own work, frees its events, returns its lane and its pinned page
};

// a fetch in two halves (session.hip: fetch_begin / fetch_finish)
struct FetchPlan {
    std::vector<ChunkState> state;
    std::vector<uint32_t> len;      // n_reads ops lengths, then n_chunks consensus lengths
    uint64_t cons_total = 0, ops_total = 0;
    bool want_cons = false, want_ops = false;
    int any_fail = 0;
    hipEvent_t ev0 = nullptr;
};

// ---- session.hip
int dev_alloc_bytes(DevPtr &d, size_t bytes);  // from the block pool, or fresh from the driver
template <typename T>
int dev_alloc(DevPtr &d, size_t count) {
    return dev_alloc_bytes(d, (count ? count : 1) * sizeof(T));
}
template <typename T>
int dev_upload(jtk_lc_session *s, DevPtr &d, const std::vector<T> &v) {
    int rc = dev_alloc<T>(d, v.size());
    if (rc) return rc;
    if (!v.empty()) JTK_HIP_TRY(hipMemcpyAsync(d.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s->stream));
    return 0;
}
int session_wait(jtk_lc_session *s);        // until everything the session has put on its stream so far is done
int session_chain_settled(jtk_lc_session *s);  // until the merged chain launch the session left early has ended as a whole
void tstart(jtk_lc_session *s, int kind);  // a timed stretch of the session's stream; ~jtk_lc_session frees the events
void tstop(jtk_lc_session *s);
int session_create_ex(const jtk_lc_params_t *params, size_t n_chunks, const jtk_lc_chunk_t *chunks,
                      const uint8_t *tmpl_bases, const uint8_t *read_bases, const uint64_t *read_off,
                      const uint8_t *ops, const uint64_t *ops_off, const uint8_t *strand,
                      uint32_t post_stride, int device, const ChunkExtra *extra, uint32_t ignore_edge,
                      jtk_lc_session_t **out, bool polish_only = false);
int run_batch(jtk_lc_session_t *s, int skip_polish);  // one pass of the kernel sequence over the resident batch
// a session's step (the opening of a pass, or a polish round) as a segment of the round kernels' table
RoundSegment round_segment(const jtk_lc_session *s, const jtk_lc_session::RoundRequest &rq);
int fetch_begin(jtk_lc_session_t *s, FetchPlan &pl, uint32_t *label, double *log_post, jtk_lc_result_t *result, bool want_cons,
                bool want_ops);
int fetch_finish(jtk_lc_session_t *s, FetchPlan &pl, uint8_t *cons_out, uint64_t *cons_off, uint64_t cons_base, uint64_t cons_cap,
                 uint8_t *ops_out, uint64_t *ops_out_off, uint64_t ops_base, uint64_t ops_cap);
int fetch_split_results(jtk_lc_session_t *s, uint32_t *label, double *log_post, jtk_lc_result_t *result);
// ---- session_split.hip: clustering_recursive's split branch for the chunks of copy number >= 8, after the batch pass
int run_split(jtk_lc_session_t *s);
