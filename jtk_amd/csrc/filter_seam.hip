// filter_seam.hip -- jtk_lc_debug_filter (include/jtk_lc_debug.h): the variant filter of a clustering pass on planted input.
// Host code only.  The batch is laid out by plan_batch (session_plan.h) exactly as a session's -- reads without bases, so
// every ReadMeta / ChunkMeta offset, tmpl_cap and the buffer totals are the product's -- the input is placed at those offsets,
// and the stage runs through launch_finalize / launch_filter / launch_pick_trace as session_run and jtk_lc_session_trace call
// them.  No kernel is instantiated here.
#include <cmath>
#include <limits>

#include "session_internal.h"
#include "session_plan.h"

namespace {
struct SeamStream {
    hipStream_t s = nullptr;
    ~SeamStream() {
        if (s) (void)hipStreamDestroy(s);
    }
};
}  // namespace

int jtk_lc_debug_filter(const jtk_lc_params_t *params, size_t n_chunks, const jtk_lc_chunk_t *chunks, const uint8_t *tmpl_bases,
                        const uint8_t *strand, int mode, const double *values, const int32_t *exps, const double *lk, double *cand,
                        uint32_t *dim, uint32_t *pos, uint32_t *vtype, double *feat, uint32_t *trace, int device) {
    g_last_error.clear();
    // ---- the arguments: every refusal is the host's, before a device is looked for
    if (mode != JTK_LC_DEBUG_FILTER_TABLE && mode != JTK_LC_DEBUG_FILTER_ROWS_FUSED && mode != JTK_LC_DEBUG_FILTER_ROWS_TABLE)
        return jtk_fail(JTK_ERR_INVALID_ARG, "jtk_lc_debug_filter: no such mode");
    const bool rows = mode != JTK_LC_DEBUG_FILTER_TABLE;
    if (!params || !chunks || !tmpl_bases || !strand || !values || (rows && (!exps || !lk)) || !cand || !dim || !pos || !vtype || !feat ||
        !trace)
        return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    if (n_chunks == 0) return jtk_fail(JTK_ERR_INVALID_ARG, "jtk_lc_debug_filter: no chunk");
    if (params->gains.max_homopolymer_len == 0 || params->gains.max_homopolymer_len > JTK_GAINS_MAX_HOMOP)
        return jtk_fail(JTK_ERR_INVALID_ARG, "gains.max_homopolymer_len out of range");
    uint64_t n_reads = 0;
    int rc = check_contiguous(chunks, n_chunks, &n_reads);
    if (rc) return rc;
    for (size_t c = 0; c < n_chunks; c++) {
        if (chunks[c].copy_num == 0 || chunks[c].copy_num > JTK_MAX_COPY)
            return jtk_fail(JTK_ERR_INVALID_ARG, "jtk_lc_debug_filter: one clustering() call sees a copy number of 1 .. 7");
        if (chunks[c].n_reads == 0 || chunks[c].tmpl_len == 0) return jtk_fail(JTK_ERR_INVALID_ARG, "jtk_lc_debug_filter: an empty chunk");
    }
    const std::vector<uint64_t> no_bases(n_reads + 1, 0);  // reads without bases and without ops
    BatchPlan bp;
    std::string msg;
    if ((rc = plan_batch(*params, n_chunks, chunks, no_bases.data(), no_bases.data(), strand, JTK_MAX_COPY, nullptr, false, bp, msg)))
        return jtk_fail(rc, msg);
    const int fused = mode == JTK_LC_DEBUG_FILTER_ROWS_FUSED;
    if (fused && batch_needs_tables(false, bp.max_n))
        return jtk_fail(JTK_ERR_INVALID_ARG, "jtk_lc_debug_filter: the fused filter takes pile-ups of up to 65,535 reads");
    std::vector<uint8_t> h_tmpl;
    if (!recode_templates(bp, chunks, tmpl_bases, h_tmpl)) return jtk_fail(JTK_ERR_INVALID_ARG, "non-ACGT base in a template");
    for (const ChunkState &st : bp.state0)
        if (st.status != 0) return jtk_fail(st.status, "jtk_lc_debug_filter: a template too long for the session's bands");

    // ---- the input at the plan's offsets; what the plan leaves between two reads is NaN (exponents: INT_MIN)
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<double> h_raw(bp.raw, nan), h_lk(bp.n_reads, 0.0);
    std::vector<int> h_G(bp.row, std::numeric_limits<int>::min());
    {
        uint64_t vo = 0, eo = 0;
        for (size_t c = 0; c < n_chunks; c++) {
            const ChunkMeta &cm = bp.chunks[c];
            const uint64_t rows_c = chunks[c].tmpl_len + 1, per_read = (rows ? JTK_ACC_N : JTK_NUM_ROW) * rows_c;
            for (uint32_t r = 0; r < cm.n_reads; r++) {
                const ReadMeta &rm = bp.reads[cm.read_first + r];
                memcpy(h_raw.data() + (rows ? rm.raw_off : rm.table_off), values + vo, per_read * sizeof(double));
                vo += per_read;
                if (rows) {
                    memcpy(h_G.data() + rm.row_off, exps + eo, rows_c * sizeof(int));
                    eo += rows_c;
                    h_lk[cm.read_first + r] = lk[cm.read_first + r];
                }
            }
        }
    }

    // ---- the device: a session's buffers for this stage, from the plan's totals
    if ((rc = jtk_require_device(device))) return rc;
    SeamStream stream;
    JTK_HIP_TRY(hipStreamCreate(&stream.s));
    hipStream_t st = stream.s;
    const std::vector<jtk_lc_params_t> pv(1, *params);
    const std::vector<HmmDev> hv = {hmm_to_dev(params->forward), hmm_to_dev(params->reverse)};
    DevBuf d_params, d_hmm2, d_chunks, d_reads, d_state, d_tmpl, d_raw, d_rawG, d_lk, d_homop, d_homop_off, d_aux, d_aux_off, d_cand,
        d_list, d_sel, d_feat, d_vtype, d_pos, d_tr, d_cnt;
#define SEAM_TRY(expr)                                                                              \
    do {                                                                                            \
        const int _rc = (expr);                                                                     \
        if (_rc) return jtk_fail(_rc, "jtk_lc_debug_filter: a device buffer could not be set up");  \
    } while (0)
    SEAM_TRY(d_params.upload(pv, st));
    SEAM_TRY(d_hmm2.upload(hv, st));
    SEAM_TRY(d_chunks.upload(bp.chunks, st));
    SEAM_TRY(d_reads.upload(bp.reads, st));
    SEAM_TRY(d_state.upload(bp.state0, st));
    SEAM_TRY(d_tmpl.upload(h_tmpl, st));
    SEAM_TRY(d_raw.upload(h_raw, st));
    SEAM_TRY(d_rawG.upload(h_G, st));
    SEAM_TRY(d_lk.upload(h_lk, st));
    SEAM_TRY(d_homop_off.upload(bp.homop_off, st));
    SEAM_TRY(d_aux_off.upload(bp.aux_off, st));
#undef SEAM_TRY
    const size_t n_tr = (size_t)n_chunks * JTK_LC_DEBUG_FILTER_TRACE_WORDS;
    static_assert(JTK_LC_DEBUG_FILTER_TRACE_WORDS == 2 + JTK_TRACE_MAX_PICKS, "trace words");
    JTK_HIP_TRY(d_homop.alloc(bp.tmpl * sizeof(uint16_t)));
    JTK_HIP_TRY(d_aux.alloc(bp.aux * sizeof(double)));
    JTK_HIP_TRY(d_cand.alloc(bp.cand * sizeof(double)));
    JTK_HIP_TRY(d_list.alloc(bp.cand * sizeof(uint32_t)));
    JTK_HIP_TRY(d_sel.alloc(bp.cand));
    JTK_HIP_TRY(d_feat.alloc(bp.feat * sizeof(double)));
    JTK_HIP_TRY(d_vtype.alloc(2 * n_chunks * JTK_MAX_DIM * sizeof(uint32_t)));
    JTK_HIP_TRY(d_pos.alloc(n_chunks * JTK_MAX_DIM * sizeof(uint32_t)));
    JTK_HIP_TRY(d_tr.alloc(n_tr * sizeof(uint32_t)));
    JTK_HIP_TRY(d_cnt.alloc(bp.cand * sizeof(uint32_t)));
    JTK_HIP_TRY(hipMemsetAsync(d_feat.p, 0, bp.feat * sizeof(double), st));
    JTK_HIP_TRY(hipMemsetAsync(d_vtype.p, 0, 2 * n_chunks * JTK_MAX_DIM * sizeof(uint32_t), st));
    JTK_HIP_TRY(hipMemsetAsync(d_pos.p, 0, n_chunks * JTK_MAX_DIM * sizeof(uint32_t), st));
    JTK_HIP_TRY(hipMemsetAsync(d_tr.p, 0, n_tr * sizeof(uint32_t), st));
    DevBufs bufs;
    memset(&bufs, 0, sizeof bufs);
    for (int b = 0; b < 3; b++) bufs.tmpl[b] = static_cast<uint8_t *>(d_tmpl.p);  // (the state says set 0: the batch as uploaded)
    const ReadMeta *reads = static_cast<const ReadMeta *>(d_reads.p);
    const ChunkMeta *cms = static_cast<const ChunkMeta *>(d_chunks.p);
    ChunkState *state = static_cast<ChunkState *>(d_state.p);
    const HmmDev *hmm2 = static_cast<const HmmDev *>(d_hmm2.p);
    const jtk_lc_params_t *dp = static_cast<const jtk_lc_params_t *>(d_params.p);
    double *raw = static_cast<double *>(d_raw.p);
    const int *rawG = static_cast<const int *>(d_rawG.p);
    const double *dlk = static_cast<const double *>(d_lk.p);

    // ---- the stage, as session_run has it
    if (mode == JTK_LC_DEBUG_FILTER_ROWS_TABLE) launch_finalize(st, (uint32_t)bp.n_reads, reads, cms, state, hmm2, raw, rawG, dlk, bp.max_tmpl, 0);
    launch_filter(st, (uint32_t)n_chunks, reads, cms, state, bufs, dp, raw, static_cast<uint16_t *>(d_homop.p),
                  static_cast<const uint64_t *>(d_homop_off.p), static_cast<double *>(d_aux.p), static_cast<const uint64_t *>(d_aux_off.p),
                  static_cast<double *>(d_cand.p), static_cast<uint32_t *>(d_list.p), static_cast<uint8_t *>(d_sel.p),
                  static_cast<double *>(d_feat.p), static_cast<uint32_t *>(d_vtype.p), static_cast<uint32_t *>(d_pos.p), bp.max_tmpl, hmm2,
                  rawG, dlk, fused);
    std::vector<double> h_cand(bp.cand);
    std::vector<ChunkState> h_state(n_chunks);
    JTK_HIP_TRY(hipMemcpyAsync(h_cand.data(), d_cand.p, bp.cand * sizeof(double), hipMemcpyDeviceToHost, st));
    JTK_HIP_TRY(hipMemcpyAsync(h_state.data(), d_state.p, n_chunks * sizeof(ChunkState), hipMemcpyDeviceToHost, st));
    JTK_HIP_TRY(hipMemcpyAsync(pos, d_pos.p, n_chunks * JTK_MAX_DIM * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    JTK_HIP_TRY(hipMemcpyAsync(vtype, d_vtype.p, 2 * n_chunks * JTK_MAX_DIM * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    JTK_HIP_TRY(hipMemcpyAsync(feat, d_feat.p, bp.feat * sizeof(double), hipMemcpyDeviceToHost, st));
    JTK_HIP_TRY(hipStreamSynchronize(st));
    JTK_HIP_TRY(hipGetLastError());
    // ---- the pick once more per chunk, for its order (jtk_lc_session_trace's launch; it leaves every output as it was)
    for (size_t c = 0; c < n_chunks; c++) {
        if (bp.chunks[c].copy_num < 2) continue;  // (clustering() returns before the search: the kernel would pick among none)
        launch_pick_trace(st, (uint32_t)c, reads, cms, state, dp, raw, static_cast<const uint16_t *>(d_homop.p),
                          static_cast<const uint64_t *>(d_homop_off.p), static_cast<const double *>(d_cand.p), static_cast<uint32_t *>(d_list.p),
                          static_cast<uint8_t *>(d_sel.p), static_cast<double *>(d_feat.p), static_cast<uint32_t *>(d_vtype.p),
                          static_cast<uint32_t *>(d_pos.p), hmm2, rawG, dlk, fused,
                          static_cast<uint32_t *>(d_tr.p) + c * JTK_LC_DEBUG_FILTER_TRACE_WORDS, static_cast<uint32_t *>(d_cnt.p) + bp.chunks[c].cand_off);
    }
    JTK_HIP_TRY(hipMemcpyAsync(trace, d_tr.p, n_tr * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    JTK_HIP_TRY(hipStreamSynchronize(st));
    JTK_HIP_TRY(hipGetLastError());
    uint64_t co = 0;
    for (size_t c = 0; c < n_chunks; c++) {
        if (h_state[c].status != 0) return jtk_fail(h_state[c].status, "jtk_lc_debug_filter: a chunk failed");
        const uint64_t cols = (uint64_t)JTK_NUM_ROW * (chunks[c].tmpl_len + 1);
        memcpy(cand + co, h_cand.data() + bp.chunks[c].cand_off, cols * sizeof(double));
        co += cols;
        dim[c] = h_state[c].dim;
    }
    return JTK_OK;
}
