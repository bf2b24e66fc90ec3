// session_trace.hip -- readers of a finished session: the reference's trace! rows of one chunk (include/jtk_lc.h:
// jtk_lc_session_trace) and the chain's per-chunk profile (include/jtk_lc_debug.h).  Host code only.
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "session_internal.h"
#include "session_plan.h"

namespace {
void trace_row(std::string &out, const char *fmt, ...) {
    char line[512];
    va_list ap;
    va_start(ap, fmt);
    int m = vsnprintf(line, sizeof line, fmt, ap);
    va_end(ap);
    if (m < 0) return;
    out.append(line, std::min<size_t>((size_t)m, sizeof line - 1));
    out.push_back('\n');
}
std::string fx(double x, int prec) {  // Rust's {x:.N}: the correctly rounded decimal, as printf's; NaN is "NaN"
    if (x != x) return "NaN";
    char b[400];
    snprintf(b, sizeof b, "%.*f", prec, x);
    return b;
}
}  // namespace

int jtk_lc_session_trace(jtk_lc_session_t *s, size_t chunk, char *text, size_t cap, size_t *len) {
    g_last_error.clear();
    if (!s || !len || (cap && !text)) return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    *len = 0;
    if (chunk >= s->n_chunks) return jtk_fail(JTK_ERR_INVALID_ARG, "no such chunk in the session");
    if (s->polish_only || s->features_only || !s->ran)
        return jtk_fail(JTK_ERR_INVALID_ARG, "jtk_lc_session_trace needs a session whose last jtk_lc_session_run clustered its chunks");
    if (s->has_split)  // (run_split re-uses the session's buffers for the sub-problems of clustering_recursive, mod.rs:125-189)
        return jtk_fail(JTK_ERR_UNSUPPORTED, "jtk_lc_session_trace: the session holds a chunk of copy number >= 8 (clustering_recursive)");
    JTK_HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = s->stream;
    const uint32_t ci = (uint32_t)chunk;
    const ChunkMeta &cm = s->h_chunks[ci];
    ChunkState cs;
    JTK_HIP_TRY(hipMemcpyAsync(&cs, s->d_state.as<ChunkState>() + ci, sizeof cs, hipMemcpyDeviceToHost, st));
    JTK_HIP_TRY(hipStreamSynchronize(st));
    if (cs.status != 0) return jtk_fail(cs.status, "jtk_lc_session_trace: the chunk failed in the run");
    std::string out;
    if (cm.copy_num < 2) {  // clustering() returns before anything is logged (pseudo_mcmc.rs:86-88)
        *len = 0;
        return JTK_OK;
    }
    const uint32_t n = cm.n_reads, L = cs.tmpl_len, cols = JTK_NUM_ROW * (L + 1);
    // ---- the pick once more, with its trace arrays
    DevPtr d_tr, d_cnt, d_order1, d_ws, d_ws_off, d_trace;
    int rc;
    if ((rc = dev_alloc<uint32_t>(d_tr, 2 + JTK_TRACE_MAX_PICKS))) return rc;
    if ((rc = dev_alloc<uint32_t>(d_cnt, cols))) return rc;
    JTK_HIP_TRY(hipMemsetAsync(d_tr.p, 0, (2 + JTK_TRACE_MAX_PICKS) * sizeof(uint32_t), st));
    launch_pick_trace(st, ci, s->d_reads.as<ReadMeta>(), s->d_chunks.as<ChunkMeta>(), s->d_state.as<ChunkState>(),
                      s->d_params.as<jtk_lc_params_t>(), s->d_raw.as<double>(), s->d_homop.as<uint16_t>(), s->d_homop_off.as<uint64_t>(),
                      s->d_cand.as<double>(), s->d_list.as<uint32_t>(), s->d_sel.as<uint8_t>(), s->d_feat.as<double>(),
                      s->d_vtype.as<uint32_t>(), s->d_pos.as<uint32_t>(), s->d_hmm2.as<HmmDev>(), s->d_rawG.as<int>(), s->d_lk.as<double>(),
                      s->ran_fused ? 1 : 0, d_tr.as<uint32_t>(), d_cnt.as<uint32_t>());
    std::vector<uint32_t> tr(2 + JTK_TRACE_MAX_PICKS);
    JTK_HIP_TRY(hipMemcpyAsync(tr.data(), d_tr.p, tr.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    JTK_HIP_TRY(hipMemcpyAsync(&cs, s->d_state.as<ChunkState>() + ci, sizeof cs, hipMemcpyDeviceToHost, st));
    JTK_HIP_TRY(hipStreamSynchronize(st));
    JTK_HIP_TRY(hipGetLastError());
    const uint32_t np = std::min(tr[0], cols), n_picks = std::min<uint32_t>(tr[1], JTK_TRACE_MAX_PICKS), D = cs.dim;
    std::vector<uint32_t> list(np), cnt(np), pos(JTK_MAX_DIM);
    std::vector<double> cand(cols), feat((size_t)n * D);
    if (np) {
        JTK_HIP_TRY(hipMemcpyAsync(list.data(), s->d_list.as<uint32_t>() + cm.cand_off, np * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        JTK_HIP_TRY(hipMemcpyAsync(cnt.data(), d_cnt.p, np * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    JTK_HIP_TRY(hipMemcpyAsync(cand.data(), s->d_cand.as<double>() + cm.cand_off, cols * sizeof(double), hipMemcpyDeviceToHost, st));
    JTK_HIP_TRY(hipMemcpyAsync(pos.data(), s->d_pos.as<uint32_t>() + (uint64_t)ci * JTK_MAX_DIM, JTK_MAX_DIM * sizeof(uint32_t),
                           hipMemcpyDeviceToHost, st));
    if (!feat.empty())
        JTK_HIP_TRY(hipMemcpyAsync(feat.data(), s->d_feat.as<double>() + cm.feat_off, feat.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    JTK_HIP_TRY(hipStreamSynchronize(st));
    auto diff_letter = [](uint32_t row) { return row < 4 ? "S" : (row < 8 + JTK_COPY_SIZE ? "I" : "D"); };  // pos_to_bp_and_difftype :168-178
    trace_row(out, "TOTAL\t%u", np);                                                                       // :467
    for (uint32_t i = 0; i < np; i++)                                                                       // :468-472
        trace_row(out, "CAND\t%u\t%u\t%s\t%u", list[i] / JTK_NUM_ROW, list[i] % JTK_NUM_ROW, fx(cand[list[i]], 1).c_str(), cnt[i]);
    for (uint32_t p = 0; p < n_picks; p++) {                                                                // :537-539
        const uint32_t col = tr[2 + p] < np ? list[tr[2 + p]] : 0;
        trace_row(out, "PICK\t%u\t%s\t%s", col / JTK_NUM_ROW, diff_letter(col % JTK_NUM_ROW), fx(cand[col], 3).c_str());
    }
    for (uint32_t d = 0; d < D; d++) {                                                                      // :122-127
        double sum = 0.0;
        for (uint32_t r = 0; r < n; r++) {
            const double x = feat[(size_t)r * D + d];
            sum += x != x ? 0.0 : (x > 0.0 ? x : 0.0);  // f64::max(x, 0) ignores NaN
        }
        trace_row(out, "DUMP\t%u\t%u\t%u\t%s\t%s", d, pos[d] / JTK_NUM_ROW, pos[d] % JTK_NUM_ROW, fx(cand[pos[d]], 1).c_str(),
                  fx(sum, 1).c_str());
    }
    // ---- cluster_filtered_variants once more, with its records (:213-274); its early return logs nothing (:221-225)
    if (!(D == 0 || n <= cm.copy_num)) {
        const uint32_t k = chain_dims_of(cm).k, dmax = chain_dims_of(cm).d;
        std::vector<uint32_t> order1(1, ci);
        std::vector<uint64_t> ws_off1(1, 0);
        if ((rc = dev_upload(s, d_order1, order1))) return rc;
        if ((rc = dev_upload(s, d_ws_off, ws_off1))) return rc;
        if ((rc = dev_alloc<uint8_t>(d_ws, mcmc_ws_bytes(n, dmax, k)))) return rc;
        const size_t tn = mcmc_trace_doubles(n);
        if ((rc = dev_alloc<double>(d_trace, tn))) return rc;
        JTK_HIP_TRY(hipMemsetAsync(d_trace.p, 0, tn * sizeof(double), st));
        if (launch_mcmc_trace(st, s->d_chunks.as<ChunkMeta>(), s->d_state.as<ChunkState>(), s->d_params.as<jtk_lc_params_t>(),
                              s->d_feat.as<double>(), s->d_vtype.as<uint32_t>(), s->d_label.as<uint32_t>(), s->d_post.as<double>(),
                              s->post_stride, s->d_lg.as<double>(), s->d_lg_off.as<uint64_t>(), n, dmax, k, d_order1.as<uint32_t>(),
                              d_ws.as<uint8_t>(), d_ws_off.as<uint64_t>(), d_trace.as<double>()) != 0) {
            (void)hipStreamSynchronize(st);
            return jtk_fail(JTK_ERR_INTERNAL, "the chain kernel could not be launched (jump table upload failed)");
        }
        std::vector<double> tv(tn);
        JTK_HIP_TRY(hipMemcpyAsync(tv.data(), d_trace.p, tn * sizeof(double), hipMemcpyDeviceToHost, st));
        JTK_HIP_TRY(hipMemcpyAsync(&cs, s->d_state.as<ChunkState>() + ci, sizeof cs, hipMemcpyDeviceToHost, st));
        JTK_HIP_TRY(hipStreamSynchronize(st));
        JTK_HIP_TRY(hipGetLastError());
        if (cs.status != 0) return jtk_fail(cs.status, "jtk_lc_session_trace: the chunk failed when its chain ran again");
        trace_row(out, "RANGE\t%u..=%u", (unsigned)tv[0], (unsigned)tv[1]);                                 // :236
        const uint32_t nrec = std::min<uint32_t>((uint32_t)tv[2], 8u);
        for (uint32_t r = 0; r < nrec; r++) {
            const double *rec = tv.data() + 8 + 16 * r;
            const unsigned kk = (unsigned)rec[0];
            trace_row(out, "LK\t%u\t%s", kk, fx(rec[1], 3).c_str());                                        // :250
            trace_row(out, "LK\t%u\t%s\t%s\t%u", kk, fx(rec[1], 3).c_str(), fx(rec[2], 3).c_str(), (unsigned)rec[3]);  // :256
            if (rec[4] != 0.0) {                                                                            // :258-262
                std::string c = "COUNTS\t[";
                for (unsigned q = 0; q < kk && q < JTK_MAX_COPY; q++) c += (q ? ", " : "") + std::to_string((unsigned)rec[5 + q]);
                trace_row(out, "%s]", c.c_str());
            }
        }
    }
    *len = out.size();
    if (out.size() > cap) return jtk_fail(JTK_ERR_INVALID_ARG, "jtk_lc_session_trace: the text needs " + std::to_string(out.size()) + " bytes");
    if (!out.empty()) memcpy(text, out.data(), out.size());
    return JTK_OK;
}

// include/jtk_lc_debug.h: per chunk, the cycles of its chain and the proposals that could not be stepped over
int jtk_lc_debug_chain_profile(jtk_lc_session_t *s, uint64_t *cycles, uint32_t *events) {
    g_last_error.clear();
    if (!s) return jtk_fail(JTK_ERR_INVALID_ARG, "null session");
    JTK_HIP_TRY(hipSetDevice(s->device));
    std::vector<ChunkState> state(s->n_chunks);
    JTK_HIP_TRY(hipMemcpyAsync(state.data(), s->d_state.p, state.size() * sizeof(ChunkState), hipMemcpyDeviceToHost, s->stream));
    JTK_HIP_TRY(hipStreamSynchronize(s->stream));
    for (uint32_t c = 0; c < s->n_chunks; c++) {
        if (cycles) cycles[c] = state[c].chain_cycles;
        if (events) events[c] = state[c].chain_events;
    }
    return JTK_OK;
}
