// session_features.hip -- jtk_lc_cluster_features: the chain alone, on feature matrices the caller already holds.
#include <cstring>

#include "session_internal.h"
#include "session_plan.h"

int jtk_lc_cluster_features(const jtk_lc_params_t *params, size_t n_chunks, const jtk_lc_feature_chunk_t *chunks,
                            const double *variants, const uint32_t *variant_type, uint32_t *label, double *log_post,
                            uint32_t post_stride, jtk_lc_result_t *result, int device) {
    g_last_error.clear();
    if (!params || (n_chunks && (!chunks || !variants || !variant_type || !label || !log_post || !result)))
        return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    int rc = jtk_require_device(device);
    if (rc) return rc;
    // declared before the session: destructors run in reverse order, so the session's (which synchronises its stream)
    // runs before these blocks go back to the pool on every early return
    DevPtr d_params, d_chunks, d_state, d_var, d_vt, d_vtoff, d_label, d_post, d_lg, d_lgoff;
    jtk_lc_session sess;
    jtk_lc_session *s = &sess;
    s->device = device;
    JTK_HIP_TRY(hipStreamCreate(&s->stream));
    std::vector<ChunkMeta> cms(n_chunks);
    std::vector<ChunkState> sts(n_chunks);
    std::vector<uint64_t> vt_off(n_chunks), lg_off(n_chunks);
    uint64_t n_reads = 0, n_var = 0, n_vt = 0, lgo = 0;
    uint32_t max_k = 2;
    if ((rc = check_contiguous(chunks, n_chunks, &n_reads))) return rc;
    for (size_t c = 0; c < n_chunks; c++) {
        const jtk_lc_feature_chunk_t &fc = chunks[c];
        if (fc.copy_num > max_k && fc.copy_num <= JTK_MAX_COPY) max_k = fc.copy_num;
        memset(&cms[c], 0, sizeof(ChunkMeta));
        memset(&sts[c], 0, sizeof(ChunkState));
        cms[c].chunk_id = fc.chunk_id;
        cms[c].copy_num = fc.copy_num;
        cms[c].n_reads = fc.n_reads;
        cms[c].read_first = (uint32_t)fc.read_first;
        cms[c].feat_off = fc.var_off;
        cms[c].local_coverage = fc.local_coverage;
        sts[c].dim = fc.dim;
        sts[c].k = 1;
        if (fc.dim > JTK_MAX_DIM || fc.copy_num > JTK_MAX_COPY) sts[c].status = JTK_ERR_UNSUPPORTED;
        else if (fc.copy_num > post_stride)  // a posterior row holds up to copy_num entries
            return jtk_fail(JTK_ERR_INVALID_ARG, "post_stride smaller than a chunk's copy_num");
        vt_off[c] = fc.vt_off;
        lg_off[c] = lgo;
        lgo += (uint64_t)fc.n_reads * (JTK_MAX_COPY + 1);
        if (fc.var_off + (uint64_t)fc.n_reads * fc.dim > n_var) n_var = fc.var_off + (uint64_t)fc.n_reads * fc.dim;
        if (fc.vt_off + fc.dim > n_vt) n_vt = fc.vt_off + fc.dim;
    }
    // the two launches: the table-driven kernels on what fits a CU's LDS, mcmc_kernel_huge on the rest (session_plan.h)
    std::vector<uint8_t> failed(n_chunks);
    for (size_t c = 0; c < n_chunks; c++) failed[c] = sts[c].status != 0;
    FeatureChainPlan fp;
    plan_feature_chain(n_chunks, chunks, failed, max_k, JTK_CU_LDS_BYTES, fp);
    std::vector<jtk_lc_params_t> pv(1, *params);
    std::vector<double> varv(variants, variants + n_var);
    std::vector<uint32_t> vtv(variant_type, variant_type + 2 * n_vt);
    if ((rc = dev_upload(s, d_params, pv))) return rc;
    if ((rc = dev_upload(s, d_chunks, cms))) return rc;
    if ((rc = dev_upload(s, d_state, sts))) return rc;
    if ((rc = dev_upload(s, d_var, varv))) return rc;
    if ((rc = dev_upload(s, d_vt, vtv))) return rc;
    if ((rc = dev_upload(s, d_vtoff, vt_off))) return rc;
    if ((rc = dev_upload(s, d_lgoff, lg_off))) return rc;
    if ((rc = dev_alloc<uint32_t>(d_label, n_reads))) return rc;
    if ((rc = dev_alloc<double>(d_post, n_reads * post_stride))) return rc;
    if ((rc = dev_alloc<double>(d_lg, lgo))) return rc;
    DevPtr d_split, d_order, d_ws, d_wsoff;  // light / general chunk lists of the chain launch; the two launches' chunk lists
    if ((rc = dev_upload(s, d_order, fp.order))) return rc;
    if (fp.n_ws) {
        if ((rc = dev_alloc<uint8_t>(d_ws, fp.ws_bytes))) return rc;
        if ((rc = dev_upload(s, d_wsoff, fp.ws_off))) return rc;
    }
    tstart(s, JTK_K_MCMC);  // (the session owns the events: no return below leaks one)
    if ((rc = dev_alloc<uint32_t>(d_split, 2 * n_chunks + 8))) return rc;
    if (fp.n_lds && launch_mcmc(s->stream, fp.n_lds, d_chunks.as<ChunkMeta>(), d_state.as<ChunkState>(),
                    d_params.as<jtk_lc_params_t>(), d_var.as<double>(), d_vt.as<uint32_t>(), d_vtoff.as<uint64_t>(), 1,
                    d_label.as<uint32_t>(), d_post.as<double>(), post_stride, d_lg.as<double>(), d_lgoff.as<uint64_t>(),
                    fp.lds.n, fp.lds.d, max_k, nullptr, d_order.as<uint32_t>(), d_split.as<uint32_t>(), nullptr, nullptr, nullptr) != 0)
        return jtk_fail(JTK_ERR_INTERNAL, "the chain kernel could not be launched (jump table upload failed)");
    if (fp.n_ws &&
        launch_mcmc_huge(s->stream, fp.n_ws, d_chunks.as<ChunkMeta>(), d_state.as<ChunkState>(),
                         d_params.as<jtk_lc_params_t>(), d_var.as<double>(), d_vt.as<uint32_t>(), d_vtoff.as<uint64_t>(), 1,
                         d_label.as<uint32_t>(), d_post.as<double>(), post_stride, d_lg.as<double>(), d_lgoff.as<uint64_t>(), fp.ws.n, fp.ws.d,
                         max_k, nullptr, d_order.as<uint32_t>() + fp.n_lds, d_ws.as<uint8_t>(), d_wsoff.as<uint64_t>()) != 0)
        return jtk_fail(JTK_ERR_INTERNAL, "the chain kernel could not be launched (jump table upload failed)");
    tstop(s);
    JTK_HIP_TRY(hipMemcpyAsync(sts.data(), d_state.p, sts.size() * sizeof(ChunkState), hipMemcpyDeviceToHost, s->stream));
    JTK_HIP_TRY(hipMemcpyAsync(label, d_label.p, n_reads * 4, hipMemcpyDeviceToHost, s->stream));
    JTK_HIP_TRY(hipMemcpyAsync(log_post, d_post.p, n_reads * post_stride * 8, hipMemcpyDeviceToHost, s->stream));
    JTK_HIP_TRY(hipStreamSynchronize(s->stream));
    JTK_HIP_TRY(hipGetLastError());
    float ms = 0;
    (void)hipEventElapsedTime(&ms, s->timers.back().a, s->timers.back().b);
    memset(&g_timing, 0, sizeof g_timing);
    g_timing.total_ms = ms;
    g_timing.kernel_ms[JTK_K_MCMC] = ms;
    g_timing.kernel_launches[JTK_K_MCMC] = 1;
    int any_fail = 0;
    for (size_t c = 0; c < n_chunks; c++) {
        result[c].score = sts[c].status == 0 ? sts[c].score : 0.0;
        result[c].cluster_num = sts[c].status == 0 ? sts[c].k : 1;
        result[c].status = sts[c].status;
        result[c].polish_rounds = 0;
        result[c].n_variants = sts[c].dim;
        if (sts[c].status != 0) any_fail = 1;
    }
    return any_fail ? jtk_fail(JTK_ERR_CHUNK_FAILED, "at least one chunk failed; see result[].status") : 0;
}
