// session_refit.hip -- the model refit of the stage preamble (model_tune.rs:96-156), and the two entry points that run the
// pair-HMM of a resident batch for its own sake: one pile-up's modification table and the likelihoods of the gains calibration.
#include <cmath>
#include <cstring>

#include "session_internal.h"

namespace {
const int FIT_COUNTS = 45;  // 9 transitions (M,I,D x M,I,D), mat_emit[16], ins_emit[20]

// M-step on summed counts: every row is divided by its sum; rows without mass keep the old values
void fit_mstep(const jtk_hmm_t &old, const double *cnt, jtk_hmm_t &out) {
    out = old;
    double *tr[3] = {&out.mat_mat, &out.ins_mat, &out.del_mat};
    for (int st = 0; st < 3; st++) {
        const double sum = (cnt[3 * st] + cnt[3 * st + 1]) + cnt[3 * st + 2];
        if (sum > 0.0)
            for (int q = 0; q < 3; q++) tr[st][q] = cnt[3 * st + q] / sum;
    }
    for (int x = 0; x < 4; x++) {
        const double *e = cnt + 9 + 4 * x;
        const double sum = ((e[0] + e[1]) + e[2]) + e[3];
        if (sum > 0.0)
            for (int q = 0; q < 4; q++) out.mat_emit[4 * x + q] = e[q] / sum;
    }
    for (int cx = 0; cx < 5; cx++) {
        const double *e = cnt + 25 + 4 * cx;
        const double sum = ((e[0] + e[1]) + e[2]) + e[3];
        if (sum > 0.0)
            for (int q = 0; q < 4; q++) out.ins_emit[4 * cx + q] = e[q] / sum;
    }
}

// The opening of a pass and one sweep of every read, as two tables of one segment each (session.hip: round_segment): the
// session at its opening, then in round 0.  The reads of wide bands take their own kernel, which is outside the table.
void queue_open_and_sweep(jtk_lc_session *s) {
    hipStream_t st = s->stream;
    RoundSegTable t;
    memset(&t, 0, sizeof t);
    t.n = 1;
    jtk_lc_session::RoundRequest rq;
    rq.open = 1;
    t.seg[0] = round_segment(s, rq);
    launch_reset_pass(st, t);
    launch_band_prep(st, t);
    rq.open = 0;  // round 0, every chunk
    t.seg[0] = round_segment(s, rq);
    t.seg[0].skip_le_radius = 0;  // overrides round_segment: no launch_phmm_pair here, phmm_kernel takes the narrow bands too
    launch_phmm(st, t, s->stripes->set(), s->n_waves, s->d_counter.as<uint32_t>(), &s->tk_phmm);
    if (s->n_wide_reads)
        launch_phmm_wide(st, s->n_reads, s->d_reads.as<ReadMeta>(), s->d_chunks.as<ChunkMeta>(), s->d_state.as<ChunkState>(), s->bufs,
                         s->d_ey.as<uint8_t>(), s->d_delta.as<uint64_t>(), s->d_hmm2.as<HmmDev>(),
                         s->d_wide_scratch.as<double>(), s->wide_stride, s->n_wide_waves, s->d_wide_counter.as<uint32_t>(), &s->tk_wide,
                         s->d_raw.as<double>(), s->d_rawG.as<int>(), s->d_lk.as<double>(), s->max_tmpl, s->max_read, 0,
                         s->max_wide_radius);
}
}  // namespace

// `rounds` x [ polish every training pile-up with HMMPolishConfig::new(band / 2, N, 0) (model_tune.rs:137-143), then one
// Baum-Welch step on all of them with the LARGEST band (fit_antidiagonal_par_multiple(&packs, bw / 2), :136,:144-151) ].
// Polishing and the expected counts run on the device; the M-step is a few dozen divisions on the host.
int jtk_lc_fit_model(const jtk_lc_params_t *params, size_t n_chunks, const jtk_lc_chunk_t *chunks, const uint8_t *tmpl_bases,
                     const uint8_t *read_bases, const uint64_t *read_off, const uint8_t *ops, const uint64_t *ops_off,
                     const uint8_t *strand, uint32_t rounds, jtk_hmm_t *forward_out, jtk_hmm_t *reverse_out, int device) {
    g_last_error.clear();
    if (!params || !forward_out || !reverse_out || !chunks || !read_off || !ops_off || !strand)
        return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    size_t n_reads = 0, tmpl_total = 0;
    uint32_t max_bw = 0;
    for (size_t c = 0; c < n_chunks; c++) {
        n_reads += chunks[c].n_reads;
        tmpl_total += (size_t)chunks[c].tmpl_len;
        max_bw = std::max<uint32_t>(max_bw, (uint32_t)std::ceil((double)chunks[c].tmpl_len * params->band_frac));
    }
    if (n_chunks == 0 || n_reads == 0) return jtk_fail(JTK_ERR_INVALID_ARG, "no training pile-up");  // assert!, model_tune.rs:135
    if (max_bw / 2 > JTK_WIDE_MAX_RADIUS) return jtk_fail(JTK_ERR_UNSUPPORTED, "band radius > 255");
    jtk_lc_params_t cur = *params;
    if (cur.gains.max_homopolymer_len == 0) cur.gains.max_homopolymer_len = 1;  // the gains play no part in the refit
    // working copies: consensus and ops change from round to round; band_width stays that of the unpolished chunk (:123)
    std::vector<jtk_lc_chunk_t> ch(chunks, chunks + n_chunks);
    std::vector<uint8_t> cons(2 * tmpl_total + 64 * n_chunks + 64), cops(2 * (size_t)ops_off[n_reads] + 64 * n_reads + 64);
    std::vector<uint64_t> coff(n_chunks + 1), ooff(ops_off, ops_off + n_reads + 1);
    std::vector<ChunkExtra> extra(n_chunks);
    memcpy(cops.data(), ops, (size_t)ops_off[n_reads]);
    uint64_t o = 0;
    for (size_t c = 0; c < n_chunks; c++) {
        coff[c] = o;
        memcpy(cons.data() + o, tmpl_bases + chunks[c].tmpl_off, (size_t)chunks[c].tmpl_len);
        o += chunks[c].tmpl_len;
        memset(&extra[c], 0, sizeof extra[c]);
        extra[c].radius = (uint32_t)std::ceil((double)chunks[c].tmpl_len * params->band_frac) / 2;
        ch[c].copy_num = 1;
    }
    coff[n_chunks] = o;
    std::vector<uint8_t> cons2(cons.size()), cops2(cops.size());
    std::vector<uint64_t> coff2(n_chunks + 1), ooff2(n_reads + 1);
    std::vector<jtk_lc_result_t> res(n_chunks);
    std::vector<double> counts((size_t)n_reads * FIT_COUNTS), lks(n_reads);
    for (uint32_t round = 0; round < rounds; round++) {
        for (size_t c = 0; c < n_chunks; c++) {
            ch[c].tmpl_off = coff[c];
            ch[c].tmpl_len = coff[c + 1] - coff[c];
        }
        jtk_lc_session_t *s = nullptr;
        int rc = session_create_ex(&cur, n_chunks, ch.data(), cons.data(), read_bases, read_off, cops.data(), ooff.data(), strand,
                                   1, device, extra.data(), 0 /* ignore_edge, model_tune.rs:140 */, &s, true);
        if (rc) return rc;
        std::unique_ptr<jtk_lc_session> guard(s);
        s->resume_rng = false;
        if ((rc = run_batch(s, 0))) return rc;
        rc = jtk_lc_session_fetch(s, nullptr, nullptr, res.data(), cons2.data(), coff2.data(), cons2.size(), cops2.data(),
                                  ooff2.data(), cops2.size());
        if (rc) return rc;  // a training pile-up that fails fails the fit (the reference would panic)
        // ---- E-step on the polished pile-ups, every read with the largest band's radius
        {
            std::vector<ChunkMeta> wide(s->h_chunks);
            for (auto &cm : wide) {
                cm.radius = max_bw / 2;
                cm.take_num = 0;
            }
            // (checked before anything is allocated or queued: an early return must not hand a block with a pending memset
            // back to the pool)
            const size_t lds = phmm_counts_lds_bytes(s->max_tmpl, s->max_read, max_bw / 2);
            if (lds > 160 * 1024) return jtk_fail(JTK_ERR_UNSUPPORTED, "template + read too long for the LDS staging of phmm_counts_kernel");
            DevPtr d_wide, d_counts, d_lk, d_scratch, d_counter;
            if ((rc = dev_upload(s, d_wide, wide))) return rc;
            if ((rc = dev_alloc<double>(d_counts, (size_t)n_reads * FIT_COUNTS))) return rc;
            if ((rc = dev_alloc<double>(d_lk, n_reads))) return rc;
            if ((rc = dev_alloc<uint32_t>(d_counter, 4))) return rc;
            JTK_HIP_TRY(hipMemsetAsync(d_counter.p, 0, 4 * sizeof(uint32_t), s->stream));  // a fresh ticket counter (once per round)
            uint32_t tk_counts = 0;
            hipDeviceProp_t prop;
            JTK_HIP_TRY(hipGetDeviceProperties(&prop, device));
            const uint64_t stride = phmm_counts_scratch_doubles(s->max_tmpl, s->max_read, max_bw / 2);
            uint64_t waves = std::min<uint64_t>(n_reads, (uint64_t)prop.multiProcessorCount * 2);
            waves = std::max<uint64_t>(1, std::min<uint64_t>(waves, (32ull << 30) / (stride * 8)));
            if ((rc = dev_alloc<double>(d_scratch, stride * waves))) return rc;
            launch_phmm_counts(s->stream, s->n_reads, s->d_reads.as<ReadMeta>(), d_wide.as<ChunkMeta>(),
                               s->d_state.as<ChunkState>(), s->bufs, s->d_ey.as<uint8_t>(), s->d_delta.as<uint64_t>(),
                               s->d_hmm2.as<HmmDev>(), d_scratch.as<double>(), stride, (uint32_t)waves,
                               d_counter.as<uint32_t>(), &tk_counts, d_counts.as<double>(), d_lk.as<double>(), s->max_tmpl,
                               s->max_read, max_bw / 2);
            JTK_HIP_TRY(hipMemcpyAsync(counts.data(), d_counts.p, counts.size() * 8, hipMemcpyDeviceToHost, s->stream));
            JTK_HIP_TRY(hipMemcpyAsync(lks.data(), d_lk.p, lks.size() * 8, hipMemcpyDeviceToHost, s->stream));
            JTK_HIP_TRY(hipStreamSynchronize(s->stream));
            JTK_HIP_TRY(hipGetLastError());
        }
        double sum[2][FIT_COUNTS];
        memset(sum, 0, sizeof sum);
        for (size_t g = 0; g < n_reads; g++) {  // reads in order, as the oracle adds them
            const int st = strand[g] ? 0 : 1;
            for (int k = 0; k < FIT_COUNTS; k++) sum[st][k] += counts[g * FIT_COUNTS + k];
        }
        jtk_hmm_t nf, nr;
        fit_mstep(cur.forward, sum[0], nf);
        fit_mstep(cur.reverse, sum[1], nr);
        cur.forward = nf;
        cur.reverse = nr;
        cons.swap(cons2);
        cops.swap(cops2);
        coff.swap(coff2);
        ooff.swap(ooff2);
    }
    *forward_out = cur.forward;
    *reverse_out = cur.reverse;
    return 0;
}

int jtk_lc_modification_table(const jtk_lc_params_t *params, const uint8_t *tmpl, uint64_t tmpl_len,
                              uint32_t n_reads, const uint8_t *read_bases, const uint64_t *read_off,
                              const uint8_t *ops, const uint64_t *ops_off, const uint8_t *strand, double *table,
                              double *lk, int device) {
    g_last_error.clear();
    if (!table || !lk) return jtk_fail(JTK_ERR_INVALID_ARG, "null output");
    jtk_lc_chunk_t ch;
    memset(&ch, 0, sizeof ch);
    ch.chunk_id = 0;
    ch.copy_num = 2;
    ch.n_reads = n_reads;
    ch.tmpl_off = 0;
    ch.tmpl_len = tmpl_len;
    ch.read_first = 0;
    jtk_lc_session_t *s = nullptr;
    int rc = jtk_lc_session_create(params, 1, &ch, tmpl, read_bases, read_off, ops, ops_off, strand, 2, device, &s);
    if (rc) return rc;
    std::unique_ptr<jtk_lc_session> guard(s);
    hipStream_t st = s->stream;
    ChunkState *state = s->d_state.as<ChunkState>();
    queue_open_and_sweep(s);
    launch_finalize(st, s->n_reads, s->d_reads.as<ReadMeta>(), s->d_chunks.as<ChunkMeta>(), state,
                    s->d_hmm2.as<HmmDev>(), s->d_raw.as<double>(), s->d_rawG.as<int>(), s->d_lk.as<double>(), s->max_tmpl, 0);
    ChunkState cs;
    JTK_HIP_TRY(hipMemcpyAsync(&cs, state, sizeof cs, hipMemcpyDeviceToHost, st));
    JTK_HIP_TRY(hipMemcpyAsync(lk, s->d_lk.p, (size_t)n_reads * 8, hipMemcpyDeviceToHost, st));
    const size_t cols = (size_t)JTK_NUM_ROW * (tmpl_len + 1);
    for (uint32_t r = 0; r < n_reads; r++)
        JTK_HIP_TRY(hipMemcpyAsync(table + (size_t)r * cols, s->d_raw.as<double>() + s->h_reads[r].table_off, cols * 8,
                               hipMemcpyDeviceToHost, st));
    JTK_HIP_TRY(hipStreamSynchronize(st));
    JTK_HIP_TRY(hipGetLastError());
    if (cs.status != 0) return jtk_fail(cs.status, "modification table failed (ops mismatch or unsupported band)");
    return 0;
}

// log P(read | template) of every read of a resident batch with a fixed band radius: band_prep + the forward
// sweep of phmm_kernel (the backward sweep runs too and is ignored; these batches are tiny).  Used by the
// gains calibration (gains.hip), which evaluates kiley's likelihood_antidiagonal_bootstrap 180,000 times.
int jtk_internal_likelihoods(const jtk_lc_params_t *params, size_t n_chunks, const jtk_lc_chunk_t *chunks,
                             const uint8_t *tmpl_bases, const uint8_t *read_bases, const uint64_t *read_off,
                             const uint8_t *ops, const uint64_t *ops_off, const uint8_t *strand, uint32_t radius,
                             int device, double *lk_out) {
    std::vector<ChunkExtra> extra(n_chunks);
    for (auto &e : extra) {
        memset(&e, 0, sizeof e);
        e.radius = radius;
    }
    jtk_lc_session_t *s = nullptr;
    uint32_t stride = 1;
    for (size_t c = 0; c < n_chunks; c++) stride = std::max(stride, std::min<uint32_t>(chunks[c].copy_num, JTK_MAX_COPY));
    int rc = session_create_ex(params, n_chunks, chunks, tmpl_bases, read_bases, read_off, ops, ops_off, strand, stride, device,
                               extra.data(), 0, &s);
    if (rc) return rc;
    std::unique_ptr<jtk_lc_session> guard(s);
    hipStream_t st = s->stream;
    ChunkState *state = s->d_state.as<ChunkState>();
    queue_open_and_sweep(s);
    std::vector<ChunkState> cs(n_chunks);
    JTK_HIP_TRY(hipMemcpyAsync(cs.data(), state, cs.size() * sizeof(ChunkState), hipMemcpyDeviceToHost, st));
    JTK_HIP_TRY(hipMemcpyAsync(lk_out, s->d_lk.p, (size_t)s->n_reads * 8, hipMemcpyDeviceToHost, st));
    JTK_HIP_TRY(hipStreamSynchronize(st));
    JTK_HIP_TRY(hipGetLastError());
    for (const ChunkState &c : cs)
        if (c.status != 0) return jtk_fail(c.status, "likelihood batch failed (ops mismatch or unsupported band)");
    return 0;
}
