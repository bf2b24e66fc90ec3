// encode_nodes.hip -- jtk_lc_encode_nodes: `encode_node` with `fine_mapping` and `fit_query_by_edlib`
// (haplotyper/src/encode/deletion_fill.rs:451-566) for a batch of trials, restated as it stands.  Per trial:
//   host    the lower-bound filter (:461-465, f64) and, at the end, the verdict (:501-505, f64 from integer counts)
//   device  encode_window_kernel: the window of the raw read, reverse-complemented when the node is reverse, upper-cased (:467-472)
//   host    jtk_lc_align_reads_mode, infix, the read free: edlib's placement of the consensus in the window (:544-547); its ops
//           pass through the host once and come back as the first guide, padded with Dels over the window's ends (:548-550)
//   device  two passes of the guided aligner of guided.hip, x = window, y = consensus (:553-554); encode_next_kernel makes the
//           second pass's descriptors from the first one's ops
//           encode_fit_kernel: Ins and Del swapped, the Ins runs at both ends trimmed (:556-564, :595-609), the match and
//           op counts (:501-502), edge_identity's four counts (:568-592), and the descriptors of the third pass
//           the third pass, x = the chunk's sequence, y = the trimmed window (:526)
// Everything between the upload of the first guides and the copy back of the results is enqueued on one stream without a wait.
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "device_common.h"
#include "encode_window.h"
#include "guided_internal.h"
#include "jtk_lc_debug.h"
#include "wave_util.h"

namespace {

constexpr uint32_t EN_EDGE_LEN = 100;   // deletion_fill.rs:9
constexpr double EN_EDGE_BOUND = 0.5;   // :7
constexpr int EN_MATCH = 2, EN_MISMATCH = -6, EN_OPEN = -5, EN_EXT = -1;  // ALN_PARAMETER (haplotyper/src/lib.rs)

struct EnFit {
    uint32_t trim_head, trim_tail, mat_num, ops_len, head_match, head_len, tail_match, tail_len;
};
struct EnTrial {   // what encode_fit_kernel needs besides the second pass's results
    uint64_t win_off, chunk_off;
    uint32_t win_len, cons_len, chunk_len, band;
};

// the second pass: the same sequences, guided by the first pass's ops
__global__ void __launch_bounds__(256) encode_next_kernel(uint32_t n, const jtk_guided_pair_t *in, const uint64_t *slot_end, const uint32_t *nops,
                                                          jtk_guided_pair_t *out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    jtk_guided_pair_t p = in[t];
    p.guide_off = slot_end[t] - nops[t];
    p.guide_len = nops[t];
    out[t] = p;
}

// One wave per trial, on the second pass's ops (in their slot, rewritten in place with Ins and Del swapped).
__global__ void __launch_bounds__(256) encode_fit_kernel(uint32_t n, const EnTrial *trials, const int32_t *status, uint8_t *slots,
                                                         const uint64_t *slot_end, const uint32_t *nops, EnFit *fit, jtk_guided_pair_t *next) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t t = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (t >= n) return;
    const EnTrial tr = trials[t];
    EnFit f{};
    jtk_guided_pair_t p{};
    if (status[t] == 0) {
        const uint32_t len = nops[t];
        const uint64_t at = slot_end[t] - len;
        uint8_t *ops = slots + at;
        // ---- the swap; the first and the last op that is no Ins
        uint32_t first = len, last_plus = 0;
        for (uint32_t q = lane; q < len; q += 64) {
            uint8_t op = ops[q];
            op = op == JTK_OP_INS ? JTK_OP_DEL : op == JTK_OP_DEL ? JTK_OP_INS : op;
            ops[q] = op;
            if (op != JTK_OP_INS) {
                first = q < first ? q : first;
                last_plus = q + 1;
            }
        }
        jtk_wave_sync();  // the counts below read bytes that other lanes have just rewritten
        for (uint32_t o = 32; o; o >>= 1) {
            const uint32_t u = __shfl_xor(first, o, 64), v = __shfl_xor(last_plus, o, 64);
            first = u < first ? u : first;
            last_plus = v > last_plus ? v : last_plus;
        }
        // trim_head_tail_insertion pops the tail first: ops that are all Ins count as tail
        f.trim_tail = len - last_plus;
        f.trim_head = last_plus ? first : 0;
        f.ops_len = len - f.trim_tail - f.trim_head;
        // ---- the counts; rpos = consensus bases consumed up to and including the op (edge_identity :568-592)
        const uint32_t head_end = EN_EDGE_LEN < tr.cons_len ? EN_EDGE_LEN : tr.cons_len;
        const uint32_t tail_start = tr.cons_len > EN_EDGE_LEN ? tr.cons_len - EN_EDGE_LEN : 0;
        uint32_t rpos_before = 0;
        for (uint32_t base = 0; base < f.ops_len; base += 64) {
            const uint32_t q = base + lane;
            const bool active = q < f.ops_len;
            const uint8_t op = active ? ops[f.trim_head + q] : (uint8_t)JTK_OP_INS;
            const uint64_t consumes = __ballot(active && op != JTK_OP_INS);
            const uint32_t rpos = rpos_before + (uint32_t)__popcll(consumes & (~0ull >> (63 - lane)));
            const bool is_match = active && op == JTK_OP_MATCH;
            const bool in_head = active && rpos < head_end, in_tail = active && tail_start <= rpos;
            f.mat_num += (uint32_t)__popcll(__ballot(is_match));
            f.head_len += (uint32_t)__popcll(__ballot(in_head));
            f.head_match += (uint32_t)__popcll(__ballot(in_head && is_match));
            f.tail_len += (uint32_t)__popcll(__ballot(in_tail));
            f.tail_match += (uint32_t)__popcll(__ballot(in_tail && is_match));
            rpos_before += (uint32_t)__popcll(consumes);
        }
        // ---- the third pass: the chunk's sequence against what is left of the window
        p.x_off = tr.chunk_off;
        p.x_len = tr.chunk_len;
        p.y_off = tr.win_off + f.trim_head;
        p.y_len = tr.win_len - f.trim_head - f.trim_tail;
        p.guide_off = at + f.trim_head;
        p.guide_len = f.ops_len;
        p.radius = tr.band;
    }
    if (lane == 0) {
        fit[t] = f;
        next[t] = p;
    }
}

thread_local double g_encode_timing[8];

uint32_t band_of(uint32_t window_len, double sim_thr) {  // ((len as f64 * sim_thr * 0.3).ceil() as usize).max(10), :552
    const double v = std::ceil((double)window_len * sim_thr * 0.3);
    const uint32_t b = !(v > 0.0) ? 0u : v >= 4294967295.0 ? 0xffffffffu : (uint32_t)v;  // `as usize` saturates; NaN gives 0
    return b > 10u ? b : 10u;
}

}  // namespace

extern "C" void jtk_lc_debug_encode_timing(double *out) {
    if (out) std::memcpy(out, g_encode_timing, sizeof(g_encode_timing));
}

extern "C" int jtk_lc_encode_nodes(size_t n_trials, const jtk_encode_trial_t *trials, const uint8_t *read_bases, const uint8_t *cons_bases,
                                   const uint8_t *chunk_bases, jtk_encode_result_t *result, uint8_t *ops_out, uint64_t *ops_out_off,
                                   uint64_t ops_cap, int device) {
    g_last_error.clear();
    if (!ops_out_off || (n_trials && (!trials || !read_bases || !cons_bases || !chunk_bases || !result))) return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    if (n_trials >= 0x7fffffffu) return jtk_fail(JTK_ERR_UNSUPPORTED, "2^31 - 1 trials or more");
    for (size_t t = 0; t < n_trials; t++) {
        if (trials[t].start >= trials[t].end) return jtk_fail(JTK_ERR_INVALID_ARG, "a window with start >= end");
        if (!trials[t].cons_len || !trials[t].chunk_len) return jtk_fail(JTK_ERR_INVALID_ARG, "an empty consensus or chunk sequence");
    }
    if (int rc = jtk_require_device(device)) return rc;
    // ---- 1. the lower-bound filter
    std::vector<uint32_t> live;  // the trials that go on, in order
    for (size_t t = 0; t < n_trials; t++) {
        const jtk_encode_trial_t &tr = trials[t];
        jtk_encode_result_t &r = result[t];
        std::memset(&r, 0, sizeof(r));
        const uint32_t wl = tr.end - tr.start;
        const uint32_t lower = tr.cons_len > wl ? tr.cons_len - wl : 0;
        const double diff_lower_bound = (double)lower / (double)tr.cons_len;
        r.band = band_of(wl, tr.sim_thr);
        r.position_from_start = tr.start;
        if (tr.sim_thr < diff_lower_bound) {
            r.verdict = JTK_ENCODE_LOWER_BOUND;
            continue;
        }
        r.verdict = JTK_ENCODE_REJECTED;
        live.push_back((uint32_t)t);
    }
    const size_t n = live.size();
    std::memset(g_encode_timing, 0, sizeof(g_encode_timing));
    g_encode_timing[0] = (double)n;
    for (size_t t = 0; t <= n_trials; t++) ops_out_off[t] = 0;
    if (!n) return 0;
    // ---- 2. the windows
    std::vector<EnWindow> wins(n);
    std::vector<uint64_t> win_off(n + 1, 0);
    uint64_t cons_bytes = 0, chunk_bytes = 0;
    for (size_t k = 0; k < n; k++) {
        const jtk_encode_trial_t &tr = trials[live[k]];
        wins[k].off = win_off[k];
        wins[k].len = tr.end - tr.start;
        wins[k].is_forward = tr.is_forward ? 1u : 0u;
        win_off[k + 1] = win_off[k] + wins[k].len;
        cons_bytes = std::max(cons_bytes, tr.cons_off + tr.cons_len);
        chunk_bytes = std::max(chunk_bytes, tr.chunk_off + tr.chunk_len);
    }
    std::vector<uint8_t> raw(win_off[n]), windows(win_off[n]);
    for (size_t k = 0; k < n; k++) {
        const jtk_encode_trial_t &tr = trials[live[k]];
        std::memcpy(raw.data() + win_off[k], read_bases + tr.read_off + tr.start, wins[k].len);
    }
    DevStream s;
    JTK_HIP_TRY(s.create());
    const hipStream_t st = s.st;
    DevArr<EnWindow> d_wins;
    DevArr<uint8_t> d_raw, d_win, d_cons, d_chunk;
    DevArr<uint32_t> d_flags;
    {
        int rc;
        const std::vector<uint8_t> cons_v(cons_bases, cons_bases + cons_bytes), chunk_v(chunk_bases, chunk_bases + chunk_bytes);
        if ((rc = d_wins.upload(wins, st)) || (rc = d_raw.upload(raw, st)) || (rc = d_cons.upload(cons_v, st)) || (rc = d_chunk.upload(chunk_v, st)))
            return jtk_fail(rc, "device upload failed");
        JTK_HIP_TRY(d_win.alloc(win_off[n]));
        JTK_HIP_TRY(d_flags.alloc(1));
        JTK_HIP_TRY(d_flags.zero(1, st));
        encode_window_kernel<<<(uint32_t)n, 256, 0, st>>>((uint32_t)n, d_wins.cget(), d_raw.cget(), d_win.get(), d_flags.get());
        JTK_HIP_TRY(hipGetLastError());
        uint32_t flags = 0;
        JTK_HIP_TRY(d_win.download(windows.data(), win_off[n], st));
        JTK_HIP_TRY(d_flags.download(&flags, 1, st));
        JTK_HIP_TRY(hipStreamSynchronize(st));
        JTK_HIP_TRY(hipGetLastError());
        if (flags) return jtk_fail(JTK_ERR_INVALID_ARG, "non-ACGT base in a window");
        for (size_t k = 0; k < n; k++) {  // (the consensus is looked at by the infix alignment)
            const jtk_encode_trial_t &tr = trials[live[k]];
            for (uint64_t q = tr.chunk_off; q < tr.chunk_off + tr.chunk_len; q++)
                if (chunk_v[q] != 'A' && chunk_v[q] != 'C' && chunk_v[q] != 'G' && chunk_v[q] != 'T')
                    return jtk_fail(JTK_ERR_INVALID_ARG, "non-ACGT base in a chunk sequence");
        }
    }
    // ---- 3. the infix alignment of every consensus into its window, and the first guides
    std::vector<int32_t> st_v(n, 0);
    std::vector<uint8_t> guide;
    std::vector<jtk_guided_pair_t> pairs(n);
    {
        std::vector<jtk_lc_chunk_t> chunks(n);
        uint64_t cap = 0;
        for (size_t k = 0; k < n; k++) {
            const jtk_encode_trial_t &tr = trials[live[k]];
            chunks[k] = jtk_lc_chunk_t{0, 0, 1, tr.cons_off, tr.cons_len, k};
            cap += (uint64_t)tr.cons_len + wins[k].len;
        }
        std::vector<uint8_t> e_ops(cap + 1);
        std::vector<uint64_t> e_off(n + 1);
        std::vector<uint32_t> dist(n), e_start(n), e_end(n);
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = jtk_lc_align_reads_mode(n, chunks.data(), cons_bases, windows.data(), win_off.data(), JTK_ALIGN_INFIX, JTK_ALIGN_FREE_READ, 0,
                                               e_ops.data(), e_off.data(), cap, dist.data(), e_start.data(), e_end.data(), st_v.data(), device);
        g_encode_timing[7] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (rc && rc != JTK_ERR_CHUNK_FAILED) return rc;
        g_last_error.clear();  // a refused trial is reported at the end
        guide.reserve(cap);
        for (size_t k = 0; k < n; k++) {
            const jtk_encode_trial_t &tr = trials[live[k]];
            jtk_guided_pair_t &p = pairs[k];
            p.x_off = win_off[k];
            p.x_len = wins[k].len;
            p.y_off = tr.cons_off;
            p.y_len = tr.cons_len;
            p.guide_off = guide.size();
            p.radius = result[live[k]].band;
            if (!st_v[k]) {  // in the guided orientation the window is x: a window base without a consensus base is a Del
                guide.insert(guide.end(), e_start[k], (uint8_t)JTK_OP_DEL);
                for (uint64_t q = e_off[k]; q < e_off[k + 1]; q++)
                    guide.push_back(e_ops[q] == JTK_OP_INS ? (uint8_t)JTK_OP_DEL : e_ops[q] == JTK_OP_DEL ? (uint8_t)JTK_OP_INS : e_ops[q]);
                guide.insert(guide.end(), wins[k].len - e_end[k], (uint8_t)JTK_OP_DEL);
            }
            p.guide_len = (uint32_t)(guide.size() - p.guide_off);
        }
    }
    // ---- 4. the three guided passes and what lies between them
    std::vector<uint32_t> wlen(n), clen(n), klen(n), band(n);
    std::vector<uint64_t> slot_end12(n), slot_end3(n);
    std::vector<EnTrial> en(n);
    uint64_t s12 = 0, s3 = 0;
    for (size_t k = 0; k < n; k++) {
        const jtk_encode_trial_t &tr = trials[live[k]];
        wlen[k] = wins[k].len;
        clen[k] = tr.cons_len;
        klen[k] = tr.chunk_len;
        band[k] = pairs[k].radius;
        if (wlen[k] > 32000 || klen[k] > 32000) st_v[k] = JTK_ERR_UNSUPPORTED;  // (the infix alignment has refused a longer consensus)
        s12 += (uint64_t)wlen[k] + clen[k];
        s3 += (uint64_t)klen[k] + wlen[k];
        slot_end12[k] = s12;
        slot_end3[k] = s3;
        en[k] = EnTrial{win_off[k], tr.chunk_off, wlen[k], clen[k], klen[k], band[k]};
    }
    DevArr<jtk_guided_pair_t> d_pairs1, d_pairs2, d_pairs3;
    DevArr<uint8_t> d_guide, d_slots1, d_slots2, d_slots3;
    DevArr<uint64_t> d_end12, d_end3;
    DevArr<EnTrial> d_en;
    DevArr<EnFit> d_fit;
    DevArr<int32_t> d_status, d_score[3];
    DevArr<uint32_t> d_start[3], d_endv[3], d_nops[3];
    {
        int rc;
        if ((rc = d_pairs1.upload(pairs, st)) || (rc = d_guide.upload(guide, st)) || (rc = d_status.upload(st_v, st)) || (rc = d_end12.upload(slot_end12, st)) ||
            (rc = d_end3.upload(slot_end3, st)) || (rc = d_en.upload(en, st)))
            return jtk_fail(rc, "device upload failed");
    }
    JTK_HIP_TRY(d_pairs2.alloc(n));
    JTK_HIP_TRY(d_pairs3.alloc(n));
    JTK_HIP_TRY(d_fit.alloc(n));
    JTK_HIP_TRY(d_slots1.alloc(s12 + 1));
    JTK_HIP_TRY(d_slots2.alloc(s12 + 1));
    JTK_HIP_TRY(d_slots3.alloc(s3 + 1));
    for (int q = 0; q < 3; q++) {
        JTK_HIP_TRY(d_score[q].alloc(n));
        JTK_HIP_TRY(d_start[q].alloc(n));
        JTK_HIP_TRY(d_endv[q].alloc(n));
        JTK_HIP_TRY(d_nops[q].alloc(n));
        JTK_HIP_TRY(d_score[q].zero(n, st));
        JTK_HIP_TRY(d_nops[q].zero(n, st));
    }
    GuidedRun run[3];
    GuidedArea area;  // the passes run behind each other: one work area, sized for the largest of them before the first starts
    GuidedBatch b;
    b.n = n;
    b.infix = 1;
    b.match = EN_MATCH;
    b.mismatch = EN_MISMATCH;
    b.gap_open = EN_OPEN;
    b.gap_ext = EN_EXT;
    b.h_radius = band.data();
    b.d_status = d_status.get();
    auto outputs = [&](int q) {
        b.d_score = d_score[q].get();
        b.d_start = d_start[q].get();
        b.d_end = d_endv[q].get();
        b.d_nops = d_nops[q].get();
    };
    b.h_xlen = wlen.data();
    b.h_ylen = clen.data();
    if (int rc = guided_plan(b, run[0])) return rc;
    if (int rc = guided_plan(b, run[1])) return rc;
    b.h_xlen = klen.data();
    b.h_ylen = wlen.data();  // the query is the window or less
    if (int rc = guided_plan(b, run[2])) return rc;
    for (int q = 0; q < 3; q++)
        if (int rc = guided_reserve(area, run[q])) return rc;
    // the first pass
    b.d_pairs = d_pairs1.cget();
    b.d_x = d_win.cget();
    b.d_y = d_cons.cget();
    b.d_guide = d_guide.cget();
    b.h_xlen = wlen.data();
    b.h_ylen = clen.data();
    b.d_slots = d_slots1.get();
    b.d_slot_end = d_end12.cget();
    outputs(0);
    if (int rc = guided_enqueue(b, run[0], area, st)) return rc;
    // the second, guided by the first one's ops
    const uint32_t blocks = (uint32_t)((n + 255) / 256);
    encode_next_kernel<<<blocks, 256, 0, st>>>((uint32_t)n, d_pairs1.cget(), d_end12.cget(), d_nops[0].cget(), d_pairs2.get());
    JTK_HIP_TRY(hipGetLastError());
    b.d_pairs = d_pairs2.cget();
    b.d_guide = d_slots1.cget();
    b.d_slots = d_slots2.get();
    outputs(1);
    if (int rc = guided_enqueue(b, run[1], area, st)) return rc;
    // swap, trim, count; the third pass
    encode_fit_kernel<<<(uint32_t)((n + 3) / 4), 256, 0, st>>>((uint32_t)n, d_en.cget(), d_status.cget(), d_slots2.get(), d_end12.cget(), d_nops[1].cget(),
                                                              d_fit.get(), d_pairs3.get());
    JTK_HIP_TRY(hipGetLastError());
    b.d_pairs = d_pairs3.cget();
    b.d_x = d_chunk.cget();
    b.d_y = d_win.cget();
    b.d_guide = d_slots2.cget();
    b.h_xlen = klen.data();
    b.h_ylen = wlen.data();
    b.d_slots = d_slots3.get();
    b.d_slot_end = d_end3.cget();
    outputs(2);
    if (int rc = guided_enqueue(b, run[2], area, st)) return rc;
    // ---- 5. the results
    std::vector<EnFit> fit(n);
    std::vector<int32_t> score(n);
    std::vector<uint32_t> nops(n);
    JTK_HIP_TRY(d_fit.download(fit.data(), n, st));
    JTK_HIP_TRY(d_score[2].download(score.data(), n, st));
    JTK_HIP_TRY(d_nops[2].download(nops.data(), n, st));
    JTK_HIP_TRY(d_status.download(st_v.data(), n, st));
    JTK_HIP_TRY(hipStreamSynchronize(st));
    JTK_HIP_TRY(hipGetLastError());
    for (int q = 0; q < 3; q++)
        if (int rc = guided_elapsed(run[q], &g_encode_timing[1 + q], &g_encode_timing[4 + q])) return rc;
    int rc = 0;
    std::vector<uint64_t> dst_off(n + 1, 0);
    for (size_t k = 0; k < n; k++) {
        if (st_v[k] == JTK_ERR_INTERNAL) return jtk_fail(JTK_ERR_INTERNAL, "guided: the walk left the band");
        if (st_v[k]) {
            rc = JTK_ERR_CHUNK_FAILED;
            nops[k] = 0;
        }
        dst_off[k + 1] = dst_off[k] + nops[k];
    }
    const uint64_t total = dst_off[n];
    if (total > ops_cap || (total && !ops_out)) return jtk_fail(JTK_ERR_INVALID_ARG, "ops_cap is smaller than the ops of the batch");
    if (total) {
        DevArr<uint64_t> d_off;
        DevArr<uint8_t> d_out;
        if (int rc2 = d_off.upload(dst_off, st)) return jtk_fail(rc2, "device upload failed");
        JTK_HIP_TRY(d_out.alloc(total));
        if (int rc2 = guided_pack(n, d_slots3.cget(), d_end3.cget(), d_nops[2].cget(), d_off.cget(), d_out.get(), st)) return rc2;
        JTK_HIP_TRY(d_out.download(ops_out, total, st));
        JTK_HIP_TRY(hipStreamSynchronize(st));
        JTK_HIP_TRY(hipGetLastError());
    }
    for (size_t k = 0, t = 0; t < n_trials; t++) {  // a trial that stopped at the filter has an empty share
        ops_out_off[t] = dst_off[k];
        if (k < n && live[k] == t) k++;
    }
    ops_out_off[n_trials] = total;
    for (size_t k = 0; k < n; k++) {
        const jtk_encode_trial_t &tr = trials[live[k]];
        jtk_encode_result_t &r = result[live[k]];
        r.status = st_v[k];
        if (st_v[k]) continue;
        const EnFit &f = fit[k];
        r.trim_head = f.trim_head;
        r.trim_tail = f.trim_tail;
        r.position_from_start = (uint64_t)tr.start + (tr.is_forward ? f.trim_head : f.trim_tail);
        r.query_len = wlen[k] - f.trim_head - f.trim_tail;
        r.score = score[k];
        r.mat_num = f.mat_num;
        r.ops_len = f.ops_len;
        r.head_match = f.head_match;
        r.head_len = f.head_len;
        r.tail_match = f.tail_match;
        r.tail_len = f.tail_len;
        // :501-505; f64::min returns the other operand when one is NaN, as fmin does
        const double identity = (double)f.mat_num / (double)f.ops_len;
        const double head = (double)f.head_match / (double)f.head_len, tail = (double)f.tail_match / (double)f.tail_len;
        const bool below_dissim = 1.0 - tr.sim_thr < identity && EN_EDGE_BOUND < std::fmin(head, tail);
        r.verdict = below_dissim ? JTK_ENCODE_ACCEPTED : JTK_ENCODE_REJECTED;
    }
    if (rc) return jtk_fail(rc, "a trial was refused by the infix alignment or by a guided pass (see its status)");
    return 0;
}
