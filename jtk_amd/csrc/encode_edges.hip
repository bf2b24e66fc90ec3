// encode_edges.hip -- jtk_lc_encode_edges: `encode_edge` with `tune_position` (haplotyper/src/dense_encoding.rs:627-759) for a
// batch of trials, restated as it stands.  Per trial:
//   device  encode_window_kernel: the window of the raw read, reverse-complemented when the trial is reverse, upper-cased (:722-727)
//   host    jtk_lc_align_reads_mode, infix, the window free: the stretch [seq_start, seq_end) of the window (:731-739)
//   host    jtk_lc_align_reads_mode, infix, the contig free, on the truncated window: [ctg_start, ctg_end) and the guide (:746-755);
//           the descriptors of the guided pass and the cut are host arithmetic on these numbers
//   device  one global pass of the guided aligner of guided.hip, x = contig[ctg_start .. ctg_end), y = the truncated window (:757)
//           edge_cut_kernel: the pass's ops against the contig's break points (:640-692): per chunk the counts, the query range and
//           the position; edge_pack_kernel: every trial's op stream, virtual Dels included, into its share of the op area
//   host    the verdict (:671, f64 from the integer counts) and the packing of the shares behind each other
// Everything between the upload of the guides and the copy back of the results is enqueued on one stream without a wait.
#include <chrono>
#include <cstring>
#include <vector>

#include "device_common.h"
#include "encode_window.h"
#include "guided_internal.h"
#include "jtk_lc_debug.h"
#include "wave_util.h"

namespace {

constexpr int EE_MATCH = 2, EE_MISMATCH = -6, EE_OPEN = -5, EE_EXT = -1;  // ALN_PARAMETER (haplotyper/src/lib.rs)
constexpr int32_t EE_SKIP = 1;  // the status of a trial without a guided pass (an empty truncated window) while it is on the device

struct EeCut {  // what the cut needs of a trial besides the pass's ops: host arithmetic on the two infix alignments
    uint64_t break_first;  // into the break points
    uint64_t node_first;   // the trial's first node slot
    uint64_t out_first;    // the trial's share of the op area, out_cap bytes
    uint32_t out_cap;
    uint32_t n_chunks, first_chunk;
    uint32_t lead;  // the Dels in front of the pass's ops: ctg_start - the break point below it (:647-650)
    uint32_t ctg_start, ctg_end, seq_start;
    uint32_t start, end, is_forward;
};
struct EeRec {  // at the op that closes a chunk: window bases and Matches of the stream so far, and the op's index in the stream
    uint32_t y, m, idx, pad;
};
struct EeOut {
    uint32_t head_ins, total;  // the leading Ins run; the ops of the trial's chunks together
};

// One wave per trial, on the pass's ops in their slot.  The stream of :652-655 is the ops behind their leading Ins run, then
// (contig_len - ctg_end) Dels that are never written: a chunk whose break point lies behind ctg_end is closed by arithmetic.
__global__ void __launch_bounds__(256) edge_cut_kernel(uint32_t n, const EeCut *cuts, const int32_t *status, const uint8_t *slots,
                                                       const uint64_t *slot_end, const uint32_t *nops, const uint32_t *breaks, EeRec *recs,
                                                       EeOut *outs, jtk_edge_node_t *nodes) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t t = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (t >= n) return;
    const EeCut c = cuts[t];
    const uint32_t *bp = breaks + c.break_first;
    EeRec *rec = recs + c.node_first;
    jtk_edge_node_t *nd = nodes + c.node_first;
    const bool live = status[t] == 0 && c.first_chunk < c.n_chunks;
    EeOut o{};
    if (live) {
        const uint32_t len = nops[t];
        const uint8_t *ops = slots + (slot_end[t] - len);
        // ---- remove_leading_insertions: the first op that is no Ins
        uint32_t head = len;
        for (uint32_t base = 0; base < len; base += 64) {
            const uint32_t q = base + lane;
            const uint64_t other = __ballot(q < len && ops[q] != JTK_OP_INS);
            if (other) {
                head = base + (uint32_t)__ffsll((long long)other) - 1;
                break;
            }
        }
        const uint32_t real = len - head;
        // ---- the walk: per lane, what the stream has consumed up to and including its op
        uint32_t x_before = 0, y_before = 0, m_before = 0;
        const uint64_t upto = ~0ull >> (63 - lane);
        for (uint32_t base = 0; base < real; base += 64) {
            const uint32_t s = base + lane;
            const bool active = s < real;
            const uint8_t op = active ? ops[head + s] : (uint8_t)JTK_OP_INS;
            const uint64_t bx = __ballot(active && op != JTK_OP_INS), by = __ballot(active && op != JTK_OP_DEL);
            const uint64_t bm = __ballot(active && op == JTK_OP_MATCH);
            if (active && op != JTK_OP_INS) {  // xpos has just risen: does it stand on a break point?
                const uint32_t xpos = c.ctg_start + x_before + (uint32_t)__popcll(bx & upto);
                uint32_t lo = c.first_chunk, hi = c.n_chunks;
                while (lo < hi) {
                    const uint32_t mid = lo + ((hi - lo) >> 1);
                    if (bp[mid] < xpos)
                        lo = mid + 1;
                    else
                        hi = mid;
                }
                if (lo < c.n_chunks && bp[lo] == xpos)
                    rec[lo] = EeRec{y_before + (uint32_t)__popcll(by & upto), m_before + (uint32_t)__popcll(bm & upto), s, 0};
            }
            x_before += (uint32_t)__popcll(bx);
            y_before += (uint32_t)__popcll(by);
            m_before += (uint32_t)__popcll(bm);
        }
        // ---- the chunks that a Del behind the pass's ops closes
        for (uint32_t k = c.first_chunk + lane; k < c.n_chunks; k += 64)
            if (bp[k] > c.ctg_end) rec[k] = EeRec{y_before, m_before, real + (bp[k] - c.ctg_end) - 1, 0};
        jtk_wave_sync();  // the differences below read records that other lanes have written
        o.head_ins = head;
        o.total = c.lead + rec[c.n_chunks - 1].idx + 1;
    }
    // ---- a chunk's node: the difference of its record and the one before
    for (uint32_t k = lane; k < c.n_chunks; k += 64) {
        jtk_edge_node_t node{};
        node.verdict = JTK_EDGE_NOT_REACHED;
        if (live && k >= c.first_chunk) {
            const EeRec cur = rec[k];
            const bool first = k == c.first_chunk;
            const EeRec prev = first ? EeRec{0, 0, 0xffffffffu, 0} : rec[k - 1];
            const uint32_t ypos = o.head_ins + cur.y;
            node.verdict = JTK_EDGE_REJECTED;  // the host takes the verdict from the two counts
            node.mat_num = cur.m - prev.m;
            node.ops_len = cur.idx - prev.idx + (first ? c.lead : 0u);
            node.query_len = cur.y - prev.y;
            node.query_off = c.seq_start + ypos - node.query_len;
            node.position_from_start = c.is_forward ? (uint64_t)c.start + node.query_off : (uint64_t)c.end - c.seq_start - ypos;
        }
        nd[k] = node;
    }
    if (lane == 0) outs[t] = o;
}

// one workgroup per trial: lead x Del, the pass's ops behind their leading Ins run, Dels up to the last closing op
__global__ void __launch_bounds__(256) edge_pack_kernel(uint32_t n, const EeCut *cuts, const int32_t *status, const uint8_t *slots,
                                                        const uint64_t *slot_end, const uint32_t *nops, const EeOut *outs, uint8_t *area) {
    const uint32_t t = blockIdx.x;
    if (t >= n || status[t] != 0) return;
    const EeCut c = cuts[t];
    const EeOut o = outs[t];
    const uint32_t len = nops[t];
    const uint8_t *ops = slots + (slot_end[t] - len);
    const uint32_t real = len - o.head_ins;
    const uint32_t total = o.total < c.out_cap ? o.total : c.out_cap;
    for (uint32_t v = threadIdx.x; v < total; v += blockDim.x) {
        uint8_t op = JTK_OP_DEL;
        if (v >= c.lead && v - c.lead < real) op = ops[o.head_ins + (v - c.lead)];
        area[c.out_first + v] = op;
    }
}

thread_local double g_edges_timing[8];

}  // namespace

extern "C" void jtk_lc_debug_edges_timing(double *out) {
    if (out) std::memcpy(out, g_edges_timing, sizeof(g_edges_timing));
}

extern "C" int jtk_lc_encode_edges(size_t n_trials, const jtk_edge_trial_t *trials, const uint8_t *read_bases, const uint8_t *contig_bases,
                                   const uint32_t *break_points, const uint64_t *node_off, jtk_edge_result_t *result, jtk_edge_node_t *nodes,
                                   uint8_t *ops_out, uint64_t *ops_out_off, uint64_t ops_cap, int device) {
    g_last_error.clear();
    if (!ops_out_off || !node_off || (n_trials && (!trials || !read_bases || !contig_bases || !break_points || !result || !nodes)))
        return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    if (n_trials >= 0x7fffffffu) return jtk_fail(JTK_ERR_UNSUPPORTED, "2^31 - 1 trials or more");
    if (node_off[0] != 0) return jtk_fail(JTK_ERR_INVALID_ARG, "node_off is not the prefix sum of n_chunks");
    const size_t n = n_trials;
    uint64_t ops_need = 0, contig_bytes = 0, break_count = 0;
    auto acgt = [](uint8_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; };
    for (size_t t = 0; t < n; t++) {
        const jtk_edge_trial_t &tr = trials[t];
        if (tr.start >= tr.end) return jtk_fail(JTK_ERR_INVALID_ARG, "a window with start >= end");
        if (!tr.n_chunks) return jtk_fail(JTK_ERR_INVALID_ARG, "a trial without chunks");
        if (!tr.contig_len) return jtk_fail(JTK_ERR_INVALID_ARG, "an empty contig");
        if (node_off[t + 1] - node_off[t] != tr.n_chunks) return jtk_fail(JTK_ERR_INVALID_ARG, "node_off is not the prefix sum of n_chunks");
        const uint32_t *bp = break_points + tr.break_first;
        for (uint32_t k = 0; k < tr.n_chunks; k++)
            if (bp[k] <= (k ? bp[k - 1] : 0u)) return jtk_fail(JTK_ERR_INVALID_ARG, "break points that do not ascend strictly");
        if (bp[tr.n_chunks - 1] != tr.contig_len) return jtk_fail(JTK_ERR_INVALID_ARG, "the last break point is not the contig's length");
        for (uint64_t q = tr.contig_off; q < tr.contig_off + tr.contig_len; q++)
            if (!acgt(contig_bases[q])) return jtk_fail(JTK_ERR_INVALID_ARG, "non-ACGT base in a contig");
        for (uint64_t q = tr.read_off + tr.start; q < tr.read_off + tr.end; q++) {
            const uint8_t b = read_bases[q];
            if (!acgt(b >= 'a' && b <= 'z' ? (uint8_t)(b - 32) : b)) return jtk_fail(JTK_ERR_INVALID_ARG, "non-ACGT base in a window");
        }
        ops_need += (uint64_t)tr.contig_len + (tr.end - tr.start);
        contig_bytes = std::max(contig_bytes, tr.contig_off + tr.contig_len);
        break_count = std::max(break_count, tr.break_first + tr.n_chunks);
    }
    // decided before any device work, whatever the batch's ops come to
    if (ops_cap < ops_need || (ops_need && !ops_out)) return jtk_fail(JTK_ERR_INVALID_ARG, "ops_cap is smaller than sum(contig_len + end - start)");
    if (int rc = jtk_require_device(device)) return rc;
    const uint64_t n_nodes = node_off[n];
    std::memset(g_edges_timing, 0, sizeof(g_edges_timing));
    g_edges_timing[0] = (double)n;
    for (uint64_t e = 0; e <= n_nodes; e++) ops_out_off[e] = 0;
    if (!n) return 0;
    // ---- 1. the windows
    std::vector<EnWindow> wins(n);
    std::vector<uint64_t> win_off(n + 1, 0);
    for (size_t k = 0; k < n; k++) {
        wins[k].off = win_off[k];
        wins[k].len = trials[k].end - trials[k].start;
        wins[k].is_forward = trials[k].is_forward ? 1u : 0u;
        win_off[k + 1] = win_off[k] + wins[k].len;
    }
    std::vector<uint8_t> raw(win_off[n]), windows(win_off[n]);
    for (size_t k = 0; k < n; k++) std::memcpy(raw.data() + win_off[k], read_bases + trials[k].read_off + trials[k].start, wins[k].len);
    DevStream s;
    JTK_HIP_TRY(s.create(2));
    const hipStream_t st = s.st;
    DevArr<EnWindow> d_wins;
    DevArr<uint8_t> d_raw, d_win, d_contig;
    DevArr<uint32_t> d_flags;
    const std::vector<uint8_t> contig_v(contig_bases, contig_bases + contig_bytes);
    {
        int rc;
        if ((rc = d_wins.upload(wins, st)) || (rc = d_raw.upload(raw, st)) || (rc = d_contig.upload(contig_v, st))) return jtk_fail(rc, "device upload failed");
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
    }
    // ---- 2. the two infix alignments: the window's stretch, then the contig's stretch and the guide
    std::vector<int32_t> st_v(n, 0);
    std::vector<uint32_t> seq_start(n), seq_end(n), ctg_start(n, 0), ctg_end(n, 0), dist(n);
    std::vector<uint8_t> guide;
    std::vector<uint64_t> guide_off(n + 1, 0);
    std::vector<uint8_t> go(n, 0);  // 1: the trial has a truncated window to lay the contig on
    {
        std::vector<jtk_lc_chunk_t> chunks(n);
        uint64_t cap = 0;
        for (size_t k = 0; k < n; k++) {
            chunks[k] = jtk_lc_chunk_t{0, 0, 1, trials[k].contig_off, trials[k].contig_len, k};
            cap += (uint64_t)trials[k].contig_len + wins[k].len;
        }
        std::vector<uint8_t> e_ops(cap + 1);
        std::vector<uint64_t> e_off(n + 1);
        auto t0 = std::chrono::steady_clock::now();
        int rc = jtk_lc_align_reads_mode(n, chunks.data(), contig_bases, windows.data(), win_off.data(), JTK_ALIGN_INFIX, JTK_ALIGN_FREE_READ, 0, e_ops.data(),
                                         e_off.data(), cap, dist.data(), seq_start.data(), seq_end.data(), st_v.data(), device);
        g_edges_timing[4] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (rc && rc != JTK_ERR_CHUNK_FAILED) return rc;
        // the truncated windows, behind each other; a refused trial and an empty stretch take no part in the second alignment
        std::vector<uint64_t> cut_off(n + 1, 0);
        for (size_t k = 0; k < n; k++) {
            go[k] = !st_v[k] && seq_start[k] < seq_end[k];
            cut_off[k + 1] = cut_off[k] + (go[k] ? seq_end[k] - seq_start[k] : 0u);
            if (!go[k]) chunks[k].tmpl_len = 0;
        }
        std::vector<uint8_t> cut(cut_off[n] + 1);
        for (size_t k = 0; k < n; k++)
            if (go[k]) std::memcpy(cut.data() + cut_off[k], windows.data() + win_off[k] + seq_start[k], seq_end[k] - seq_start[k]);
        std::vector<int32_t> st2(n, 0);
        guide.resize(cap + 1);
        t0 = std::chrono::steady_clock::now();
        rc = jtk_lc_align_reads_mode(n, chunks.data(), contig_bases, cut.data(), cut_off.data(), JTK_ALIGN_INFIX, JTK_ALIGN_FREE_TEMPLATE, 0, guide.data(),
                                     guide_off.data(), cap, dist.data(), ctg_start.data(), ctg_end.data(), st2.data(), device);
        g_edges_timing[5] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (rc && rc != JTK_ERR_CHUNK_FAILED) return rc;
        g_last_error.clear();  // a refused trial is reported at the end
        for (size_t k = 0; k < n; k++) {
            if (!st_v[k] && st2[k]) st_v[k] = st2[k];
            if (st_v[k]) go[k] = 0;
            if (!go[k]) ctg_start[k] = ctg_end[k] = 0;
        }
    }
    // ---- 3. the descriptors of the guided pass and of the cut
    std::vector<jtk_guided_pair_t> pairs(n);
    std::vector<EeCut> cuts(n);
    std::vector<uint32_t> xlen(n), ylen(n), radius(n);
    std::vector<uint64_t> slot_end(n);
    uint64_t slot = 0, area_bytes = 0;
    for (size_t k = 0; k < n; k++) {
        const jtk_edge_trial_t &tr = trials[k];
        const uint32_t *bp = break_points + tr.break_first;
        jtk_guided_pair_t &p = pairs[k];
        EeCut &c = cuts[k];
        std::memset(&p, 0, sizeof(p));
        std::memset(&c, 0, sizeof(c));
        c.break_first = tr.break_first;
        c.node_first = node_off[k];
        c.out_first = area_bytes;
        c.n_chunks = c.first_chunk = tr.n_chunks;
        c.start = tr.start;
        c.end = tr.end;
        c.is_forward = tr.is_forward ? 1u : 0u;
        p.radius = radius[k] = tr.radius;
        if (go[k]) {
            p.x_off = tr.contig_off + ctg_start[k];
            p.x_len = ctg_end[k] - ctg_start[k];
            p.y_off = win_off[k] + seq_start[k];
            p.y_len = seq_end[k] - seq_start[k];
            p.guide_off = guide_off[k];
            p.guide_len = (uint32_t)(guide_off[k + 1] - guide_off[k]);
            c.first_chunk = (uint32_t)(std::upper_bound(bp, bp + tr.n_chunks, ctg_start[k]) - bp);  // the first k with ctg_start < bp[k], :642
            c.lead = c.first_chunk < tr.n_chunks ? ctg_start[k] - (c.first_chunk ? bp[c.first_chunk - 1] : 0u) : 0u;
            c.ctg_start = ctg_start[k];
            c.ctg_end = ctg_end[k];
            c.seq_start = seq_start[k];
            c.out_cap = tr.contig_len + p.y_len;
        } else if (!st_v[k]) {
            st_v[k] = EE_SKIP;
        }
        xlen[k] = p.x_len;
        ylen[k] = p.y_len;
        slot += (uint64_t)p.x_len + p.y_len;
        slot_end[k] = slot;
        area_bytes += c.out_cap;
    }
    const std::vector<uint32_t> breaks_v(break_points, break_points + break_count);
    DevArr<jtk_guided_pair_t> d_pairs;
    DevArr<EeCut> d_cuts;
    DevArr<EeRec> d_recs;
    DevArr<EeOut> d_outs;
    DevArr<jtk_edge_node_t> d_nodes;
    DevArr<uint8_t> d_guide, d_slots, d_area;
    DevArr<uint64_t> d_slot_end;
    DevArr<uint32_t> d_breaks, d_start, d_endv, d_nops;
    DevArr<int32_t> d_status, d_score;
    {
        int rc;
        if ((rc = d_pairs.upload(pairs, st)) || (rc = d_cuts.upload(cuts, st)) || (rc = d_guide.upload(guide, st)) || (rc = d_status.upload(st_v, st)) ||
            (rc = d_slot_end.upload(slot_end, st)) || (rc = d_breaks.upload(breaks_v, st)))
            return jtk_fail(rc, "device upload failed");
    }
    JTK_HIP_TRY(d_recs.alloc(n_nodes));
    JTK_HIP_TRY(d_recs.zero(n_nodes, st));
    JTK_HIP_TRY(d_outs.alloc(n));
    JTK_HIP_TRY(d_nodes.alloc(n_nodes));
    JTK_HIP_TRY(d_slots.alloc(slot + 1));
    JTK_HIP_TRY(d_area.alloc(area_bytes));
    JTK_HIP_TRY(d_score.alloc(n));
    JTK_HIP_TRY(d_start.alloc(n));
    JTK_HIP_TRY(d_endv.alloc(n));
    JTK_HIP_TRY(d_nops.alloc(n));
    JTK_HIP_TRY(d_score.zero(n, st));
    JTK_HIP_TRY(d_nops.zero(n, st));
    GuidedRun run;
    GuidedArea area;
    GuidedBatch b;
    b.n = n;
    b.d_pairs = d_pairs.cget();
    b.d_x = d_contig.cget();
    b.d_y = d_win.cget();
    b.d_guide = d_guide.cget();
    b.infix = 0;
    b.match = EE_MATCH;
    b.mismatch = EE_MISMATCH;
    b.gap_open = EE_OPEN;
    b.gap_ext = EE_EXT;
    b.h_xlen = xlen.data();
    b.h_ylen = ylen.data();
    b.h_radius = radius.data();
    b.d_score = d_score.get();
    b.d_status = d_status.get();
    b.d_start = d_start.get();
    b.d_end = d_endv.get();
    b.d_nops = d_nops.get();
    b.d_slots = d_slots.get();
    b.d_slot_end = d_slot_end.cget();
    if (int rc = guided_plan(b, run)) return rc;
    if (int rc = guided_reserve(area, run)) return rc;
    if (int rc = guided_enqueue(b, run, area, st)) return rc;
    // ---- 4. the cut and the trials' op streams
    JTK_HIP_TRY(hipEventRecord(s.ev[0], st));
    edge_cut_kernel<<<(uint32_t)((n + 3) / 4), 256, 0, st>>>((uint32_t)n, d_cuts.cget(), d_status.cget(), d_slots.cget(), d_slot_end.cget(), d_nops.cget(),
                                                            d_breaks.cget(), d_recs.get(), d_outs.get(), d_nodes.get());
    JTK_HIP_TRY(hipGetLastError());
    edge_pack_kernel<<<(uint32_t)n, 256, 0, st>>>((uint32_t)n, d_cuts.cget(), d_status.cget(), d_slots.cget(), d_slot_end.cget(), d_nops.cget(), d_outs.cget(),
                                                  d_area.get());
    JTK_HIP_TRY(hipGetLastError());
    JTK_HIP_TRY(hipEventRecord(s.ev[1], st));
    // ---- 5. the results
    std::vector<EeOut> outs(n);
    std::vector<int32_t> score(n);
    std::vector<jtk_edge_node_t> nodes_v(n_nodes);
    std::vector<uint8_t> area_v(area_bytes);
    JTK_HIP_TRY(d_outs.download(outs.data(), n, st));
    JTK_HIP_TRY(d_score.download(score.data(), n, st));
    JTK_HIP_TRY(d_status.download(st_v.data(), n, st));
    if (n_nodes) JTK_HIP_TRY(d_nodes.download(nodes_v.data(), n_nodes, st));
    if (area_bytes) JTK_HIP_TRY(d_area.download(area_v.data(), area_bytes, st));
    JTK_HIP_TRY(hipStreamSynchronize(st));
    JTK_HIP_TRY(hipGetLastError());
    {
        float ms = 0.f;
        JTK_HIP_TRY(s.elapsed(0, 1, &ms));
        g_edges_timing[6] = ms;
        if (int rc = guided_elapsed(run, &g_edges_timing[1], &g_edges_timing[2])) return rc;
        g_edges_timing[3] = run.slices;
    }
    int rc = 0;
    uint64_t total = 0;
    for (size_t k = 0; k < n; k++) {
        if (st_v[k] == JTK_ERR_INTERNAL) return jtk_fail(JTK_ERR_INTERNAL, "guided: the walk left the band");
        const jtk_edge_trial_t &tr = trials[k];
        const EeCut &c = cuts[k];
        jtk_edge_result_t &r = result[k];
        jtk_edge_node_t *nd = nodes_v.data() + node_off[k];
        std::memset(&r, 0, sizeof(r));
        r.first_chunk = tr.n_chunks;
        const bool answered = st_v[k] == 0 || st_v[k] == EE_SKIP;
        if (!answered) {
            rc = JTK_ERR_CHUNK_FAILED;
            r.status = st_v[k];
        } else {
            r.seq_start = seq_start[k];
            r.seq_end = seq_end[k];
        }
        if (st_v[k] == 0) {
            r.score = score[k];
            r.ctg_start = c.ctg_start;
            r.ctg_end = c.ctg_end;
            r.first_chunk = c.first_chunk;
            r.head_ins = outs[k].head_ins;
        }
        uint64_t from = c.out_first;
        for (uint32_t q = 0; q < tr.n_chunks; q++) {
            jtk_edge_node_t &e = nd[q];
            ops_out_off[node_off[k] + q] = total;
            if (st_v[k] != 0 || e.verdict == JTK_EDGE_NOT_REACHED) {
                std::memset(&e, 0, sizeof(e));
                e.verdict = JTK_EDGE_NOT_REACHED;
                continue;
            }
            if (from + e.ops_len > c.out_first + c.out_cap) return jtk_fail(JTK_ERR_INTERNAL, "encode_edges: a trial's ops outgrow its share");
            // :671, f64 from the two integers
            e.verdict = 1.0 - tr.sim_thr < (double)e.mat_num / (double)e.ops_len ? JTK_EDGE_ACCEPTED : JTK_EDGE_REJECTED;
            std::memcpy(ops_out + total, area_v.data() + from, e.ops_len);
            from += e.ops_len;
            total += e.ops_len;
        }
    }
    ops_out_off[n_nodes] = total;
    std::copy(nodes_v.begin(), nodes_v.end(), nodes);
    if (rc) return jtk_fail(rc, "a trial was refused by an infix alignment or by the guided pass (see its status)");
    return 0;
}
