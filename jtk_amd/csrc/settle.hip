// settle.hip -- jtk_lc_settle_nodes: what correct_deletion does to a read's node list once the trials are in, and the per-node
// numbers purge_largeindel reads.
//
//   correct_deletion_error (encode/deletion_fill.rs:349-361)   sort by (chunk, position), remove_slippy_alignment, sort by position,
//                                                              remove_slippy_alignment, remove_overlapping_encoding
//   re_encode_read (determine_chunks.rs:548-562)               the same with the first sort by chunk alone
//   remove_slippy_alignment (encode/mod.rs:288-313)            its `score` is a node's (Match + Mismatch) - (Ins + Del)
//   remove_overlapping_encoding (encode/mod.rs:248-286)        its identity is 1.0 - indel / total
//   purge_large_deletion_nodes (purge_diverged.rs:75-80)       del_size = misc::max_region (misc.rs:345-358) / 2
// On the device: one wave per read.  The statistics walk a node's ops 64 at a time (counts from ballots, as purge.hip walks a
// node; the largest range sum from a wave scan over the (sum, best prefix, best suffix, best) monoid).  The keys and statistics of
// the read's nodes then sit in the wave's work area -- ST_LDS_NODES nodes of LDS, or a slice of a global block for a longer
// read, through the same pointers -- both sorts are rank-by-count over it (a node's rank = the nodes that sort before it, the
// position in the list breaking ties, which is what makes them stable), and the three removal passes are one lane's walk over
// the sorted list: each step depends on what the one before it kept.
#include <cstring>
#include <string>
#include <vector>

#include "device_common.h"
#include "jtk_lc_debug.h"
#include "prim_host.h"
#include "wave_util.h"

namespace {

constexpr uint32_t ST_WAVES = 4;          // waves (reads in flight) per workgroup
constexpr uint32_t ST_LDS_NODES = 128;    // nodes of a read whose work area is LDS: 44 bytes each, 5.5 KiB per wave, 22 KiB per
                                          // workgroup -- seven workgroups, 28 waves, on a CU's 160 KiB
constexpr uint32_t ST_NODE_BYTES = 44;    // chunk, position (8 each), query_len, is_forward, score, total, indel, two lists (4 each)
constexpr uint32_t ST_GRID = 4096;        // workgroups at most (the waves loop over the reads)
constexpr uint64_t ST_MAX_NODES = 0x7fffffffull;  // nodes of one call, and ops of one node: indices are 32-bit
constexpr uint32_t ST_DROPPED = 0xffffffffu;      // order[] behind a read's survivors
constexpr long long ST_NEG = -(1ll << 60);        // "no range": below every sum, and two of them still fit

thread_local double g_settle_timing[4];  // reads, reads in global memory, kernel ms, ms of the whole call

// A read's work area: LDS or global memory, through generic pointers.
struct Area {
    uint64_t *chunk, *pos;
    uint32_t *qlen, *fwd;
    int32_t *score;
    uint32_t *total, *indel;
    uint32_t *a, *b;  // the two node lists
};

// The largest sum of a non-empty range: what two adjacent stretches know of themselves is enough for their union.
struct Mss {
    long long sum, pre, suf, best;
};
__device__ __forceinline__ long long st_max(long long x, long long y) { return x > y ? x : y; }
__device__ __forceinline__ Mss st_join(const Mss &l, const Mss &r) {
    Mss o;
    o.sum = l.sum + r.sum;
    o.pre = st_max(l.pre, l.sum + r.pre);
    o.suf = st_max(r.suf, r.sum + l.suf);
    o.best = st_max(st_max(l.best, r.best), l.suf + r.pre);
    return o;
}
__device__ __forceinline__ Mss st_shfl_up(const Mss &v, uint32_t o) {
    Mss u;
    u.sum = __shfl_up(v.sum, o, 64);
    u.pre = __shfl_up(v.pre, o, 64);
    u.suf = __shfl_up(v.suf, o, 64);
    u.best = __shfl_up(v.best, o, 64);
    return u;
}

// One node's statistics by the whole wave; every lane gets the same values.  Returns 0, JTK_ERR_INVALID_ARG (an op above 3:
// the statistics are then 0) or JTK_ERR_UNSUPPORTED (no ops, or the ops take a number of read bases other than query_len).
__device__ __forceinline__ int st_node_stats(const uint8_t *ops, uint32_t on, uint32_t query_len, uint32_t lane, jtk_node_stats_t *out) {
    uint32_t indel = 0, taken = 0;
    bool bad = false;
    Mss all = {0, ST_NEG, ST_NEG, ST_NEG};
    for (uint32_t base = 0; base < on; base += 64) {
        const uint32_t i = base + lane;
        const bool active = i < on;
        const uint32_t op = active ? ops[i] : 0xffu;
        if (__ballot(active && op > 3u)) {
            bad = true;
            break;
        }
        const bool gap = active && op >= 2u;
        indel += (uint32_t)__popcll(__ballot(gap));
        taken += (uint32_t)__popcll(__ballot(active && op <= 2u));  // Match, Mismatch, Ins take a read base
        const long long w = gap ? 2 : -1;
        Mss v = {active ? w : 0, active ? w : ST_NEG, active ? w : ST_NEG, active ? w : ST_NEG};
#pragma unroll
        for (uint32_t o = 1; o < 64; o <<= 1) {  // inclusive scan: lane l ends with the join of lanes 0 ..= l
            const Mss u = st_shfl_up(v, o);
            if (lane >= o) v = st_join(u, v);
        }
        Mss blk;
        blk.sum = __shfl(v.sum, 63, 64);
        blk.pre = __shfl(v.pre, 63, 64);
        blk.suf = __shfl(v.suf, 63, 64);
        blk.best = __shfl(v.best, 63, 64);
        all = st_join(all, blk);
    }
    if (bad) {
        out->score = 0;
        out->total = out->indel = 0;
        out->del_size = 0;
        return JTK_ERR_INVALID_ARG;
    }
    out->total = on;
    out->indel = indel;
    out->score = (int32_t)(on - indel) - (int32_t)indel;
    // with an indel the best range of the run-length cigar is the best range of the per-base weights (it ends on run
    // boundaries and is >= 2); without one the cigar is a single Match run, whose only range is -total
    out->del_size = indel ? all.best / 2 : -(long long)on / 2;
    return (on == 0 || taken != query_len) ? JTK_ERR_UNSUPPORTED : 0;
}

// dst[rank of k] = the k-th node of `src` (nullptr: node k), by (chunk if by_chunk, position if by_pos, k)
__device__ __forceinline__ void st_rank_sort(const Area &w, uint32_t m, const uint32_t *src, uint32_t *dst, bool by_chunk, bool by_pos,
                                             uint32_t lane) {
    for (uint32_t k = lane; k < m; k += 64) {
        const uint32_t i = src ? src[k] : k;
        const uint64_t ci = by_chunk ? w.chunk[i] : 0, pi = by_pos ? w.pos[i] : 0;
        uint32_t rank = 0;
        for (uint32_t k2 = 0; k2 < m; k2++) {
            const uint32_t j = src ? src[k2] : k2;
            const uint64_t cj = by_chunk ? w.chunk[j] : 0, pj = by_pos ? w.pos[j] : 0;
            rank += (cj < ci || (cj == ci && (pj < pi || (pj == pi && k2 < k)))) ? 1u : 0u;
        }
        dst[rank] = i;
    }
}

// remove_slippy_alignment on the list L[0 .. m), in place, by one lane; returns what is left (m >= 1)
__device__ __forceinline__ uint32_t st_slippy(const Area &w, uint32_t *L, uint32_t m) {
    uint32_t out = 0, prev = L[0];
    for (uint32_t k = 1; k < m; k++) {
        const uint32_t node = L[k];
        const bool disjoint = w.pos[prev] + w.qlen[prev] < w.pos[node];
        if (w.chunk[prev] != w.chunk[node] || w.fwd[prev] != w.fwd[node] || disjoint) {
            L[out++] = prev;  // out <= k - 1: behind what is still to be read
            prev = node;
        } else if (w.score[prev] < w.score[node]) {
            prev = node;
        }
    }
    L[out++] = prev;
    return out;
}

// remove_overlapping_encoding on the list L[0 .. m), in place, by one lane; returns what is left.
// The reference removes one node of the FIRST violating pair and starts over.  Let that pair be (i, i + 1): the pairs before it
// do not violate, and the removal leaves them as they are.  The only pair that is new afterwards is (i - 1, i + 1) where node i
// went, or (i, i + 2) where node i + 1 went; every pair behind it is a pair that has not been looked at yet.  So the first
// violating pair of the new list is not before (i - 1, .), and a scan that goes on from there finds what the restart finds.
// Here L[0 .. out) is the part whose adjacent pairs are known not to violate; the next node is tested against its last entry.
// Where that entry goes, the node meets the entry before it (the step back by one pair); where the node goes, the next node
// meets the same entry.
__device__ __forceinline__ uint32_t st_overlap(const Area &w, uint32_t *L, uint32_t m) {
    uint32_t out = 0;
    for (uint32_t k = 0; k < m; k++) {
        const uint32_t node = L[k];
        const uint64_t ls = w.pos[node], le = ls + w.qlen[node];
        bool stays = true;
        while (out) {
            const uint32_t top = L[out - 1];
            const uint64_t fs = w.pos[top], fe = fs + w.qlen[top];
            if (!((fs <= ls && le < fe) || (ls <= fs && fe < le))) break;
            const double former = 1.0 - (double)w.indel[top] / (double)w.total[top];
            const double latter = 1.0 - (double)w.indel[node] / (double)w.total[node];
            if (former < latter) {
                out--;
            } else {
                stays = false;
                break;
            }
        }
        if (stays) L[out++] = node;  // out <= k
    }
    return out;
}

__global__ void __launch_bounds__(ST_WAVES * 64) settle_kernel(uint32_t n_reads, const uint64_t *node_off, const jtk_settle_node_t *nodes,
                                                               const uint8_t *ops, const uint64_t *ops_off, int mode, uint8_t *gwork,
                                                               uint64_t n_total, jtk_node_stats_t *stats, uint32_t *n_kept, uint32_t *order,
                                                               uint8_t *keep, int32_t *read_status) {
    __shared__ uint64_t s_u64[ST_WAVES][2 * ST_LDS_NODES];
    __shared__ uint32_t s_u32[ST_WAVES][7 * ST_LDS_NODES];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t wave = blockIdx.x * ST_WAVES + wv, n_waves = gridDim.x * ST_WAVES;
    for (uint32_t r = wave; r < n_reads; r += n_waves) {
        const uint64_t first = node_off[r];
        const uint32_t n = (uint32_t)(node_off[r + 1] - first);
        Area w;
        if (n <= ST_LDS_NODES) {
            w.chunk = s_u64[wv];
            w.pos = s_u64[wv] + ST_LDS_NODES;
            w.qlen = s_u32[wv];
            w.fwd = s_u32[wv] + ST_LDS_NODES;
            w.score = (int32_t *)(s_u32[wv] + 2 * ST_LDS_NODES);
            w.total = s_u32[wv] + 3 * ST_LDS_NODES;
            w.indel = s_u32[wv] + 4 * ST_LDS_NODES;
            w.a = s_u32[wv] + 5 * ST_LDS_NODES;
            w.b = s_u32[wv] + 6 * ST_LDS_NODES;
        } else {  // the read's slice of nine arrays of n_total entries each
            uint32_t *u32 = (uint32_t *)(gwork + 16 * n_total);
            w.chunk = (uint64_t *)gwork + first;
            w.pos = (uint64_t *)gwork + n_total + first;
            w.qlen = u32 + first;
            w.fwd = u32 + n_total + first;
            w.score = (int32_t *)(u32 + 2 * n_total + first);
            w.total = u32 + 3 * n_total + first;
            w.indel = u32 + 4 * n_total + first;
            w.a = u32 + 5 * n_total + first;
            w.b = u32 + 6 * n_total + first;
        }
        jtk_wave_sync();  // the previous read's work area has been read to the end
        // ---- the statistics, node by node, and the keys
        int st = 0;
        for (uint32_t k = 0; k < n; k++) {
            const uint64_t e = first + k, ob = ops_off[e];
            jtk_node_stats_t s;
            const int rc = st_node_stats(ops + ob, (uint32_t)(ops_off[e + 1] - ob), nodes[e].query_len, lane, &s);
            if (st == 0) st = rc;
            if (lane == 0) {
                stats[e].score = s.score;
                stats[e].total = s.total;
                stats[e].indel = s.indel;
                stats[e].del_size = s.del_size;
                w.score[k] = s.score;
                w.total[k] = s.total;
                w.indel[k] = s.indel;
            }
        }
        uint32_t m = n;
        const bool settle = mode != JTK_SETTLE_STATS_ONLY && st == 0 && n > 0;
        if (settle) {
            for (uint32_t k = lane; k < n; k += 64) {
                const jtk_settle_node_t nd = nodes[first + k];
                w.chunk[k] = nd.chunk;
                w.pos[k] = nd.position_from_start;
                w.qlen[k] = nd.query_len;
                w.fwd[k] = nd.is_forward != 0;
            }
            jtk_wave_sync();
            st_rank_sort(w, n, nullptr, w.a, true, mode == JTK_SETTLE_BY_CHUNK_POS, lane);  // (a)
            jtk_wave_sync();
            if (lane == 0) m = st_slippy(w, w.a, n);  // (b)
            m = __shfl(m, 0, 64);
            jtk_wave_sync();
            st_rank_sort(w, m, w.a, w.b, false, true, lane);  // (c)
            jtk_wave_sync();
            if (lane == 0) m = st_overlap(w, w.b, st_slippy(w, w.b, m));  // (d), (e)
            m = __shfl(m, 0, 64);
            for (uint32_t k = lane; k < n; k += 64) w.a[k] = 0;  // now the flags
            jtk_wave_sync();
            for (uint32_t k = lane; k < m; k += 64) w.a[w.b[k]] = 1;
            jtk_wave_sync();
        }
        for (uint32_t k = lane; k < n; k += 64) {
            order[first + k] = settle ? (k < m ? w.b[k] : ST_DROPPED) : k;
            keep[first + k] = settle ? (uint8_t)w.a[k] : (uint8_t)1;
        }
        if (lane == 0) {
            n_kept[r] = m;
            read_status[r] = st;
        }
    }
}

}  // namespace

extern "C" void jtk_lc_debug_settle_timing(double *out) {
    if (out) std::memcpy(out, g_settle_timing, sizeof(g_settle_timing));
}

extern "C" int jtk_lc_settle_nodes(size_t n_reads, const uint64_t *node_off, const jtk_settle_node_t *nodes, const uint8_t *ops,
                                   const uint64_t *ops_off, int mode, jtk_node_stats_t *stats, uint32_t *n_kept, uint32_t *order, uint8_t *keep,
                                   int32_t *read_status, int device) {
    g_last_error.clear();
    std::memset(g_settle_timing, 0, sizeof(g_settle_timing));
    if (mode != JTK_SETTLE_STATS_ONLY && mode != JTK_SETTLE_BY_CHUNK_POS && mode != JTK_SETTLE_BY_CHUNK)
        return jtk_fail(JTK_ERR_INVALID_ARG, "mode is none of jtk_settle_mode");
    if (!node_off || (n_reads && (!n_kept || !read_status))) return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    if (n_reads > ST_MAX_NODES) return jtk_fail(JTK_ERR_UNSUPPORTED, "2^31 reads or more");
    if (int rc = jtk_check_offsets(n_reads, node_off, "node_off", ST_MAX_NODES)) return rc;
    const uint64_t n = node_off[n_reads];
    if (n > ST_MAX_NODES) return jtk_fail(JTK_ERR_UNSUPPORTED, "2^31 nodes or more");
    if (n && (!nodes || !ops_off || !stats || !order || !keep)) return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    if (n) {
        if (int rc = jtk_check_offsets(n, ops_off, "ops_off", ST_MAX_NODES)) return rc;
        if (ops_off[n] && !ops) return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    }
    if (int rc = jtk_require_device(device)) return rc;
    if (!n_reads) return 0;
    uint64_t n_global = 0;
    for (size_t r = 0; r < n_reads; r++) n_global += node_off[r + 1] - node_off[r] > ST_LDS_NODES;
    DevStream s;
    JTK_HIP_TRY(s.create(4));
    DevArr<uint64_t> d_node_off, d_ops_off;
    DevArr<jtk_settle_node_t> d_nodes;
    DevArr<uint8_t> d_ops, d_work, d_keep;
    DevArr<jtk_node_stats_t> d_stats;
    DevArr<uint32_t> d_kept, d_order;
    DevArr<int32_t> d_status;
    JTK_HIP_TRY(hipEventRecord(s.ev[0], s.st));
    {
        int rc;
        static const uint64_t zero = 0;  // ops_off of a call without nodes
        if ((rc = d_node_off.upload(node_off, n_reads + 1, s.st)) || (rc = d_nodes.upload(nodes, n, s.st)) ||
            (rc = d_ops_off.upload(n ? ops_off : &zero, n + 1, s.st)) || (rc = d_ops.upload(ops, n ? ops_off[n] : 0, s.st)))
            return jtk_fail(rc, "device upload failed");
    }
    JTK_HIP_TRY(d_work.alloc(n_global ? (size_t)n * ST_NODE_BYTES : 0));
    JTK_HIP_TRY(d_stats.alloc(n));
    JTK_HIP_TRY(d_stats.zero(std::max<uint64_t>(n, 1), s.st));  // the padding of jtk_node_stats_t goes back to the caller too
    JTK_HIP_TRY(d_kept.alloc(n_reads));
    JTK_HIP_TRY(d_order.alloc(n));
    JTK_HIP_TRY(d_keep.alloc(n));
    JTK_HIP_TRY(d_status.alloc(n_reads));
    JTK_HIP_TRY(hipEventRecord(s.ev[1], s.st));
    settle_kernel<<<jtk_blocks(n_reads, ST_WAVES, ST_GRID), ST_WAVES * 64, 0, s.st>>>((uint32_t)n_reads, d_node_off.cget(), d_nodes.cget(), d_ops.cget(),
                                                                                      d_ops_off.cget(), mode, d_work.get(), n, d_stats.get(),
                                                                                      d_kept.get(), d_order.get(), d_keep.get(), d_status.get());
    JTK_HIP_TRY(hipEventRecord(s.ev[2], s.st));
    std::vector<jtk_node_stats_t> h_stats(n);
    std::vector<uint32_t> h_kept(n_reads), h_order(n);
    std::vector<uint8_t> h_keep(n);
    std::vector<int32_t> h_status(n_reads);
    if (n) {
        JTK_HIP_TRY(d_stats.download(h_stats.data(), n, s.st));
        JTK_HIP_TRY(d_order.download(h_order.data(), n, s.st));
        JTK_HIP_TRY(d_keep.download(h_keep.data(), n, s.st));
    }
    JTK_HIP_TRY(d_kept.download(h_kept.data(), n_reads, s.st));
    JTK_HIP_TRY(d_status.download(h_status.data(), n_reads, s.st));
    JTK_HIP_TRY(hipEventRecord(s.ev[3], s.st));
    JTK_HIP_TRY(hipStreamSynchronize(s.st));
    JTK_HIP_TRY(hipGetLastError());
    float kernel_ms = 0.f, call_ms = 0.f;
    JTK_HIP_TRY(s.elapsed(1, 2, &kernel_ms));
    JTK_HIP_TRY(s.elapsed(0, 3, &call_ms));
    g_settle_timing[0] = (double)n_reads;
    g_settle_timing[1] = (double)n_global;
    g_settle_timing[2] = kernel_ms;
    g_settle_timing[3] = call_ms;
    if (n) {
        std::memcpy(stats, h_stats.data(), n * sizeof(jtk_node_stats_t));
        std::copy(h_order.begin(), h_order.end(), order);
        std::copy(h_keep.begin(), h_keep.end(), keep);
    }
    std::copy(h_kept.begin(), h_kept.end(), n_kept);
    std::copy(h_status.begin(), h_status.end(), read_status);
    for (const int32_t st : h_status)
        if (st) return jtk_fail(JTK_ERR_CHUNK_FAILED, "a read has a node without ops, with an op above 3, or whose ops do not take query_len bases (read_status[])");
    return 0;
}
