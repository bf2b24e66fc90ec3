// purge.hip -- jtk_lc_node_errors / jtk_lc_error_quantile / jtk_lc_estimate_error_rate / jtk_lc_purge_diverged: the step the
// reference runs right after local_clustering (`ds.purge`, cli/src/pipeline.rs:164-165), and the two functions it rests on.
//
//   Node::recover (definitions/src/lib.rs:773-813)            the alignment columns of a node against its chunk; a node's error
//                                                              rate is (columns that are not '|') / (columns), one f64 division
//                                                              (determine_chunks.rs:796-803 == estimate_error_rate.rs:68-70)
//   calc_sim_thr (determine_chunks.rs:806-823)                the value at index min(floor(n q), n - 1) of the ascending rates
//   estimate_error_rate (estimate_error_rate.rs:37-133)       alternating fit of one rate per read and one per (chunk, cluster)
//   purge_diverged_nodes (purge_diverged.rs:238-322)          clusters whose fitted rate exceeds thr are dropped with their nodes
// On the device: the column walk (one wave per node, 64 ops per step, positions from ballots), the rates, both sorts (rocprim)
// and every sum of the fit.  The fit's sums are ORDERED: a (chunk, cluster) slot adds its nodes in read order, then node order
// (one thread per slot over a stable sort of the nodes by slot), a read adds its nodes in order (one thread per read), the
// per-read residual terms are added in read order and the slots' squares in ascending chunk id (one wave, every lane the same
// sum).  No float atomics anywhere: the bits, and through the `< 0.00001` test the iteration count, are the reference's.
// The flags and the per-node write-back lists of purge_diverged_nodes are a pass over small arrays and run on the host.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "device_common.h"
#include "jtk_lc_debug.h"
#include "prim_host.h"

namespace {

constexpr uint32_t PG_NONE = 0xffffffffu;     // chunk index of a node whose chunk id is not in chunks[]
constexpr uint32_t PG_WALK_GRID = 2048;       // workgroups of the column walk (4 waves each; they loop over the nodes)
constexpr uint32_t PG_GRID = 4096;            // workgroups of the element-wise kernels
constexpr uint32_t PG_MAX_LEN = 0x7fffffffu;  // bases / ops of one node or chunk: positions are 32-bit
constexpr uint32_t PG_MAX_ITER = 100000;      // a guard: the reference would not return
constexpr uint64_t PG_NAN_BITS = 0x7ff8000000000000ull;  // the 0 / 0 of a read without nodes

thread_local double g_purge_timing[4];  // upload ms, column walk ms, device ms of the whole call, iterations

__device__ __forceinline__ uint32_t pg_upper(uint32_t b) { return b - (uint32_t)'a' < 26u ? b - 32u : b; }
__device__ __forceinline__ uint32_t pg_below(uint64_t mask) {  // set bits of `mask` below this lane
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// Node::recover's alignment row, counted: one wave per node, one op per lane and step.  The read and template positions of a
// lane are the wave's running positions plus the number of lanes below it whose op consumes that sequence; a position is
// compared with its sequence's length before anything is loaded from it.  The first op in order that is no op code or that
// steps past a sequence decides the node's status.
__global__ void __launch_bounds__(256) node_errors_kernel(uint32_t n_nodes, const uint32_t *cidx, const uint64_t *seq_off, const uint64_t *ops_off,
                                                          const uint64_t *tmpl_off, const uint8_t *seq, const uint8_t *ops, const uint8_t *tmpl,
                                                          uint32_t *err_num, uint32_t *err_len, int32_t *status) {
    const uint32_t lane = threadIdx.x & 63u, wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t e = wave; e < n_nodes; e += n_waves) {
        const uint32_t c = cidx[e];
        uint32_t errs = 0, cols = 0;
        int32_t st = 0;
        if (c == PG_NONE) {
            st = JTK_ERR_CHUNK_FAILED;  // chunks[&node.chunk]
        } else {
            const uint64_t ob = ops_off[e], sb = seq_off[e], tb = tmpl_off[c];
            const uint32_t on = (uint32_t)(ops_off[e + 1] - ob), sn = (uint32_t)(seq_off[e + 1] - sb), tn = (uint32_t)(tmpl_off[c + 1] - tb);
            uint32_t q = 0, r = 0;  // wave-uniform
            for (uint32_t base = 0; base < on; base += 64) {
                const uint32_t i = base + lane;
                const bool active = i < on;
                const uint32_t op = active ? ops[ob + i] : 0xffu;
                const bool bad = active && op > 3u;
                const bool cr = active && op <= 2u;                 // Match, Mismatch, Ins take a read base
                const bool ct = active && (op <= 1u || op == 3u);   // Match, Mismatch, Del take a template base
                const uint64_t mr = __ballot(cr), mt = __ballot(ct), mb = __ballot(bad);
                const uint32_t qp = q + pg_below(mr), rp = r + pg_below(mt);
                const bool over = (cr && qp >= sn) || (ct && rp >= tn);
                const uint64_t fail = mb | __ballot(over);
                if (fail) {
                    st = (mb & (fail & (0ull - fail))) ? JTK_ERR_INVALID_ARG : JTK_ERR_OPS_MISMATCH;
                    break;
                }
                bool not_bar = active && op >= 2u;
                if (cr && ct) not_bar = pg_upper(seq[sb + qp]) != pg_upper(tmpl[tb + rp]);
                errs += (uint32_t)__popcll(__ballot(not_bar));
                q += (uint32_t)__popcll(mr);
                r += (uint32_t)__popcll(mt);
            }
            cols = on;
            if (st == 0 && on == 0) st = JTK_ERR_CHUNK_FAILED;  // 0 / 0
        }
        if (lane == 0) {
            err_num[e] = st ? 0u : errs;
            err_len[e] = st ? 0u : cols;
            status[e] = st;
        }
    }
}

__global__ void rate_kernel(uint32_t n, const uint32_t *num, const uint32_t *len, double *rate) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) rate[e] = (double)num[e] / (double)len[e];
}
__global__ void fill_kernel(uint32_t n, double *p, double v) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = v;
}
__global__ void iota_kernel(uint32_t n, uint32_t *p) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = i;
}

// estimate_error_rate.rs:80-94: one thread per (chunk, cluster) slot adds `error - read_err` over its nodes, which `order`
// lists in read order, then node order; max(., 0) / (count + 0.1), f64::max taking the number where the sum is NaN
__global__ void slot_kernel(uint32_t n_slots, const uint32_t *slot_start, const uint32_t *order, const double *rate, const uint32_t *read_of,
                            const double *read_err, double *chunk_err) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < n_slots; s += stride) {
        const uint32_t b = slot_start[s], e = slot_start[s + 1];
        double sum = 0.0;
        for (uint32_t i = b; i < e; i++) {
            const uint32_t n = order[i];
            sum += rate[n] - read_err[read_of[n]];
        }
        chunk_err[s] = (sum > 0.0 ? sum : 0.0) / ((double)(e - b) + 0.1);
    }
}

// :96-102 (update != 0) and the read's term of `residual` :23-30 with the read rate that then holds: one thread per read
__global__ void read_kernel(uint32_t n_reads, const uint64_t *node_off, const uint32_t *slot, const double *rate, const double *chunk_err,
                            double *read_err, double *term, int update) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += stride) {
        const uint64_t b = node_off[r], e = node_off[r + 1];
        double re;
        if (update) {
            double s = 0.0;
            for (uint64_t i = b; i < e; i++) s += rate[i] - chunk_err[slot[i]];
            re = e == b ? __longlong_as_double((long long)PG_NAN_BITS) : s / (double)(e - b);
            read_err[r] = re;
        } else {
            re = read_err[r];
        }
        double t = 0.0;
        for (uint64_t i = b; i < e; i++) {
            const double x = rate[i] - re - chunk_err[slot[i]];
            t += x * x;
        }
        term[r] = t;
    }
}

// a[idx[0]], a[idx[1]], ... (idx == nullptr: a[0], a[1], ...) added from 0 in that order, squared first where `square`; every
// lane of the wave ends with the same sum (64 values are loaded at once, then added one by one)
__device__ __forceinline__ double pg_ordered_sum(uint32_t n, const double *a, const uint32_t *idx, bool square, uint32_t lane) {
    double acc = 0.0;
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t i = base + lane;
        double v = 0.0;
        if (i < n) v = a[idx ? idx[i] : i];
        if (square) v = v * v;
        const uint32_t m = n - base < 64u ? n - base : 64u;
        for (uint32_t j = 0; j < m; j++) acc += __shfl(v, (int)j, 64);
    }
    return acc;
}
// `residual` :20-34: the per-read terms in read order, plus the squares of the slots' rates in the reference's flat order
__global__ void __launch_bounds__(64) resid_kernel(uint32_t n_reads, const double *term, uint32_t n_slots, const uint32_t *reg_order,
                                                   const double *chunk_err, double *out) {
    const uint32_t lane = threadIdx.x;
    const double residual = pg_ordered_sum(n_reads, term, nullptr, false, lane);
    const double reg_term = pg_ordered_sum(n_slots, chunk_err, reg_order, true, lane);
    if (lane == 0) *out = residual + reg_term;
}

// :109-122: error - (chunk + read), squared
__global__ void square_kernel(uint32_t n, const uint32_t *slot, const uint32_t *read_of, const double *rate, const double *chunk_err,
                              const double *read_err, double *sq) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
        const double x = rate[e] - (chunk_err[slot[e]] + read_err[read_of[e]]);
        sq[e] = x * x;
    }
}

// the value at `idx` of the ascending order of n non-negative doubles (their bit patterns sort as unsigned integers)
int pg_select(const DevStream &s, uint32_t n, const double *d_vals, uint32_t idx, double *out) {
    DevArr<uint64_t> d_sorted;
    RocTemp tmp;
    JTK_HIP_TRY(d_sorted.alloc(n));
    JTK_HIP_TRY(tmp.run([&](void *t, size_t &bytes) {
        return rocprim::radix_sort_keys(t, bytes, (const uint64_t *)d_vals, d_sorted.get(), (size_t)n, 0u, 64u, s.st);
    }));
    JTK_HIP_TRY(d_sorted.download((uint64_t *)out, 1, s.st, idx));
    JTK_HIP_TRY(hipStreamSynchronize(s.st));
    JTK_HIP_TRY(hipGetLastError());
    return 0;
}

// calc_sim_thr's index (determine_chunks.rs:821)
uint32_t pg_quantile_index(uint32_t n, double q) { return (uint32_t)std::min<uint64_t>((uint64_t)std::floor((double)n * q), (uint64_t)n - 1); }

// chunks[] by id: `sorted` = indices into chunks[] ascending by id; JTK_ERR_INVALID_ARG where an id repeats
int pg_index_chunks(size_t n_chunks, const jtk_cc_chunk_t *chunks, std::vector<uint32_t> &sorted) {
    sorted.resize(n_chunks);
    for (size_t c = 0; c < n_chunks; c++) sorted[c] = (uint32_t)c;
    std::sort(sorted.begin(), sorted.end(), [&](uint32_t a, uint32_t b) { return chunks[a].id < chunks[b].id; });
    for (size_t c = 1; c < n_chunks; c++)
        if (chunks[sorted[c]].id == chunks[sorted[c - 1]].id) return jtk_fail(JTK_ERR_INVALID_ARG, "chunk ids repeat");
    return 0;
}
uint32_t pg_chunk_of(const jtk_cc_chunk_t *chunks, const std::vector<uint32_t> &sorted, uint64_t id) {
    auto it = std::lower_bound(sorted.begin(), sorted.end(), id, [&](uint32_t a, uint64_t v) { return chunks[a].id < v; });
    return it != sorted.end() && chunks[*it].id == id ? *it : PG_NONE;
}

int pg_check_reads(size_t n_reads, const uint64_t *node_off) {
    if (!node_off) return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    if (int rc = jtk_check_offsets(n_reads, node_off, "node_off")) return rc;
    if (n_reads >= PG_NONE || node_off[n_reads] >= PG_NONE) return jtk_fail(JTK_ERR_UNSUPPORTED, "more than 2^32 - 2 reads or nodes");
    return 0;
}

// What the device holds between the steps of one call.
struct Work {
    DevStream s;  // two pairs of events: create(4)
    uint32_t n_nodes = 0, n_reads = 0;
    DevArr<uint32_t> d_num, d_len;
    DevArr<double> d_rate;
    std::vector<uint32_t> cidx;  // per node: index into chunks[], PG_NONE for an id that is not there
};

// the sequences of a data set up, the column walk, its three arrays back
int pg_walk(Work &w, size_t n_chunks, const uint8_t *seq_bases, const uint64_t *seq_off, const uint8_t *ops, const uint64_t *ops_off,
            const uint8_t *tmpl_bases, const uint64_t *tmpl_off, std::vector<uint32_t> &num, std::vector<uint32_t> &len, std::vector<int32_t> &status) {
    const uint32_t n = w.n_nodes;
    DevArr<uint32_t> d_cidx;
    DevArr<uint64_t> d_seq_off, d_ops_off, d_tmpl_off;
    DevArr<uint8_t> d_seq, d_ops, d_tmpl;
    DevArr<int32_t> d_status;
    JTK_HIP_TRY(hipEventRecord(w.s.ev[0], w.s.st));
    {  // straight from the caller's arrays: about a gigabyte at the headline's size
        int rc;
        if ((rc = d_cidx.upload(w.cidx, w.s.st)) || (rc = d_seq_off.upload(seq_off, (size_t)n + 1, w.s.st)) ||
            (rc = d_ops_off.upload(ops_off, (size_t)n + 1, w.s.st)) || (rc = d_tmpl_off.upload(tmpl_off, n_chunks + 1, w.s.st)) ||
            (rc = d_seq.upload(seq_bases, seq_off[n], w.s.st)) || (rc = d_ops.upload(ops, ops_off[n], w.s.st)) ||
            (rc = d_tmpl.upload(tmpl_bases, tmpl_off[n_chunks], w.s.st)))
            return jtk_fail(rc, "device upload failed");
        JTK_HIP_TRY(hipStreamSynchronize(w.s.st));
    }
    JTK_HIP_TRY(w.d_num.alloc(n));
    JTK_HIP_TRY(w.d_len.alloc(n));
    JTK_HIP_TRY(d_status.alloc(n));
    JTK_HIP_TRY(hipEventRecord(w.s.ev[1], w.s.st));
    node_errors_kernel<<<jtk_blocks(n, 4, PG_WALK_GRID), 256, 0, w.s.st>>>(n, d_cidx.cget(), d_seq_off.cget(), d_ops_off.cget(), d_tmpl_off.cget(), d_seq.cget(),
                                                                         d_ops.cget(), d_tmpl.cget(), w.d_num.get(), w.d_len.get(), d_status.get());
    JTK_HIP_TRY(hipEventRecord(w.s.ev[2], w.s.st));
    num.resize(n);
    len.resize(n);
    status.resize(n);
    JTK_HIP_TRY(w.d_num.download(num.data(), n, w.s.st));
    JTK_HIP_TRY(w.d_len.download(len.data(), n, w.s.st));
    JTK_HIP_TRY(d_status.download(status.data(), n, w.s.st));
    JTK_HIP_TRY(hipStreamSynchronize(w.s.st));
    JTK_HIP_TRY(hipGetLastError());
    float ms = 0.f;
    JTK_HIP_TRY(w.s.elapsed(0, 1, &ms));
    g_purge_timing[0] = ms;
    JTK_HIP_TRY(w.s.elapsed(1, 2, &ms));
    g_purge_timing[1] = ms;
    return 0;
}

int pg_rates(Work &w) {  // d_num, d_len -> d_rate
    JTK_HIP_TRY(w.d_rate.alloc(w.n_nodes));
    rate_kernel<<<jtk_blocks(w.n_nodes, 256, PG_GRID), 256, 0, w.s.st>>>(w.n_nodes, w.d_num.cget(), w.d_len.cget(), w.d_rate.get());
    return 0;
}

struct Fit {
    std::vector<double> read_err, chunk_err;
    std::vector<uint64_t> slot_off;  // n_chunks + 1: the prefix sum of cluster_num
    std::vector<uint32_t> slot;      // per node
    double median = 0.0;
    uint32_t n_iter = 0;
};

// the slots of a data set; JTK_ERR_CHUNK_FAILED where the reference indexes past its tables (:49-50)
int pg_slots(const Work &w, const jtk_cc_node_t *nodes, size_t n_chunks, const jtk_cc_chunk_t *chunks, Fit &f) {
    f.slot_off.assign(n_chunks + 1, 0);
    for (size_t c = 0; c < n_chunks; c++) f.slot_off[c + 1] = f.slot_off[c] + chunks[c].cluster_num;
    if (f.slot_off[n_chunks] >= PG_NONE) return jtk_fail(JTK_ERR_UNSUPPORTED, "more than 2^32 - 2 clusters");
    f.slot.resize(w.n_nodes);
    for (uint32_t e = 0; e < w.n_nodes; e++) {
        const uint32_t c = w.cidx[e];
        if (c == PG_NONE) return jtk_fail(JTK_ERR_CHUNK_FAILED, "a node names a chunk id that is not in chunks[]");
        if (nodes[e].cluster >= chunks[c].cluster_num) return jtk_fail(JTK_ERR_CHUNK_FAILED, "a node's cluster is not below its chunk's cluster_num");
        f.slot[e] = (uint32_t)(f.slot_off[c] + nodes[e].cluster);
    }
    return 0;
}

// estimate_error_rate.rs:37-133 on the rates in w.d_rate; `sorted` = chunks[] ascending by id (the reference's flat order)
int pg_fit(Work &w, const uint64_t *node_off, const std::vector<uint32_t> &sorted, double fallback, Fit &f) {
    const uint32_t n = w.n_nodes, n_reads = w.n_reads, n_slots = (uint32_t)f.slot_off.back();
    std::vector<uint32_t> read_of(n), slot_start(n_slots + 1, 0), reg_order;
    for (uint32_t r = 0; r < n_reads; r++)
        for (uint64_t e = node_off[r]; e < node_off[r + 1]; e++) read_of[e] = r;
    for (uint32_t e = 0; e < n; e++) slot_start[f.slot[e] + 1]++;
    for (uint32_t s = 0; s < n_slots; s++) slot_start[s + 1] += slot_start[s];
    reg_order.reserve(n_slots);
    for (const uint32_t c : sorted)
        for (uint64_t s = f.slot_off[c]; s < f.slot_off[c + 1]; s++) reg_order.push_back((uint32_t)s);
    const hipStream_t st = w.s.st;
    DevArr<uint64_t> d_off;
    DevArr<uint32_t> d_slot, d_read_of, d_start, d_reg, d_iota, d_slot_s, d_order;
    DevArr<double> d_read_err, d_chunk_err, d_term, d_resid, d_sq;
    RocTemp tmp;
    {
        int rc;
        const std::vector<uint64_t> off_v(node_off, node_off + n_reads + 1);
        if ((rc = d_off.upload(off_v, st)) || (rc = d_slot.upload(f.slot, st)) || (rc = d_read_of.upload(read_of, st)) ||
            (rc = d_start.upload(slot_start, st)) || (rc = d_reg.upload(reg_order, st)))
            return jtk_fail(rc, "device upload failed");
        JTK_HIP_TRY(hipStreamSynchronize(st));
    }
    JTK_HIP_TRY(d_iota.alloc(n));
    JTK_HIP_TRY(d_slot_s.alloc(n));
    JTK_HIP_TRY(d_order.alloc(n));
    JTK_HIP_TRY(d_read_err.alloc(n_reads));
    JTK_HIP_TRY(d_chunk_err.alloc(n_slots));
    JTK_HIP_TRY(d_term.alloc(n_reads));
    JTK_HIP_TRY(d_resid.alloc(1));
    JTK_HIP_TRY(d_sq.alloc(n));
    const uint32_t node_grid = jtk_blocks(n, 256, PG_GRID), read_grid = jtk_blocks(n_reads, 256, PG_GRID), slot_grid = jtk_blocks(n_slots, 256, PG_GRID);
    iota_kernel<<<node_grid, 256, 0, st>>>(n, d_iota.get());
    {  // the nodes by slot, once: the radix sort is stable, so a slot's run lists its nodes in read order, then node order
        unsigned end_bit = 1;
        while (end_bit < 32 && (n_slots >> end_bit)) end_bit++;
        JTK_HIP_TRY(tmp.run([&](void *t, size_t &bytes) {
            return rocprim::radix_sort_pairs(t, bytes, d_slot.cget(), d_slot_s.get(), d_iota.cget(), d_order.get(), (size_t)n, 0u, end_bit, st);
        }));
    }
    const uint32_t *slot = d_slot.cget(), *rd_of = d_read_of.cget();
    const double *rate = w.d_rate.cget();
    double *read_err = d_read_err.get(), *chunk_err = d_chunk_err.get(), *term = d_term.get();
    auto residual = [&](int update, double *out) -> int {
        read_kernel<<<read_grid, 256, 0, st>>>(n_reads, d_off.cget(), slot, rate, chunk_err, read_err, term, update);
        resid_kernel<<<1, 64, 0, st>>>(n_reads, term, n_slots, d_reg.cget(), chunk_err, d_resid.get());
        JTK_HIP_TRY(d_resid.download(out, 1, st));
        JTK_HIP_TRY(hipStreamSynchronize(st));
        JTK_HIP_TRY(hipGetLastError());
        return 0;
    };
    fill_kernel<<<read_grid, 256, 0, st>>>(n_reads, read_err, fallback);  // :55-58
    fill_kernel<<<slot_grid, 256, 0, st>>>(n_slots, chunk_err, 0.0);
    double current = 0.0;
    if (int rc = residual(0, &current)) return rc;  // :77
    for (f.n_iter = 0;;) {
        if (f.n_iter == PG_MAX_ITER) return jtk_fail(JTK_ERR_CHUNK_FAILED, "estimate_error_rate: no convergence in 100,000 iterations");
        f.n_iter++;
        slot_kernel<<<slot_grid, 256, 0, st>>>(n_slots, d_start.cget(), d_order.cget(), rate, rd_of, read_err, chunk_err);
        double resid = 0.0;
        if (int rc = residual(1, &resid)) return rc;
        if (std::fabs(current - resid) < 0.00001) break;  // :104
        current = resid;
    }
    square_kernel<<<node_grid, 256, 0, st>>>(n, slot, rd_of, rate, chunk_err, read_err, d_sq.get());
    double sq = 0.0;
    if (int rc = pg_select(w.s, n, d_sq.cget(), n / 2, &sq)) return rc;  // :123-127
    f.median = std::sqrt(sq);
    f.read_err.resize(n_reads);
    f.chunk_err.resize(n_slots);
    if (n_reads) JTK_HIP_TRY(d_read_err.download(f.read_err.data(), n_reads, st));
    if (n_slots) JTK_HIP_TRY(d_chunk_err.download(f.chunk_err.data(), n_slots, st));
    JTK_HIP_TRY(hipStreamSynchronize(st));
    JTK_HIP_TRY(hipGetLastError());
    return 0;
}

// what every call checks of the flattened data set before it looks at a node; fills w.cidx
int pg_open(Work &w, size_t n_reads, const uint64_t *node_off, const jtk_cc_node_t *nodes, size_t n_chunks, const jtk_cc_chunk_t *chunks,
            std::vector<uint32_t> &sorted) {
    if (int rc = pg_check_reads(n_reads, node_off)) return rc;
    w.n_reads = (uint32_t)n_reads;
    w.n_nodes = (uint32_t)node_off[n_reads];
    if ((w.n_nodes && !nodes) || (n_chunks && !chunks)) return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    if (n_chunks >= PG_NONE) return jtk_fail(JTK_ERR_UNSUPPORTED, "more than 2^32 - 2 chunks");
    if (int rc = pg_index_chunks(n_chunks, chunks, sorted)) return rc;
    w.cidx.resize(w.n_nodes);
    for (uint32_t e = 0; e < w.n_nodes; e++) w.cidx[e] = pg_chunk_of(chunks, sorted, nodes[e].chunk);
    return 0;
}
int pg_check_sequences(const Work &w, size_t n_chunks, const uint8_t *seq_bases, const uint64_t *seq_off, const uint8_t *ops, const uint64_t *ops_off,
                       const uint8_t *tmpl_bases, const uint64_t *tmpl_off) {
    if (!seq_off || !ops_off || !tmpl_off) return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    if (int rc = jtk_check_offsets(w.n_nodes, seq_off, "seq_off", PG_MAX_LEN)) return rc;  // no slice of 2^31 bytes or more
    if (int rc = jtk_check_offsets(w.n_nodes, ops_off, "ops_off", PG_MAX_LEN)) return rc;
    if (int rc = jtk_check_offsets(n_chunks, tmpl_off, "tmpl_off", PG_MAX_LEN)) return rc;
    if ((seq_off[w.n_nodes] && !seq_bases) || (ops_off[w.n_nodes] && !ops) || (tmpl_off[n_chunks] && !tmpl_bases))
        return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    return 0;
}

int pg_total_ms(Work &w) {  // ev[0] (the upload's start, or this call's) to now
    JTK_HIP_TRY(hipEventRecord(w.s.ev[3], w.s.st));
    JTK_HIP_TRY(hipEventSynchronize(w.s.ev[3]));
    float ms = 0.f;
    JTK_HIP_TRY(w.s.elapsed(0, 3, &ms));
    g_purge_timing[2] = ms;
    return 0;
}

}  // namespace

extern "C" void jtk_lc_debug_purge_timing(double *out) {
    if (out) std::memcpy(out, g_purge_timing, sizeof(g_purge_timing));
}

extern "C" int jtk_lc_node_errors(size_t n_reads, const uint64_t *node_off, const jtk_cc_node_t *nodes, size_t n_chunks, const jtk_cc_chunk_t *chunks,
                                  const uint8_t *seq_bases, const uint64_t *seq_off, const uint8_t *ops, const uint64_t *ops_off,
                                  const uint8_t *tmpl_bases, const uint64_t *tmpl_off, uint32_t *err_num, uint32_t *err_len, int32_t *status,
                                  int device) {
    g_last_error.clear();
    Work w;
    std::vector<uint32_t> sorted;
    if (int rc = pg_open(w, n_reads, node_off, nodes, n_chunks, chunks, sorted)) return rc;
    if (int rc = pg_check_sequences(w, n_chunks, seq_bases, seq_off, ops, ops_off, tmpl_bases, tmpl_off)) return rc;
    if (w.n_nodes && (!err_num || !err_len || !status)) return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    if (int rc = jtk_require_device(device)) return rc;
    if (!w.n_nodes) return 0;
    JTK_HIP_TRY(w.s.create(4));
    std::vector<uint32_t> num, len;
    std::vector<int32_t> st;
    if (int rc = pg_walk(w, n_chunks, seq_bases, seq_off, ops, ops_off, tmpl_bases, tmpl_off, num, len, st)) return rc;
    if (int rc = pg_total_ms(w)) return rc;
    std::copy(num.begin(), num.end(), err_num);
    std::copy(len.begin(), len.end(), err_len);
    std::copy(st.begin(), st.end(), status);
    for (const int32_t s : st)
        if (s) return jtk_fail(JTK_ERR_CHUNK_FAILED, "a node's ops do not fit its sequences, or its chunk is not in chunks[] (status[])");
    return 0;
}

extern "C" int jtk_lc_error_quantile(size_t n_nodes, const uint32_t *err_num, const uint32_t *err_len, double quantile, double *out, int device) {
    g_last_error.clear();
    if (!err_num || !err_len || !out) return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    if (n_nodes == 0) return jtk_fail(JTK_ERR_INVALID_ARG, "no nodes (the reference indexes an empty list)");
    if (!(quantile >= 0.0 && quantile <= 1.0)) return jtk_fail(JTK_ERR_INVALID_ARG, "quantile outside [0, 1]");
    if (n_nodes >= PG_NONE) return jtk_fail(JTK_ERR_UNSUPPORTED, "more than 2^32 - 2 nodes");
    for (size_t e = 0; e < n_nodes; e++)
        if (err_len[e] == 0) return jtk_fail(JTK_ERR_INVALID_ARG, "a node without columns");
    if (int rc = jtk_require_device(device)) return rc;
    Work w;
    w.n_nodes = (uint32_t)n_nodes;
    JTK_HIP_TRY(w.s.create(4));
    {
        int rc;
        const std::vector<uint32_t> nv(err_num, err_num + n_nodes), lv(err_len, err_len + n_nodes);
        if ((rc = w.d_num.upload(nv, w.s.st)) || (rc = w.d_len.upload(lv, w.s.st))) return jtk_fail(rc, "device upload failed");
        JTK_HIP_TRY(hipStreamSynchronize(w.s.st));
    }
    if (int rc = pg_rates(w)) return rc;
    double v = 0.0;
    if (int rc = pg_select(w.s, w.n_nodes, w.d_rate.cget(), pg_quantile_index(w.n_nodes, quantile), &v)) return rc;
    *out = v;
    return 0;
}

extern "C" int jtk_lc_estimate_error_rate(size_t n_reads, const uint64_t *node_off, const jtk_cc_node_t *nodes, const uint32_t *err_num,
                                          const uint32_t *err_len, size_t n_chunks, const jtk_cc_chunk_t *chunks, double fallback, double *read_err,
                                          double *chunk_err, uint64_t *chunk_err_off, size_t chunk_err_cap, double *median_of_sqrt_err,
                                          uint32_t *n_iter, int device) {
    g_last_error.clear();
    Work w;
    std::vector<uint32_t> sorted;
    if (int rc = pg_open(w, n_reads, node_off, nodes, n_chunks, chunks, sorted)) return rc;
    if (!err_num || !err_len || !chunk_err_off || !median_of_sqrt_err || !n_iter || (n_reads && !read_err))
        return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    if (w.n_nodes == 0) return jtk_fail(JTK_ERR_INVALID_ARG, "no nodes (the reference takes the median of an empty list)");
    for (uint32_t e = 0; e < w.n_nodes; e++)
        if (err_len[e] == 0) return jtk_fail(JTK_ERR_INVALID_ARG, "a node without columns");
    Fit f;
    if (int rc = pg_slots(w, nodes, n_chunks, chunks, f)) return rc;
    if (f.slot_off.back() > chunk_err_cap || (f.slot_off.back() && !chunk_err)) return jtk_fail(JTK_ERR_INVALID_ARG, "chunk_err_cap is too small");
    if (int rc = jtk_require_device(device)) return rc;
    JTK_HIP_TRY(w.s.create(4));
    JTK_HIP_TRY(hipEventRecord(w.s.ev[0], w.s.st));
    {
        int rc;
        const std::vector<uint32_t> nv(err_num, err_num + w.n_nodes), lv(err_len, err_len + w.n_nodes);
        if ((rc = w.d_num.upload(nv, w.s.st)) || (rc = w.d_len.upload(lv, w.s.st))) return jtk_fail(rc, "device upload failed");
        JTK_HIP_TRY(hipStreamSynchronize(w.s.st));
    }
    if (int rc = pg_rates(w)) return rc;
    if (int rc = pg_fit(w, node_off, sorted, fallback, f)) return rc;
    if (int rc = pg_total_ms(w)) return rc;
    g_purge_timing[3] = f.n_iter;
    std::copy(f.read_err.begin(), f.read_err.end(), read_err);
    std::copy(f.chunk_err.begin(), f.chunk_err.end(), chunk_err);
    std::copy(f.slot_off.begin(), f.slot_off.end(), chunk_err_off);
    *median_of_sqrt_err = f.median;
    *n_iter = f.n_iter;
    return 0;
}

extern "C" int jtk_lc_purge_diverged(size_t n_reads, const uint64_t *node_off, const jtk_cc_node_t *nodes, size_t n_post, size_t n_chunks,
                                     jtk_cc_chunk_t *chunks, const uint8_t *seq_bases, const uint64_t *seq_off, const uint8_t *ops,
                                     const uint64_t *ops_off, const uint8_t *tmpl_bases, const uint64_t *tmpl_off, double thr, uint8_t *diverged,
                                     uint64_t *chunk_err_off, size_t slot_cap, uint8_t *keep, uint64_t *cluster_out, uint8_t *touched,
                                     uint8_t *post_keep, uint64_t *purged, size_t purged_cap, size_t *n_purged, double *read_err, double *chunk_err,
                                     double *median_of_sqrt_err, int device) {
    g_last_error.clear();
    Work w;
    std::vector<uint32_t> sorted;
    if (int rc = pg_open(w, n_reads, node_off, nodes, n_chunks, chunks, sorted)) return rc;
    if (int rc = pg_check_sequences(w, n_chunks, seq_bases, seq_off, ops, ops_off, tmpl_bases, tmpl_off)) return rc;
    if (!chunk_err_off || !n_purged || (w.n_nodes && (!keep || !cluster_out || !touched)) || (n_post && !post_keep))
        return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    for (uint32_t e = 0; e < w.n_nodes; e++)
        if (nodes[e].post_off > n_post || nodes[e].post_len > n_post - nodes[e].post_off)
            return jtk_fail(JTK_ERR_INVALID_ARG, "a node's posterior lies outside n_post");
    if (w.n_nodes == 0) return jtk_fail(JTK_ERR_INVALID_ARG, "no nodes (the reference indexes an empty list)");
    if (int rc = jtk_require_device(device)) return rc;
    JTK_HIP_TRY(w.s.create(4));
    // ---- get_diverged_clusters :299-309 on the device: the rates, their 0.5 quantile, the fit
    std::vector<uint32_t> num, len;
    std::vector<int32_t> st;
    if (int rc = pg_walk(w, n_chunks, seq_bases, seq_off, ops, ops_off, tmpl_bases, tmpl_off, num, len, st)) return rc;
    for (const int32_t s : st)
        if (s) return jtk_fail(JTK_ERR_CHUNK_FAILED, "a node's ops do not fit its sequences, or its chunk is not in chunks[]");
    Fit f;
    if (int rc = pg_slots(w, nodes, n_chunks, chunks, f)) return rc;
    const uint64_t n_slots = f.slot_off.back();
    if (n_slots > slot_cap || (n_slots && !diverged)) return jtk_fail(JTK_ERR_INVALID_ARG, "slot_cap is too small");
    if (int rc = pg_rates(w)) return rc;
    double fallback = 0.0;
    if (int rc = pg_select(w.s, w.n_nodes, w.d_rate.cget(), pg_quantile_index(w.n_nodes, 0.5), &fallback)) return rc;  // :301
    if (int rc = pg_fit(w, node_off, sorted, fallback, f)) return rc;
    if (int rc = pg_total_ms(w)) return rc;
    g_purge_timing[3] = f.n_iter;
    // ---- host: the flags (:304-308, :241-249), then the lists of :261-295 -- nothing is written before the last check
    std::vector<uint8_t> flag(n_slots, 0);
    std::vector<uint32_t> n_flag(n_chunks, 0);
    for (size_t c = 0; c < n_chunks; c++) {
        uint32_t k = 0;
        for (uint64_t s = f.slot_off[c]; s < f.slot_off[c + 1]; s++) k += (flag[s] = thr < f.chunk_err[s]);
        if (k == chunks[c].cluster_num) {  // all of them: "the fault of the consensus"
            for (uint64_t s = f.slot_off[c]; s < f.slot_off[c + 1]; s++) flag[s] = 0;
            k = 0;
        }
        n_flag[c] = k;
    }
    std::vector<uint64_t> purged_v;
    for (const uint32_t c : sorted)
        if (n_flag[c]) purged_v.push_back(chunks[c].id);
    if (purged_v.size() > purged_cap || (purged_v.size() && !purged)) return jtk_fail(JTK_ERR_INVALID_ARG, "purged_cap is too small");
    for (uint32_t e = 0; e < w.n_nodes; e++) {  // remove_diverged :318-321 indexes cluster_info by the posterior's positions
        const uint32_t c = w.cidx[e];
        if (n_flag[c] && !flag[f.slot[e]] && nodes[e].post_len > chunks[c].cluster_num)
            return jtk_fail(JTK_ERR_CHUNK_FAILED, "a posterior longer than cluster_num in a chunk that loses a cluster");
    }
    std::memset(post_keep, 1, n_post);
    for (uint32_t e = 0; e < w.n_nodes; e++) {
        const uint32_t c = w.cidx[e];
        const uint8_t *info = flag.data() + f.slot_off[c];
        const bool kept = !flag[f.slot[e]];
        uint64_t below = 0;
        for (uint64_t q = 0; q < nodes[e].cluster; q++) below += info[q];
        keep[e] = kept;
        cluster_out[e] = kept ? nodes[e].cluster - below : nodes[e].cluster;
        touched[e] = kept && n_flag[c];
        if (touched[e])
            for (uint32_t q = 0; q < nodes[e].post_len; q++) post_keep[nodes[e].post_off + q] = !info[q];
    }
    for (size_t c = 0; c < n_chunks; c++) chunks[c].cluster_num -= n_flag[c];
    std::copy(flag.begin(), flag.end(), diverged);
    std::copy(f.slot_off.begin(), f.slot_off.end(), chunk_err_off);
    std::copy(purged_v.begin(), purged_v.end(), purged);
    *n_purged = purged_v.size();
    if (read_err) std::copy(f.read_err.begin(), f.read_err.end(), read_err);
    if (chunk_err) std::copy(f.chunk_err.begin(), f.chunk_err.end(), chunk_err);
    if (median_of_sqrt_err) *median_of_sqrt_err = f.median;
    return 0;
}
