// session_plan.h -- the arithmetic of a resident batch, without HIP: from the caller's chunk and read descriptors to every
// ReadMeta / ChunkMeta offset, the buffer totals, the pair-kernel item list, the wide-band census, the chain's launch classes
// and the wave and stripe counts.  The kernels trust all of it blindly -- a wrong stride is an out-of-bounds access, a chunk in
// the wrong chain class a launch beyond LDS -- so it is kept where a plain C++ compiler and a sanitizer reach it
// (tests/test_session_plan.py).  session.hip turns a plan into allocations and uploads and computes none of this itself;
// session_features.hip plans its two chain launches with the same helpers.  No global state, no environment.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "batch_types.h"
#include "chain_layout.h"
#include "jtk_lc.h"

#define JTK_CU_LDS_BYTES (160u * 1024u)  // a CU's LDS: the most one workgroup can have

// ---- the chain's launches

struct ChainDims {
    uint32_t n, d, k;  // reads, columns, clusters
};

// what one clustering() call of a chunk needs room for
inline ChainDims chain_dims_of(const ChunkMeta &cm) {
    ChainDims x;
    x.n = cm.n_reads;
    x.k = std::min<uint32_t>(std::max<uint32_t>(cm.copy_num, 2u), JTK_MAX_COPY);
    // a chunk picks at most ROUND * max(copy_num, 2) columns (pseudo_mcmc.rs:421,527,532)
    x.d = std::min<uint32_t>(JTK_MAX_DIM, 3u * std::max<uint32_t>(cm.copy_num, 2u));
    return x;
}

// the maxima a launch of `members` is sized for, from `floor` upwards
template <class DimsOf>
ChainDims chain_maxima(const std::vector<uint32_t> &members, ChainDims floor, DimsOf dims_of) {
    ChainDims m = floor;
    for (uint32_t c : members) {
        const ChainDims x = dims_of(c);
        m.n = std::max(m.n, x.n);
        m.d = std::max(m.d, x.d);
        m.k = std::max(m.k, x.k);
    }
    return m;
}

// Fits a launch under `limit` bytes of LDS.  A launch is sized for its members' maxima of (reads, columns, clusters): THAT
// combination has to stay below the limit, not just every member's own need, and the maxima can combine beyond any one
// member's.  While they do, the worst member by `less` is handed on to `evicted`.  Returns the maxima of what stays.
template <class DimsOf, class Less>
ChainDims chain_fit_class(std::vector<uint32_t> &members, std::vector<uint32_t> &evicted, size_t limit, ChainDims floor,
                          DimsOf dims_of, Less less) {
    for (;;) {
        const ChainDims m = chain_maxima(members, floor, dims_of);
        if (members.empty() || mcmc_lds_bytes(m.n, m.d, m.k) <= limit) return m;
        auto worst = std::max_element(members.begin(), members.end(), less);
        evicted.push_back(*worst);
        members.erase(worst);
    }
}

// The global-memory launch: one workgroup per chunk, each with its own slice of one workspace.  Returns the workspace's bytes.
template <class DimsOf>
uint64_t chain_ws_offsets(const std::vector<uint32_t> &members, DimsOf dims_of, std::vector<uint64_t> &ws_off) {
    uint64_t ws = 0;
    ws_off.clear();
    for (uint32_t c : members) {
        const ChainDims x = dims_of(c);
        ws_off.push_back(ws);
        ws += mcmc_ws_bytes(x.n, x.d, x.k);
    }
    return ws;
}

struct ChainPlan {
    std::vector<uint32_t> order;   // d_order: the chunks of class 0, then 1, then 2
    ChainClass cls[3];             // ranges of `order`; [2]: the pile-ups whose work area lives in global memory
    std::vector<uint64_t> ws_off;  // per member of class 2, into the workspace
    uint64_t ws_bytes = 0;
};

// The chain kernel's launches.  Its LDS work area is sized per launch (reads x columns of features + tables), and two
// workgroups share a CU only below 80 KiB each: chunks whose own need stays below that form class 0 (all of a diploid /
// low-copy batch), the others class 1 (several hundred reads, or many columns).  Within a class the longest chains (reads x
// candidate cluster counts) are dispatched first.  A class whose maxima combine beyond its limit hands its largest members
// on: class 0's to class 1, class 1's -- a work area beyond a CU's 160 KiB -- to the global-memory class, where the pile-ups
// beyond JTK_MAX_PILEUP are from the start (the reference takes any depth, mod.rs:86-123: so does class 2, slowly).
// (ChunkMeta.copy_num is what ONE clustering() call sees, at most JTK_MAX_COPY: no chunk is refused here.)
inline void plan_chain(const std::vector<ChunkMeta> &chunks, const size_t limits[2], ChainPlan &cp) {
    auto dims_of = [&](uint32_t c) { return chain_dims_of(chunks[c]); };
    auto need = [&](uint32_t c) {
        const ChainDims x = dims_of(c);
        return mcmc_lds_bytes(x.n, x.d, x.k);
    };
    std::vector<uint32_t> cls[3];
    for (uint32_t c = 0; c < chunks.size(); c++) cls[chunks[c].n_reads > JTK_MAX_PILEUP ? 2 : (need(c) <= limits[0] ? 0 : 1)].push_back(c);
    cp = ChainPlan{};
    for (int q = 0; q < 3; q++) {
        auto &v = cls[q];
        ChainClass &cc = cp.cls[q];
        ChainDims m;
        if (q < 2) {
            m = chain_fit_class(v, cls[q + 1], limits[q], ChainDims{0, 0, 0}, dims_of, [&](uint32_t a, uint32_t b) { return need(a) < need(b); });
            cc.lds_bytes = v.empty() ? 0 : (uint32_t)mcmc_lds_bytes(m.n, m.d, m.k);
            std::stable_sort(v.begin(), v.end(), [&](uint32_t a, uint32_t b) {
                const ChunkMeta &x = chunks[a], &y = chunks[b];
                return (uint64_t)x.n_reads * std::min<uint32_t>(x.copy_num, 4) > (uint64_t)y.n_reads * std::min<uint32_t>(y.copy_num, 4);
            });
        } else {
            m = chain_maxima(v, ChainDims{0, 0, 0}, dims_of);
            cp.ws_bytes = chain_ws_offsets(v, dims_of, cp.ws_off);
        }
        cc.lds_n = m.n;
        cc.lds_d = m.d;
        cc.lds_k = m.k;
        cc.first = (uint32_t)cp.order.size();
        cc.count = (uint32_t)v.size();
        cp.order.insert(cp.order.end(), v.begin(), v.end());
    }
}

// jtk_lc_cluster_features: two launches.  Chunks whose work area fits a CU's LDS run in the table-driven kernels (one launch
// sized for their maxima); the others -- more than JTK_MAX_PILEUP reads, or too large a feature matrix -- in mcmc_kernel_huge
// with a global-memory work area.  `failed[c]`: the chunk did not pass validation; it is listed between the two (it returns at
// once) and sizes nothing.  `max_k`: the clusters both launches are sized for.
struct FeatureChainPlan {
    std::vector<uint32_t> order;   // the LDS launch's chunks, the failed ones, the workspace launch's
    uint32_t n_lds = 0, n_ws = 0;  // launch sizes: order[0 .. n_lds) and order[n_lds .. n_lds + n_ws)
    ChainDims lds, ws;             // what each launch is sized for
    std::vector<uint64_t> ws_off;
    uint64_t ws_bytes = 0;
};
inline void plan_feature_chain(size_t n_chunks, const jtk_lc_feature_chunk_t *chunks, const std::vector<uint8_t> &failed,
                               uint32_t max_k, size_t limit, FeatureChainPlan &fp) {
    auto dims_of = [&](uint32_t c) {
        return ChainDims{std::max<uint32_t>(1, chunks[c].n_reads), std::max<uint32_t>(1, chunks[c].dim), std::max<uint32_t>(2, chunks[c].copy_num)};
    };
    std::vector<uint32_t> in_lds, in_ws;
    for (size_t c = 0; c < n_chunks; c++) {
        if (failed[c]) continue;
        const ChainDims x = dims_of((uint32_t)c);
        (chunks[c].n_reads > JTK_MAX_PILEUP || mcmc_lds_bytes(x.n, x.d, x.k) > limit ? in_ws : in_lds).push_back((uint32_t)c);
    }
    fp = FeatureChainPlan{};
    // the maxima of the launch combine beyond a CU's LDS: its largest member leaves
    fp.lds = chain_fit_class(in_lds, in_ws, limit, ChainDims{1, 1, max_k}, dims_of, [&](uint32_t a, uint32_t b) {
        return (uint64_t)chunks[a].n_reads * std::max<uint32_t>(1, chunks[a].dim) < (uint64_t)chunks[b].n_reads * std::max<uint32_t>(1, chunks[b].dim);
    });
    std::sort(in_ws.begin(), in_ws.end());
    fp.order = in_lds;
    fp.order.insert(fp.order.end(), in_ws.begin(), in_ws.end());
    for (size_t c = 0; c < n_chunks; c++)  // (chunks that failed validation: listed too, they return at once)
        if (failed[c]) fp.order.insert(fp.order.begin() + (ptrdiff_t)in_lds.size(), (uint32_t)c);
    fp.n_ws = (uint32_t)in_ws.size();
    fp.n_lds = (uint32_t)(fp.order.size() - in_ws.size());
    fp.ws = chain_maxima(in_ws, ChainDims{1, 1, max_k}, dims_of);
    fp.ws_bytes = chain_ws_offsets(in_ws, dims_of, fp.ws_off);
}

// ---- the batch

struct BatchPlan {
    std::vector<ChunkMeta> chunks;
    std::vector<ReadMeta> reads;
    std::vector<ChunkState> state0;     // initial state
    std::vector<uint32_t> copy0;        // Chunk.copy_num as given (ChunkMeta.copy_num is what one clustering() call sees)
    std::vector<uint32_t> opslen;       // per read: ops as the caller holds them
    std::vector<uint64_t> homop_off, aux_off, lg_off;  // per chunk
    std::vector<uint32_t> pair_items;   // phmm_pair_kernel: index of a pair's first read; bit 31: a single read
    // elements of each buffer (the units are the buffer's: ReadMeta / ChunkMeta say which)
    uint64_t n_reads = 0, tmpl = 0, ops = 0, ey = 0, delta = 0, raw = 0, row = 0, total = 0, edit = 0, feat = 0, cand = 0, aux = 0, lg = 0;
    uint32_t max_tmpl = 0, max_read = 0, max_n = 0, max_copy = 0;
    uint32_t n_wide_reads = 0, max_wide_radius = 0;  // reads whose band is wider than one wavefront (radius > JTK_MAX_RADIUS)
    bool has_split = false;             // some chunk has copy_num >= UPPER_COPY_NUM
    ChainPlan chain;
};

// Lays the batch out.  `extra`: the chunks are sub-problems of the split branch and inherit radius, coverage and take_num;
// `polish_only`: no variant search and no chain, so no launch classes.  Returns 0, or JTK_ERR_INVALID_ARG with `msg` set.
inline int plan_batch(const jtk_lc_params_t &params, size_t n_chunks, const jtk_lc_chunk_t *chunks, const uint64_t *read_off,
                      const uint64_t *ops_off, const uint8_t *strand, uint32_t post_stride, const ChunkExtra *extra,
                      bool polish_only, BatchPlan &bp, std::string &msg) {
    bp = BatchPlan{};
    for (size_t c = 0; c < n_chunks; c++) bp.n_reads += chunks[c].n_reads;
    bp.chunks.resize(n_chunks);
    bp.reads.resize(bp.n_reads);
    bp.state0.resize(n_chunks);
    bp.copy0.resize(n_chunks);
    bp.opslen.resize(bp.n_reads);
    bp.homop_off.resize(n_chunks);
    bp.aux_off.resize(n_chunks);
    bp.lg_off.resize(n_chunks);
    const uint32_t H = params.gains.max_homopolymer_len;
    uint32_t rcount = 0;
    for (size_t c = 0; c < n_chunks; c++) {
        const jtk_lc_chunk_t &ch = chunks[c];
        const uint32_t tl = (uint32_t)ch.tmpl_len;
        if (ch.read_first != rcount) {
            msg = "chunks must list their reads contiguously in order";
            return JTK_ERR_INVALID_ARG;
        }
        const uint32_t cap = tl + tl / 8 + 64;
        ChunkMeta &cm = bp.chunks[c];
        memset(&cm, 0, sizeof cm);
        cm.chunk_id = ch.chunk_id;
        // one clustering() call: copy_num itself, or BRANCH_NUM = 4 in the split branch (mod.rs:136-142)
        cm.copy_num = ch.copy_num > JTK_MAX_COPY ? 4 : ch.copy_num;
        bp.copy0[c] = ch.copy_num;
        if (ch.copy_num > JTK_MAX_COPY) bp.has_split = true;
        // a posterior row holds up to cluster_num <= copy_num entries (merged sub-clusterings included, mod.rs:161-187)
        // (a sub-problem of the split branch is one clustering() call: its rows hold cm.copy_num entries)
        if ((extra ? cm.copy_num : ch.copy_num) > post_stride && ch.n_reads > 0) {
            msg = "post_stride smaller than a chunk's copy_num";
            return JTK_ERR_INVALID_ARG;
        }
        cm.n_reads = ch.n_reads;
        cm.read_first = rcount;
        cm.tmpl_cap = cap;
        cm.tmpl_off = bp.tmpl;
        cm.total_off = bp.total;
        const uint32_t band_width = (uint32_t)std::ceil((double)tl * params.band_frac);
        cm.radius = extra ? extra[c].radius : band_width / 2;
        cm.edit_cap = cap / 2 + 2;
        cm.edit_off = bp.edit;
        cm.feat_off = bp.feat;
        cm.cand_off = bp.cand;
        // per_cluster_cov (mod.rs:108-111)
        const double pcc = (double)ch.n_reads / (double)ch.copy_num;
        cm.local_coverage = ch.copy_num <= 2 ? pcc : (pcc > params.haploid_coverage ? pcc : params.haploid_coverage);
        if (extra) cm.local_coverage = extra[c].local_coverage;
        if (extra) cm.take_num = extra[c].take_num;
        ChunkState &st = bp.state0[c];
        memset(&st, 0, sizeof st);
        st.tmpl_len = tl;
        st.active = 1;
        st.k = 1;
        if (cm.radius > JTK_WIDE_MAX_RADIUS) {
            st.status = JTK_ERR_UNSUPPORTED;
        } else if (cm.radius > JTK_MAX_RADIUS) {
            bp.n_wide_reads += ch.n_reads;
            if (cm.radius > bp.max_wide_radius) bp.max_wide_radius = cm.radius;
        }
        bp.homop_off[c] = bp.tmpl;
        bp.aux_off[c] = bp.aux;
        bp.lg_off[c] = bp.lg;
        for (uint32_t r = 0; r < ch.n_reads; r++) {
            const uint64_t g = rcount + r;
            const uint64_t rl = read_off[g + 1] - read_off[g], ol = ops_off[g + 1] - ops_off[g];
            ReadMeta &rm = bp.reads[g];
            memset(&rm, 0, sizeof rm);
            rm.chunk = (uint32_t)c;
            rm.read_len = (uint32_t)rl;
            rm.ey_off = bp.ey;
            rm.ops_off = bp.ops;
            rm.ops_cap = ((uint32_t)ol + tl / 8 + 64 + 7u) & ~7u;  // slots stay 8-byte aligned: the walkers fetch 8 ops at a time
            rm.strand = strand[g] ? 1 : 0;
            rm.delta_off = bp.delta;
            rm.table_off = bp.raw;  // finalize_kernel turns the row sums into the table in place: no buffer of its own
            rm.raw_off = bp.raw;
            rm.row_off = bp.row;
            bp.opslen[g] = (uint32_t)ol;
            if (rl > bp.max_read) bp.max_read = (uint32_t)rl;
            bp.ey += rl + 1;
            bp.ops += rm.ops_cap;
            bp.delta += ((uint64_t)(cap + rl) >> 6) + 3;
            bp.raw += (uint64_t)JTK_ACC_N * (cap + 1);
            bp.row += cap + 1;
        }
        if (cap > bp.max_tmpl) bp.max_tmpl = cap;
        if (ch.n_reads > bp.max_n) bp.max_n = ch.n_reads;
        if (cm.copy_num > bp.max_copy) bp.max_copy = cm.copy_num;
        rcount += ch.n_reads;
        bp.tmpl += cap;
        bp.total += (uint64_t)JTK_NUM_ROW * (cap + 1);
        bp.cand += (uint64_t)JTK_NUM_ROW * (cap + 1);
        bp.edit += cm.edit_cap;
        bp.feat += (uint64_t)ch.n_reads * JTK_MAX_DIM;
        bp.aux += (uint64_t)3 * H * (ch.n_reads + 1) + (ch.n_reads + 1) + (JTK_MAX_COPY + 2);
        bp.lg += (uint64_t)ch.n_reads * (JTK_MAX_COPY + 1);
        // narrow bands: two reads of a chunk per wave (phmm_pair.hip)
        if (cm.radius > JTK_PAIR_MAX_RADIUS || st.status != 0) continue;
        const uint32_t voters = cm.take_num ? std::min(cm.take_num, cm.n_reads) : cm.n_reads;
        for (uint32_t r = 0; r + 1 < voters; r += 2) bp.pair_items.push_back(cm.read_first + r);
        if (voters & 1u) bp.pair_items.push_back((cm.read_first + voters - 1) | 0x80000000u);
    }
    if (!polish_only) {
        const size_t limits[2] = {JTK_CU_LDS_BYTES / 2, JTK_CU_LDS_BYTES};
        plan_chain(bp.chunks, limits, bp.chain);
    }
    if (bp.chain.order.empty()) bp.chain.order.push_back(0);
    return 0;
}

// Which variant filter a pass takes.  true: the N x 14(L+1) tables are materialised (finalize_kernel) and column_filter_kernel /
// pick_kernel<true> read them -- where the table itself is the product (window polishing) or a pile-up is too deep for
// column_filter_fused_kernel, which counts in 16-bit fields.  false: the fused filter, straight from the row sums.
#define JTK_FUSED_MAX_READS 65535u
inline bool batch_needs_tables(bool polish_only, uint32_t max_n) { return polish_only || max_n > JTK_FUSED_MAX_READS; }

inline int base_code(uint8_t c) {
    switch (c) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': return 3;
        default: return -1;
    }
}

// The templates (a few MB) recoded to 2 bits per byte at their planned offsets; false: a base that is none of ACGT.
inline bool recode_templates(const BatchPlan &bp, const jtk_lc_chunk_t *chunks, const uint8_t *tmpl_bases, std::vector<uint8_t> &tmpl) {
    tmpl.assign(bp.tmpl, 0);
    bool ok = true;
    for (size_t c = 0; c < bp.chunks.size(); c++) {
        const jtk_lc_chunk_t &ch = chunks[c];
        for (uint64_t p = 0; p < ch.tmpl_len; p++) {
            const int code = base_code(tmpl_bases[ch.tmpl_off + p]);
            if (code < 0) ok = false;
            tmpl[bp.chunks[c].tmpl_off + p] = (uint8_t)(code & 3);
        }
    }
    return ok;
}

// ---- the waves of the pair-HMM sweeps

struct SweepSizes {  // of the batch's maxima, as the kernels' own files compute them; the pair / wide ones 0 where not needed
    size_t phmm_lds_bytes, phmm_pair_lds_bytes, phmm_wide_lds_bytes;
    uint64_t phmm_wide_scratch_doubles;
};

struct WavePlan {
    uint32_t n_waves = 0;        // phmm_kernel
    uint64_t stripe_stride = 0;  // doubles of forward scratch per stripe
    uint32_t n_stripes = 0;      // what the device's shared set holds
    uint32_t n_pair_waves = 0;   // phmm_pair_kernel
    uint32_t n_wide_waves = 0;   // phmm_wide_kernel
    uint64_t wide_stride = 0;    // doubles of its scratch per wave
};

// Returns 0, or JTK_ERR_UNSUPPORTED with `msg` set when a kernel's LDS staging of the longest template + read exceeds a CU's.
inline int plan_waves(uint32_t n_cu, const SweepSizes &sizes, const BatchPlan &bp, WavePlan &wp, std::string &msg) {
    wp = WavePlan{};
    // resident waves per CU: 3 per SIMD by registers (JTK_PHMM_WAVES), and what 160 KiB of LDS hold
    uint32_t per_cu = (uint32_t)(JTK_CU_LDS_BYTES / sizes.phmm_lds_bytes);
    if (per_cu > 12) per_cu = 12;
    if (per_cu < 1) per_cu = 1;
    const uint32_t want = n_cu * per_cu;
    wp.n_waves = bp.n_reads < want ? (uint32_t)bp.n_reads : want;
    if (wp.n_waves == 0) wp.n_waves = 1;
    // one stripe per wave the DEVICE can hold (3 per SIMD by registers = 12 per CU; 16 leaves room): the set is shared
    wp.stripe_stride = (uint64_t)(bp.max_tmpl + bp.max_read + 8 + JTK_SCRATCH_GUARD) * 64 * 2;
    wp.n_stripes = n_cu * 16;
    if (!bp.pair_items.empty()) {
        const size_t pl = sizes.phmm_pair_lds_bytes;
        if (pl > JTK_CU_LDS_BYTES) {
            msg = "template + reads too long for the LDS staging of phmm_pair_kernel";
            return JTK_ERR_UNSUPPORTED;
        }
        per_cu = (uint32_t)(JTK_CU_LDS_BYTES / pl);
        if (per_cu > 8) per_cu = 8;  // two waves per SIMD by registers
        wp.n_pair_waves = std::min<uint32_t>(std::min<uint32_t>((uint32_t)bp.pair_items.size(), n_cu * per_cu),
                                             wp.n_waves);  // shares phmm_kernel's scratch stripes (launched after it)
    }
    if (bp.n_wide_reads) {
        const size_t wl = sizes.phmm_wide_lds_bytes;
        if (wl > JTK_CU_LDS_BYTES) {
            msg = "template + read too long for the LDS staging of phmm_wide_kernel";
            return JTK_ERR_UNSUPPORTED;
        }
        per_cu = (uint32_t)(JTK_CU_LDS_BYTES / wl);
        if (per_cu > 4) per_cu = 4;
        wp.wide_stride = sizes.phmm_wide_scratch_doubles;
        uint64_t wide_want = (uint64_t)n_cu * per_cu;
        const uint64_t budget = (48ull << 30) / (wp.wide_stride * 8);  // at most 48 GB of forward tables in flight
        if (wide_want > budget) wide_want = budget ? budget : 1;
        wp.n_wide_waves = (uint32_t)std::min<uint64_t>(bp.n_wide_reads, wide_want);
    }
    if (sizes.phmm_lds_bytes > JTK_CU_LDS_BYTES) {
        msg = "template + read too long for the LDS staging of phmm_kernel";
        return JTK_ERR_UNSUPPORTED;
    }
    return 0;
}
