// session.hip -- the resident-batch session: its pools, the session object and the C-ABI entry points of include/jtk_lc.h that
// create, run, fetch, trace and destroy one.
//
// One process drives one GPU.  A session validates and encodes the flat host batch, uploads it once, allocates
// every workspace up front (sized for 288 GB of HBM: the full N x 14(L+1) tables of all chunks stay
// resident), and then runs the stage as a short sequence of kernel launches on its own stream:
//
//   band_prep -> [ phmm -> finalize -> polish_round ]* until no chunk is active -> filter -> mcmc
//
// (mod.rs:86-123 per chunk).  The last polishing pass that finds no edit has produced exactly the
// modification table `clustering` would recompute (same consensus, same ops, same radius: mod.rs:105 vs
// :112, pseudo_mcmc.rs:117), so it is reused instead of recomputed.
//
// The other entry points are built on the session (session_internal.h): the split branch of chunks with copy_num >= 8
// (session_split.hip), the one-shot stage calls and window polishing (session_stages.hip), the model refit and the
// modification table (session_refit.hip), the features-only chain (session_features.hip).
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>

#include "session_internal.h"

thread_local std::string g_last_error;
thread_local jtk_lc_timing_t g_timing;

int jtk_fail(int status, const std::string &msg) {
    g_last_error = msg;
    return status;
}

int jtk_require_device(int device) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) return jtk_fail(JTK_ERR_NO_DEVICE, "no HIP device visible (jtk_lc has no CPU fallback)");
    if (device < 0 || device >= count) return jtk_fail(JTK_ERR_NO_DEVICE, "device ordinal out of range");
    JTK_HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    JTK_HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return jtk_fail(JTK_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
    return 0;
}

namespace {

inline int base_code(uint8_t c) {
    switch (c) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': return 3;
        default: return -1;
    }
}

HmmDev to_dev(const jtk_hmm_t &h) {
    HmmDev d;
    const double a[9] = {h.mat_mat, h.mat_ins, h.mat_del, h.ins_mat, h.ins_ins, h.ins_del, h.del_mat, h.del_ins, h.del_del};
    memcpy(d.a, a, sizeof a);
    memcpy(d.eM, h.mat_emit, sizeof d.eM);
    memcpy(d.eI, h.ins_emit, sizeof d.eI);
    return d;
}

// The pools below -- g_pool, g_stripes and the pinned-page free list -- stay in THIS translation unit, g_pool first.
// DevPtr::~DevPtr gives its block to g_pool, and g_stripes[] holds DevPtrs that are destroyed at process exit: within one
// translation unit objects go in reverse order of definition, so the pool outlives them.  Across translation units the order is
// unspecified, and a give() into a destroyed mutex / multimap at exit would be a fault.
//
// Device blocks of destroyed sessions are kept for the next session on the same device: a stage call is one-shot
// (create, run, fetch, destroy) and is entered several times per pipeline with batches of similar shape, and mapping
// the ~88 GB of workspaces of 2500 chunks costs ~0.2 s on a fresh device and ~2.4 s once the same memory has been
// freed before (the driver scrubs it) -- more than the kernels take.  Nothing relies on the contents of a fresh
// block.  jtk_lc_trim_cache() returns everything to the driver.
struct BlockPool {
    // Small blocks are kept too (round 6): a session holds ~40 of them (metadata, counters, offsets), hipFree of each one
    // synchronises EVERY stream of the device, and the model refit creates ten sessions in a row.  Below 1 MiB a request is
    // rounded up to a power of two (dev_alloc), so the few size classes match exactly.
    static const size_t MIN_BYTES = 256;
    static const size_t SMALL_BYTES = 1u << 20;
    // per device: JTK_LC_POOL_GB (default 32: the pool must not starve torch / RCCL / another library in the same process;
    // blocks beyond the cap go straight back to the driver), 0 disables pooling
    static size_t max_cached() {
        static const size_t v = []() -> size_t {
            const char *e = getenv("JTK_LC_POOL_GB");
            const double gb = e ? atof(e) : 32.0;
            return gb > 0.0 ? (size_t)(gb * 1073741824.0) : 0;
        }();
        return v;
    }
    std::mutex m;
    std::multimap<size_t, void *> blocks[JTK_POOL_DEVICES];
    size_t cached[JTK_POOL_DEVICES] = {};
    void *take(int dev, size_t bytes, size_t *cap) {
        std::lock_guard<std::mutex> lock(m);
        auto &b = blocks[dev];
        auto it = b.lower_bound(bytes);
        if (it == b.end() || it->first > bytes + bytes / 4 + (bytes < SMALL_BYTES ? 0 : SMALL_BYTES)) return nullptr;
        void *p = it->second;
        *cap = it->first;
        cached[dev] -= it->first;
        b.erase(it);
        return p;
    }
    bool give(int dev, void *p, size_t cap) {
        std::lock_guard<std::mutex> lock(m);
        if (cap < MIN_BYTES || cached[dev] + cap > max_cached()) return false;
        blocks[dev].emplace(cap, p);
        cached[dev] += cap;
        return true;
    }
    void trim(int dev) {
        std::lock_guard<std::mutex> lock(m);
        for (auto &kv : blocks[dev]) (void)hipFree(kv.second);
        blocks[dev].clear();
        cached[dev] = 0;
    }
};
BlockPool g_pool;

// A batch in flight uses up to four slices x two streams (the chain's general kernel runs beside its light one).  ROCm maps
// streams onto GPU_MAX_HW_QUEUES hardware queues (4 by default) and streams that share a queue run in order: a slice's 300 ms
// chain kernel would then hold up another slice's pair-HMM launches.  Eight streams need eight queues, and the host's own
// streams (the null stream as soon as anything uses it) take theirs: 12.  The variable is read when the HIP runtime
// initialises, so it is set -- unless the host has set it -- when this library is loaded; a host that has initialised HIP
// earlier sets it itself.
static bool g_queues_by_library = false;  // the variable was absent when the library was loaded
static int g_host_queues = 0;             // the host's own setting, if any
__attribute__((constructor)) void jtk_lc_default_hw_queues() {
    const char *q = getenv("GPU_MAX_HW_QUEUES");
    if (q) {
        g_host_queues = atoi(q);
    } else {
        g_queues_by_library = true;
        setenv("GPU_MAX_HW_QUEUES", "12", 0);
    }
}

std::mutex g_stripe_mutex;
std::shared_ptr<StripePool> g_stripes[JTK_POOL_DEVICES];

}  // namespace

DevPtr::~DevPtr() {
    if (!p) return;
    if (dev < 0 || dev >= JTK_POOL_DEVICES || !g_pool.give(dev, p, cap)) (void)hipFree(p);
}

// The mapped pinned pages the polish rounds report into (JTK_NACTIVE_SLOTS counters per session): taken from and returned to
// a process-wide free list -- sessions are created per slice per one-shot call, and hipHostFree synchronises the device,
// which stalls the other slices' streams.  The pages are freed with the process.
static std::mutex g_pinned_mutex;
static std::vector<uint32_t *> g_pinned_free;
static uint32_t *pinned_page_take() {
    {
        std::lock_guard<std::mutex> lock(g_pinned_mutex);
        if (!g_pinned_free.empty()) {
            uint32_t *p = g_pinned_free.back();
            g_pinned_free.pop_back();
            return p;
        }
    }
    uint32_t *p = nullptr;
    if (hipHostMalloc(reinterpret_cast<void **>(&p), JTK_NACTIVE_SLOTS * sizeof(uint32_t), hipHostMallocMapped | hipHostMallocPortable) != hipSuccess)
        return nullptr;
    return p;
}
static void pinned_page_give(uint32_t *p) {
    std::lock_guard<std::mutex> lock(g_pinned_mutex);
    g_pinned_free.push_back(p);
}

jtk_lc_session::~jtk_lc_session() {
    if (stream) (void)hipStreamSynchronize(stream);  // blocks go back to the pool, not through hipFree's implicit sync
    if (side) {
        (void)hipStreamSynchronize(side);
        (void)hipStreamDestroy(side);
    }
    for (auto &e : ev_chain)
        if (e) (void)hipEventDestroy(e);
    for (auto &t : timers) {
        if (t.a) (void)hipEventDestroy(t.a);
        if (t.b) (void)hipEventDestroy(t.b);
    }
    if (stream) (void)hipStreamDestroy(stream);
    if (h_nactive) pinned_page_give(h_nactive);  // (hipHostFree synchronises the whole device: never on the one-shot path)
    for (auto &e : ev_round)
        if (e) (void)hipEventDestroy(e);
}

int dev_alloc_bytes(DevPtr &d, size_t bytes) {
    if (bytes < BlockPool::SMALL_BYTES) {   // size classes for the small blocks (see BlockPool)
        size_t cls = BlockPool::MIN_BYTES;
        while (cls < bytes) cls <<= 1;
        bytes = cls;
    }
    int dev = 0;
    JTK_HIP_TRY(hipGetDevice(&dev));
    if (dev >= 0 && dev < JTK_POOL_DEVICES && bytes >= BlockPool::MIN_BYTES) {
        d.p = g_pool.take(dev, bytes, &d.cap);
        if (d.p) {
            d.dev = dev;
            return 0;
        }
    }
    hipError_t e = hipMalloc(&d.p, bytes);
    if (e == hipErrorOutOfMemory && dev >= 0 && dev < JTK_POOL_DEVICES) {  // cached blocks of another shape are in the way
        (void)hipGetLastError();
        g_pool.trim(dev);
        e = hipMalloc(&d.p, bytes);
    }
    JTK_HIP_TRY(e);
    d.cap = bytes;
    d.dev = dev;
    return 0;
}

void tstart(jtk_lc_session *s, int kind) {
    KernelTimer t;
    t.kind = kind;
    (void)hipEventCreate(&t.a);
    (void)hipEventCreate(&t.b);
    (void)hipEventRecord(t.a, s->stream);
    s->timers.push_back(t);
}
void tstop(jtk_lc_session *s) { (void)hipEventRecord(s->timers.back().b, s->stream); }

// ---- the session and its C-ABI entry points.  (The entry points take their C linkage from their declarations in jtk_lc.h.)

int session_create_ex(const jtk_lc_params_t *params, size_t n_chunks, const jtk_lc_chunk_t *chunks,
                      const uint8_t *tmpl_bases, const uint8_t *read_bases, const uint64_t *read_off,
                      const uint8_t *ops, const uint64_t *ops_off, const uint8_t *strand,
                      uint32_t post_stride, int device, const ChunkExtra *extra, uint32_t ignore_edge,
                      jtk_lc_session_t **out, bool polish_only) {
    g_last_error.clear();
    if (!params || !out || (n_chunks && (!chunks || !tmpl_bases || !read_bases || !read_off || !ops || !ops_off || !strand)))
        return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (post_stride == 0) return jtk_fail(JTK_ERR_INVALID_ARG, "post_stride must be >= 1");
    if (params->gains.max_homopolymer_len == 0 || params->gains.max_homopolymer_len > JTK_GAINS_MAX_HOMOP)
        return jtk_fail(JTK_ERR_INVALID_ARG, "gains.max_homopolymer_len out of range");
    int rc = jtk_require_device(device);
    if (rc) return rc;
    jtk_lc_session *s = new jtk_lc_session();
    std::unique_ptr<jtk_lc_session> guard(s);
    s->device = device;
    s->params = *params;
    s->post_stride = post_stride;
    s->n_chunks = (uint32_t)n_chunks;
    s->ignore_edge = ignore_edge;
    s->polish_only = polish_only;  // no variant search, no chain: none of their limits or workspaces apply
    s->h_copy0.resize(n_chunks);
    JTK_HIP_TRY(hipStreamCreate(&s->stream));

    // ---- host-side layout + validation + encoding
    uint64_t n_reads = 0;
    for (size_t c = 0; c < n_chunks; c++) n_reads += chunks[c].n_reads;
    s->n_reads = (uint32_t)n_reads;
    s->h_chunks.resize(n_chunks);
    s->h_reads.resize(n_reads);
    s->h_state0.resize(n_chunks);
    std::vector<uint8_t> h_tmpl;
    std::vector<uint32_t> h_opslen(n_reads);
    std::vector<uint64_t> h_homop_off(n_chunks), h_aux_off(n_chunks), h_lg_off(n_chunks);
    uint64_t tmpl_off = 0, ops_cap_off = 0, ey_off = 0, delta_off = 0, table_off = 0, raw_off = 0, row_off = 0,
             total_off = 0, edit_off = 0, feat_off = 0, cand_off = 0, aux_off = 0, lg_off = 0;
    const uint32_t H = params->gains.max_homopolymer_len;
    uint32_t rcount = 0;
    for (size_t c = 0; c < n_chunks; c++) {
        const jtk_lc_chunk_t &ch = chunks[c];
        const uint32_t tl = (uint32_t)ch.tmpl_len;
        if (ch.read_first != rcount) return jtk_fail(JTK_ERR_INVALID_ARG, "chunks must list their reads contiguously in order");
        const uint32_t cap = tl + tl / 8 + 64;
        ChunkMeta &cm = s->h_chunks[c];
        memset(&cm, 0, sizeof cm);
        cm.chunk_id = ch.chunk_id;
        // one clustering() call: copy_num itself, or BRANCH_NUM = 4 in the split branch (mod.rs:136-142)
        cm.copy_num = ch.copy_num > JTK_MAX_COPY ? 4 : ch.copy_num;
        s->h_copy0[c] = ch.copy_num;
        if (ch.copy_num > JTK_MAX_COPY) s->has_split = true;
        // a posterior row holds up to cluster_num <= copy_num entries (merged sub-clusterings included, mod.rs:161-187)
        // (a sub-problem of the split branch is one clustering() call: its rows hold cm.copy_num entries)
        if ((extra ? cm.copy_num : ch.copy_num) > post_stride && ch.n_reads > 0)
            return jtk_fail(JTK_ERR_INVALID_ARG, "post_stride smaller than a chunk's copy_num");
        cm.n_reads = ch.n_reads;
        cm.read_first = rcount;
        cm.tmpl_cap = cap;
        cm.tmpl_off = tmpl_off;
        cm.total_off = total_off;
        const uint32_t band_width = (uint32_t)std::ceil((double)tl * params->band_frac);
        cm.radius = extra ? extra[c].radius : band_width / 2;
        cm.edit_cap = cap / 2 + 2;
        cm.edit_off = edit_off;
        cm.feat_off = feat_off;
        cm.cand_off = cand_off;
        // per_cluster_cov (mod.rs:108-111)
        const double pcc = (double)ch.n_reads / (double)ch.copy_num;
        cm.local_coverage = ch.copy_num <= 2 ? pcc : (pcc > params->haploid_coverage ? pcc : params->haploid_coverage);
        if (extra) cm.local_coverage = extra[c].local_coverage;
        if (extra) cm.take_num = extra[c].take_num;
        ChunkState &st = s->h_state0[c];
        memset(&st, 0, sizeof st);
        st.tmpl_len = tl;
        st.active = 1;
        st.k = 1;
        if (cm.radius > JTK_WIDE_MAX_RADIUS) {
            st.status = JTK_ERR_UNSUPPORTED;
        } else if (cm.radius > JTK_MAX_RADIUS) {
            s->n_wide_reads += ch.n_reads;
            if (cm.radius > s->max_wide_radius) s->max_wide_radius = cm.radius;
        }
        h_homop_off[c] = tmpl_off;
        h_aux_off[c] = aux_off;
        h_lg_off[c] = lg_off;
        for (uint32_t r = 0; r < ch.n_reads; r++) {
            const uint64_t g = rcount + r;
            const uint64_t rl = read_off[g + 1] - read_off[g], ol = ops_off[g + 1] - ops_off[g];
            ReadMeta &rm = s->h_reads[g];
            memset(&rm, 0, sizeof rm);
            rm.chunk = (uint32_t)c;
            rm.read_len = (uint32_t)rl;
            rm.ey_off = ey_off;
            rm.ops_off = ops_cap_off;
            rm.ops_cap = ((uint32_t)ol + tl / 8 + 64 + 7u) & ~7u;  // slots stay 8-byte aligned: the walkers fetch 8 ops at a time
            rm.strand = strand[g] ? 1 : 0;
            rm.delta_off = delta_off;
            rm.table_off = raw_off;  // finalize_kernel turns the row sums into the table in place
            rm.raw_off = raw_off;
            rm.row_off = row_off;
            h_opslen[g] = (uint32_t)ol;
            if (rl > s->max_read) s->max_read = (uint32_t)rl;
            ey_off += rl + 1;
            ops_cap_off += rm.ops_cap;
            delta_off += ((uint64_t)(cap + rl) >> 6) + 3;
            table_off += (uint64_t)JTK_NUM_ROW * (cap + 1);
            raw_off += (uint64_t)JTK_ACC_N * (cap + 1);
            row_off += cap + 1;
        }
        if (cap > s->max_tmpl) s->max_tmpl = cap;
        if (ch.n_reads > s->max_n) s->max_n = ch.n_reads;
        if (cm.copy_num > s->max_copy) s->max_copy = cm.copy_num;
        rcount += ch.n_reads;
        tmpl_off += cap;
        total_off += (uint64_t)JTK_NUM_ROW * (cap + 1);
        cand_off += (uint64_t)JTK_NUM_ROW * (cap + 1);
        edit_off += cm.edit_cap;
        feat_off += (uint64_t)ch.n_reads * JTK_MAX_DIM;
        aux_off += (uint64_t)3 * H * (ch.n_reads + 1) + (ch.n_reads + 1) + (JTK_MAX_COPY + 2);
        lg_off += (uint64_t)ch.n_reads * (JTK_MAX_COPY + 1);
    }
    // ---- per-base encoding.  Templates (a few MB) are recoded here; the reads and their ops -- the bulk of a stage call's input --
    //      cross the bus as the caller holds them and are validated and recoded by encode_reads_kernel (io_kernels.hip), below.
    h_tmpl.assign(tmpl_off, 0);
    {
        int bad = 0;
        for (size_t c = 0; c < n_chunks; c++) {
            const jtk_lc_chunk_t &ch = chunks[c];
            const ChunkMeta &cm = s->h_chunks[c];
            for (uint64_t p = 0; p < ch.tmpl_len; p++) {
                const int code = base_code(tmpl_bases[ch.tmpl_off + p]);
                if (code < 0) bad = 1;
                h_tmpl[cm.tmpl_off + p] = (uint8_t)(code & 3);
            }
        }
        if (bad == 1) return jtk_fail(JTK_ERR_INVALID_ARG, "non-ACGT base in a template");
    }
    s->tmpl_bytes = h_tmpl.size();
    s->ops_bytes = ops_cap_off;
    if (s->has_split) {  // the sub-problems of the split branch are encoded from these again
        s->h_read_bases.assign(read_bases, read_bases + read_off[n_reads]);
        s->h_read_off.assign(read_off, read_off + n_reads + 1);
        s->h_strand.assign(strand, strand + n_reads);
    }

    // ---- device allocation + upload
    tstart(s, -1);
    std::vector<jtk_lc_params_t> pv(1, *params);
    std::vector<HmmDev> hv = {to_dev(params->forward), to_dev(params->reverse)};
    if ((rc = dev_upload(s, s->d_params, pv))) return rc;
    if ((rc = dev_upload(s, s->d_hmm2, hv))) return rc;
    if ((rc = dev_upload(s, s->d_chunks, s->h_chunks))) return rc;
    {  // The chain kernel's launches.  Its LDS work area is sized per launch (reads x columns of features + tables), and
       // two workgroups share a CU only below 80 KiB each: chunks whose own need stays below that form class 0 (all of a
       // diploid / low-copy batch), the others class 1 (several hundred reads, or many columns).  Within a class the
       // longest chains (reads x candidate cluster counts) are dispatched first.  A class-1 combination that does not fit
       // a CU's 160 KiB loses its largest members (reported as JTK_ERR_UNSUPPORTED, like a pile-up beyond JTK_MAX_PILEUP).
        auto dims_of = [&](const ChunkMeta &cm, uint32_t *n, uint32_t *d, uint32_t *k) {
            *n = cm.n_reads;
            *k = std::min<uint32_t>(std::max<uint32_t>(cm.copy_num, 2u), JTK_MAX_COPY);
            // a chunk picks at most ROUND * max(copy_num, 2) columns (pseudo_mcmc.rs:421,527,532)
            *d = std::min<uint32_t>(JTK_MAX_DIM, 3u * std::max<uint32_t>(cm.copy_num, 2u));
        };
        std::vector<uint32_t> cls[3];
        for (uint32_t c = 0; c < s->h_chunks.size() && !polish_only; c++) {
            uint32_t n, d, k;
            dims_of(s->h_chunks[c], &n, &d, &k);
            if (s->h_chunks[c].copy_num > JTK_MAX_COPY) {
                if (s->h_state0[c].status == 0) s->h_state0[c].status = JTK_ERR_UNSUPPORTED;
                continue;
            }
            if (n > JTK_MAX_PILEUP) {  // the reference takes any depth (mod.rs:86-123): so does class 2, slowly
                cls[2].push_back(c);
                continue;
            }
            cls[mcmc_lds_bytes(n, d, k) <= 80 * 1024 ? 0 : 1].push_back(c);
        }
        std::vector<uint32_t> order;
        for (int q = 0; q < 2; q++) {
            auto &v = cls[q];
            auto need = [&](uint32_t c) {
                uint32_t n, d, k;
                dims_of(s->h_chunks[c], &n, &d, &k);
                return mcmc_lds_bytes(n, d, k);
            };
            ChainClass &cc = s->chain_class[q];
            for (;;) {
                cc = ChainClass{};
                for (uint32_t c : v) {
                    uint32_t n, d, k;
                    dims_of(s->h_chunks[c], &n, &d, &k);
                    cc.lds_n = std::max(cc.lds_n, n);
                    cc.lds_d = std::max(cc.lds_d, d);
                    cc.lds_k = std::max(cc.lds_k, k);
                }
                // class 0 is launched with its members' maxima of (reads, columns, clusters): THAT combination has to stay
                // below 80 KiB for two workgroups to share a CU, not just every member's own need
                cc.lds_bytes = v.empty() ? 0 : (uint32_t)mcmc_lds_bytes(cc.lds_n, cc.lds_d, cc.lds_k);
                if (v.empty() || cc.lds_bytes <= (q == 0 ? 80u : 160u) * 1024u) break;
                auto worst = std::max_element(v.begin(), v.end(), [&](uint32_t a, uint32_t b) { return need(a) < need(b); });
                cls[q + 1].push_back(*worst);  // a class's maxima can combine beyond one member's need: hand it over (class 1's
                                               // overflow -- a work area beyond 160 KiB -- goes to the global-memory class)
                v.erase(worst);
            }
            std::stable_sort(v.begin(), v.end(), [&](uint32_t a, uint32_t b) {
                const ChunkMeta &x = s->h_chunks[a], &y = s->h_chunks[b];
                return (uint64_t)x.n_reads * std::min<uint32_t>(x.copy_num, 4) > (uint64_t)y.n_reads * std::min<uint32_t>(y.copy_num, 4);
            });
            cc.first = (uint32_t)order.size();
            cc.count = (uint32_t)v.size();
            order.insert(order.end(), v.begin(), v.end());
        }
        {   // class 2: one workgroup per chunk, its own slice of a global workspace
            ChainClass &cc = s->chain_class[2];
            cc = ChainClass{};
            std::vector<uint64_t> ws_off;
            uint64_t ws = 0;
            for (uint32_t c : cls[2]) {
                uint32_t n, d, k;
                dims_of(s->h_chunks[c], &n, &d, &k);
                cc.lds_n = std::max(cc.lds_n, n);
                cc.lds_d = std::max(cc.lds_d, d);
                cc.lds_k = std::max(cc.lds_k, k);
                ws_off.push_back(ws);
                ws += mcmc_ws_bytes(n, d, k);
            }
            cc.first = (uint32_t)order.size();
            cc.count = (uint32_t)cls[2].size();
            order.insert(order.end(), cls[2].begin(), cls[2].end());
            if (cc.count) {
                if ((rc = dev_alloc<uint8_t>(s->d_chain_ws, ws))) return rc;
                if ((rc = dev_upload(s, s->d_chain_ws_off, ws_off))) return rc;
            }
        }
        if (order.empty()) order.push_back(0);
        if ((rc = dev_upload(s, s->d_order, order))) return rc;
    }
    if ((rc = dev_upload(s, s->d_reads, s->h_reads))) return rc;
    if ((rc = dev_alloc<ChunkState>(s->d_state, n_chunks))) return rc;
    if ((rc = dev_upload(s, s->d_tmpl_init, h_tmpl))) return rc;
    if ((rc = dev_alloc<uint8_t>(s->d_ops_init, ops_cap_off))) return rc;
    if ((rc = dev_upload(s, s->d_opslen_init, h_opslen))) return rc;
    // (+8: the polish kernels fetch templates / reads in aligned 8-byte blocks)
    if ((rc = dev_alloc<uint8_t>(s->d_tmpl0, h_tmpl.size() + 8))) return rc;
    if ((rc = dev_alloc<uint8_t>(s->d_tmpl1, h_tmpl.size() + 8))) return rc;
    if ((rc = dev_alloc<uint8_t>(s->d_ops0, ops_cap_off))) return rc;
    if ((rc = dev_alloc<uint8_t>(s->d_ops1, ops_cap_off))) return rc;
    if ((rc = dev_alloc<uint32_t>(s->d_opslen0, n_reads))) return rc;
    if ((rc = dev_alloc<uint32_t>(s->d_opslen1, n_reads))) return rc;
    if ((rc = dev_alloc<uint8_t>(s->d_ey, ey_off + 8))) return rc;
    JTK_HIP_TRY(hipMemsetAsync(s->d_ey.as<uint8_t>() + ey_off, 0, 8, s->stream));   // (the polish kernels fetch aligned 8-byte blocks)
    if ((rc = dev_alloc<uint64_t>(s->d_delta, delta_off))) return rc;
    if ((rc = dev_alloc<double>(s->d_raw, raw_off))) return rc;
    if (n_reads) {
        // The reads and their ops, as the caller holds them (ASCII bases, one op per byte, back to back), straight from the
        // caller's memory into the workspace the row sums will occupy later (296 KB per read against ~4 KB of input), then
        // validated and recoded on the device: no recoded copy on the host, no first-touch of fresh host vectors.
        const uint64_t rb0 = read_off[0], rb_bytes = read_off[n_reads] - rb0, ob0 = ops_off[0], ob_bytes = ops_off[n_reads] - ob0;
        const uint64_t o_bases = 0, o_ops = (rb_bytes + 15) & ~15ull, o_boff = o_ops + ((ob_bytes + 15) & ~15ull),
                       o_ooff = o_boff + (n_reads + 1) * 8, o_flag = o_ooff + (n_reads + 1) * 8, need = o_flag + 16;
        DevPtr tmp;   // (only when the row sums' block is too small for it: pile-ups of very short templates)
        uint8_t *stage = s->d_raw.as<uint8_t>();
        if (need > raw_off * 8) {
            if ((rc = dev_alloc<uint8_t>(tmp, need))) return rc;
            stage = tmp.as<uint8_t>();
        }
        JTK_HIP_TRY(hipMemsetAsync(stage + o_flag, 0, 16, s->stream));
        if (rb_bytes) JTK_HIP_TRY(hipMemcpyAsync(stage + o_bases, read_bases + rb0, rb_bytes, hipMemcpyHostToDevice, s->stream));
        if (ob_bytes) JTK_HIP_TRY(hipMemcpyAsync(stage + o_ops, ops + ob0, ob_bytes, hipMemcpyHostToDevice, s->stream));
        JTK_HIP_TRY(hipMemcpyAsync(stage + o_boff, read_off, (n_reads + 1) * 8, hipMemcpyHostToDevice, s->stream));
        JTK_HIP_TRY(hipMemcpyAsync(stage + o_ooff, ops_off, (n_reads + 1) * 8, hipMemcpyHostToDevice, s->stream));
        launch_encode_reads(s->stream, (uint32_t)n_reads, s->d_reads.as<ReadMeta>(), stage + o_bases,
                            reinterpret_cast<const uint64_t *>(stage + o_boff), stage + o_ops,
                            reinterpret_cast<const uint64_t *>(stage + o_ooff), s->d_ey.as<uint8_t>(), s->d_ops_init.as<uint8_t>(),
                            reinterpret_cast<uint32_t *>(stage + o_flag));
        uint32_t flags = 0;
        JTK_HIP_TRY(hipMemcpyAsync(&flags, stage + o_flag, 4, hipMemcpyDeviceToHost, s->stream));
        JTK_HIP_TRY(hipStreamSynchronize(s->stream));   // (also: `tmp` may go back to the pool)
        JTK_HIP_TRY(hipGetLastError());
        if (flags & 2u) return jtk_fail(JTK_ERR_INVALID_ARG, "non-ACGT base in a read");
        if (flags & 4u) return jtk_fail(JTK_ERR_INVALID_ARG, "bad op code");
    }
    if ((rc = dev_alloc<int>(s->d_rawG, row_off))) return rc;
    if ((rc = dev_alloc<double>(s->d_lk, n_reads))) return rc;
    (void)table_off;  // no buffer of its own: the tables live where the row sums were (d_raw)
    if ((rc = dev_alloc<double>(s->d_total, total_off))) return rc;
    if ((rc = dev_alloc<Edit>(s->d_edits, edit_off))) return rc;
    if ((rc = dev_alloc<uint32_t>(s->d_newlen, n_chunks))) return rc;
    if ((rc = dev_alloc<uint32_t>(s->d_counter, 4))) return rc;
    JTK_HIP_TRY(hipMemsetAsync(s->d_counter.p, 0, 4 * sizeof(uint32_t), s->stream));  // once: the ticket counters are never reset
    if ((rc = dev_alloc<uint32_t>(s->d_nactive, JTK_NACTIVE_SLOTS))) return rc;
    if ((rc = dev_alloc<uint32_t>(s->d_chain_split, 2 * n_chunks + 8))) return rc;
    if (!polish_only) {  // the second stream (the chain's general kernel beside its light one) only where the hardware queues
                         // are there for it: the host asked for >= 8 queues, or the variable was absent when this library was
                         // loaded and jtk_lc_default_hw_queues set it (a host that initialised HIP BEFORE loading the library
                         // and never set the variable runs on 4 queues: it says so with JTK_LC_SIDE_STREAM=0)
        const char *force = getenv("JTK_LC_SIDE_STREAM");
        const bool on = force ? atoi(force) != 0 : (g_queues_by_library || g_host_queues >= 8);
        if (on) {
            JTK_HIP_TRY(hipStreamCreateWithFlags(&s->side, hipStreamNonBlocking));
            JTK_HIP_TRY(hipEventCreateWithFlags(&s->ev_chain[0], hipEventDisableTiming));
            JTK_HIP_TRY(hipEventCreateWithFlags(&s->ev_chain[1], hipEventDisableTiming));
        }
    }
    if (!polish_only) {  // the filter's and the chain's workspaces
    if ((rc = dev_alloc<uint16_t>(s->d_homop, tmpl_off))) return rc;
    if ((rc = dev_upload(s, s->d_homop_off, h_homop_off))) return rc;
    if ((rc = dev_alloc<double>(s->d_aux, aux_off))) return rc;
    if ((rc = dev_upload(s, s->d_aux_off, h_aux_off))) return rc;
    if ((rc = dev_alloc<double>(s->d_cand, cand_off))) return rc;
    if ((rc = dev_alloc<uint32_t>(s->d_list, cand_off))) return rc;
    if ((rc = dev_alloc<uint8_t>(s->d_sel, cand_off))) return rc;
    if ((rc = dev_alloc<double>(s->d_feat, feat_off))) return rc;
    if ((rc = dev_alloc<uint32_t>(s->d_vtype, (uint64_t)2 * n_chunks * JTK_MAX_DIM))) return rc;
    if ((rc = dev_alloc<uint32_t>(s->d_pos, (uint64_t)n_chunks * JTK_MAX_DIM))) return rc;
    if ((rc = dev_alloc<uint32_t>(s->d_label, n_reads))) return rc;
    if ((rc = dev_alloc<double>(s->d_post, (uint64_t)n_reads * post_stride))) return rc;
    if ((rc = dev_alloc<double>(s->d_lg, lg_off))) return rc;
    if ((rc = dev_upload(s, s->d_lg_off, h_lg_off))) return rc;
    }
    if (extra) {
        std::vector<uint64_t> h_rng(4 * n_chunks);
        for (size_t c = 0; c < n_chunks; c++) memcpy(&h_rng[4 * c], extra[c].rng, 32);
        if ((rc = dev_upload(s, s->d_rng, h_rng))) return rc;
        s->resume_rng = true;
    }
    // forward scratch: one stripe per resident wave
    {
        hipDeviceProp_t prop;
        JTK_HIP_TRY(hipGetDeviceProperties(&prop, device));
        // resident waves of phmm_kernel: 3 per SIMD by registers, 11 per CU by its ~14 KB of LDS
        // resident waves per CU: 3 per SIMD by registers (JTK_PHMM_WAVES), and what 160 KiB of LDS hold
        uint32_t per_cu = (uint32_t)((160u * 1024u) / phmm_lds_bytes(s->max_tmpl, s->max_read));
        if (per_cu > 12) per_cu = 12;
        if (per_cu < 1) per_cu = 1;
        const uint32_t want = (uint32_t)prop.multiProcessorCount * per_cu;
        s->n_waves = n_reads < want ? (uint32_t)n_reads : want;
        if (s->n_waves == 0) s->n_waves = 1;
        // one stripe per wave the DEVICE can hold (3 per SIMD by registers = 12 per CU; 16 leaves room): the set is shared
        const uint64_t stride = (uint64_t)(s->max_tmpl + s->max_read + 8 + JTK_SCRATCH_GUARD) * 64 * 2;  // doubles
        const uint32_t n_stripes = (uint32_t)prop.multiProcessorCount * 16;
        std::lock_guard<std::mutex> lock(g_stripe_mutex);
        std::shared_ptr<StripePool> mine;
        // A session that launches far fewer waves than the device holds (one pile-up's modification table, the five training
        // pile-ups of the model refit) neither needs nor may grow the device's set: n_waves stripes of its own (a 60-read call
        // holds 0.3 GB, not the 19 GB of 4,096 stripes).  It uses the device's set if one of sufficient stride is already there.
        const bool small = (uint64_t)s->n_waves * 4u <= n_stripes &&
                           !(device < JTK_POOL_DEVICES && g_stripes[device] && g_stripes[device]->stride >= stride);
        std::shared_ptr<StripePool> &cur = (small || device >= JTK_POOL_DEVICES) ? mine : g_stripes[device];
        const uint32_t n_want = small ? s->n_waves : n_stripes;
        if (!cur || cur->stride < stride || cur->n < n_want) {
            auto p = std::make_shared<StripePool>();
            p->stride = std::max<uint64_t>(stride, cur ? cur->stride : 0);
            p->n = std::max<uint32_t>(n_want, cur ? cur->n : 0);
            cur.reset();  // its blocks go back to the block cache first (if no session holds it any more)
            if ((rc = dev_alloc<double>(p->mem, p->stride * p->n))) return rc;
            if ((rc = dev_alloc<uint32_t>(p->owner, p->n))) return rc;
            // every stripe free.  On the session's own stream, waited for under the lock -- NOT hipMemset: that is an operation of
            // the null stream, which then holds a hardware queue of its own for the life of the process; with four slices x two
            // streams on eight queues one slice's second stream then shared a queue with its first, and that slice's two chain
            // kernels ran one after the other (serial chain time 1,340 -> 1,490 ms per pass until this was found)
            JTK_HIP_TRY(hipMemsetAsync(p->owner.p, 0, (size_t)p->n * sizeof(uint32_t), s->stream));
            JTK_HIP_TRY(hipStreamSynchronize(s->stream));
            cur = p;
        }
        s->stripes = cur;
    }
    {  // narrow bands: two reads of a chunk per wave (phmm_pair.hip)
        std::vector<uint32_t> items;
        for (size_t c = 0; c < n_chunks; c++) {
            const ChunkMeta &cm = s->h_chunks[c];
            if (cm.radius > JTK_PAIR_MAX_RADIUS || s->h_state0[c].status != 0) continue;
            const uint32_t voters = cm.take_num ? std::min(cm.take_num, cm.n_reads) : cm.n_reads;
            for (uint32_t r = 0; r + 1 < voters; r += 2) items.push_back(cm.read_first + r);
            if (voters & 1u) items.push_back((cm.read_first + voters - 1) | 0x80000000u);
        }
        s->n_pair_items = (uint32_t)items.size();
        if (s->n_pair_items) {
            hipDeviceProp_t prop;
            JTK_HIP_TRY(hipGetDeviceProperties(&prop, device));
            const size_t pl = phmm_pair_lds_bytes(s->max_tmpl, s->max_read);
            if (pl > 160 * 1024) return jtk_fail(JTK_ERR_UNSUPPORTED, "template + reads too long for the LDS staging of phmm_pair_kernel");
            uint32_t per_cu = (uint32_t)((160u * 1024u) / pl);
            if (per_cu > 8) per_cu = 8;  // two waves per SIMD by registers
            s->n_pair_waves = std::min<uint32_t>(std::min<uint32_t>(s->n_pair_items, (uint32_t)prop.multiProcessorCount * per_cu),
                                                 s->n_waves);  // shares phmm_kernel's scratch stripes (launched after it)
            if ((rc = dev_upload(s, s->d_pair_items, items))) return rc;
        }
    }
    if (s->n_wide_reads) {
        const size_t wl = phmm_wide_lds_bytes(s->max_tmpl, s->max_read, s->max_wide_radius);
        if (wl > 160 * 1024) return jtk_fail(JTK_ERR_UNSUPPORTED, "template + read too long for the LDS staging of phmm_wide_kernel");
        hipDeviceProp_t prop;
        JTK_HIP_TRY(hipGetDeviceProperties(&prop, device));
        uint32_t per_cu = (uint32_t)((160u * 1024u) / wl);
        if (per_cu > 4) per_cu = 4;
        s->wide_stride = phmm_wide_scratch_doubles(s->max_tmpl, s->max_read, s->max_wide_radius);
        uint64_t want = (uint64_t)prop.multiProcessorCount * per_cu;
        const uint64_t budget = (48ull << 30) / (s->wide_stride * 8);  // at most 48 GB of forward tables in flight
        if (want > budget) want = budget ? budget : 1;
        s->n_wide_waves = (uint32_t)std::min<uint64_t>(s->n_wide_reads, want);
        if ((rc = dev_alloc<double>(s->d_wide_scratch, s->wide_stride * s->n_wide_waves))) return rc;
        if ((rc = dev_alloc<uint32_t>(s->d_wide_counter, 4))) return rc;
        JTK_HIP_TRY(hipMemsetAsync(s->d_wide_counter.p, 0, 4 * sizeof(uint32_t), s->stream));
    }
    // set 0 = the batch as uploaded (never written), sets 1 / 2 = what the polish rounds write (device_common.h DevBufs)
    s->bufs.tmpl[0] = s->d_tmpl_init.as<uint8_t>();
    s->bufs.tmpl[1] = s->d_tmpl0.as<uint8_t>();
    s->bufs.tmpl[2] = s->d_tmpl1.as<uint8_t>();
    s->bufs.ops[0] = s->d_ops_init.as<uint8_t>();
    s->bufs.ops[1] = s->d_ops0.as<uint8_t>();
    s->bufs.ops[2] = s->d_ops1.as<uint8_t>();
    s->bufs.ops_len[0] = s->d_opslen_init.as<uint32_t>();
    s->bufs.ops_len[1] = s->d_opslen0.as<uint32_t>();
    s->bufs.ops_len[2] = s->d_opslen1.as<uint32_t>();
    if ((rc = dev_upload(s, s->d_state0, s->h_state0))) return rc;
    tstop(s);
    JTK_HIP_TRY(hipStreamSynchronize(s->stream));
    {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, s->timers.back().a, s->timers.back().b);
        memset(&g_timing, 0, sizeof g_timing);
        g_timing.h2d_ms = ms;
    }
    const size_t lds = phmm_lds_bytes(s->max_tmpl, s->max_read);
    if (lds > 160 * 1024) return jtk_fail(JTK_ERR_UNSUPPORTED, "template + read too long for the LDS staging of phmm_kernel");
    *out = guard.release();
    return 0;
}

int jtk_lc_session_create(const jtk_lc_params_t *params, size_t n_chunks, const jtk_lc_chunk_t *chunks,
                          const uint8_t *tmpl_bases, const uint8_t *read_bases, const uint64_t *read_off,
                          const uint8_t *ops, const uint64_t *ops_off, const uint8_t *strand,
                          uint32_t post_stride, int device, jtk_lc_session_t **out) {
    return session_create_ex(params, n_chunks, chunks, tmpl_bases, read_bases, read_off, ops, ops_off, strand,
                             post_stride, device, nullptr, 3 /* mod.rs:105 */, out);
}

// one pass of the kernel sequence over the resident batch
int run_batch(jtk_lc_session_t *s, int skip_polish) {
    JTK_HIP_TRY(hipSetDevice(s->device));
    const double h2d = g_timing.h2d_ms;
    memset(&g_timing, 0, sizeof g_timing);
    g_timing.h2d_ms = h2d;
    for (auto &t : s->timers) {
        if (t.a) (void)hipEventDestroy(t.a);
        if (t.b) (void)hipEventDestroy(t.b);
    }
    s->timers.clear();
    hipStream_t st = s->stream;
    const ReadMeta *reads = s->d_reads.as<ReadMeta>();
    const ChunkMeta *chunks = s->d_chunks.as<ChunkMeta>();
    ChunkState *state = s->d_state.as<ChunkState>();
    const HmmDev *hmm2 = s->d_hmm2.as<HmmDev>();
    hipEvent_t ev0, ev1;
    JTK_HIP_TRY(hipEventCreate(&ev0));
    JTK_HIP_TRY(hipEventCreate(&ev1));
    JTK_HIP_TRY(hipEventRecord(ev0, st));
    // reset the mutable state: every chunk back to the batch as uploaded (buffer set 0 is never written, so there is
    // nothing to copy) and the per-round counters to zero -- one small kernel, no blits
    launch_reset_pass(st, s->n_chunks, state, s->d_state0.as<ChunkState>(), s->d_nactive.as<uint32_t>(), JTK_NACTIVE_SLOTS);

    tstart(s, JTK_K_POLISH);
    launch_band_prep(st, s->n_reads, reads, chunks, state, s->bufs, s->d_delta.as<uint64_t>(), 0, s->max_tmpl, s->max_read);
    tstop(s);
    // The host has to learn when every chunk has converged, but the device never waits for it: round r+1 is queued BEFORE the
    // host looks at round r's counter (a round without active chunks does nothing: every kernel of a round >= 1 skips the
    // chunks that are not active), so a pass costs at most one empty round instead of a host round trip per round.
    if (!s->h_nactive) {
        s->h_nactive = pinned_page_take();
        if (!s->h_nactive) return jtk_fail(JTK_ERR_ALLOC, "hipHostMalloc failed");
        JTK_HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&s->h_nactive_dev), s->h_nactive, 0));
        JTK_HIP_TRY(hipEventCreateWithFlags(&s->ev_round[0], hipEventDisableTiming));
        JTK_HIP_TRY(hipEventCreateWithFlags(&s->ev_round[1], hipEventDisableTiming));
    }
    // Round 6: the variant filter takes its column statistics and the picked columns' entries straight from the row sums
    // (column_filter_fused_kernel, filter_kernels.hip), so a clustering pass never materialises the N x 14(L+1) table --
    // finalize_kernel runs only where the table itself is the product (window polishing keeps its final-pass call; the
    // modification-table entry point has its own) or where a pile-up is too deep for the fused filter.
    const bool need_tables = s->polish_only || s->max_n > 65535u;  // (the fused filter counts in 16-bit fields)
    const int max_rounds = skip_polish ? 1 : JTK_POLISH_MAX_ROUNDS + 1;
    for (int round = 0; round < max_rounds; round++) {
        const int only_active = round > 0;
        const int final_pass = skip_polish || round == JTK_POLISH_MAX_ROUNDS;
        tstart(s, JTK_K_PHMM);
        launch_phmm(st, s->n_reads, reads, chunks, state, s->bufs, s->d_ey.as<uint8_t>(), s->d_delta.as<uint64_t>(),
                    hmm2, s->stripes->set(), s->n_waves, s->d_counter.as<uint32_t>(), &s->tk_phmm,
                    s->d_raw.as<double>(), s->d_rawG.as<int>(), s->d_lk.as<double>(), s->max_tmpl, s->max_read,
                    only_active, s->n_pair_items ? JTK_PAIR_MAX_RADIUS : 0);
        if (s->n_pair_items)
            launch_phmm_pair(st, s->n_pair_items, s->d_pair_items.as<uint32_t>(), reads, chunks, state, s->bufs,
                             s->d_ey.as<uint8_t>(), s->d_delta.as<uint64_t>(), hmm2, s->stripes->set(),
                             s->n_pair_waves, s->d_counter.as<uint32_t>() + 1, &s->tk_pair, s->d_raw.as<double>(), s->d_rawG.as<int>(),
                             s->d_lk.as<double>(), s->max_tmpl, s->max_read, only_active);
        if (s->n_wide_reads)
            launch_phmm_wide(st, s->n_reads, reads, chunks, state, s->bufs, s->d_ey.as<uint8_t>(), s->d_delta.as<uint64_t>(),
                             hmm2, s->d_wide_scratch.as<double>(), s->wide_stride, s->n_wide_waves,
                             s->d_wide_counter.as<uint32_t>(), &s->tk_wide, s->d_raw.as<double>(), s->d_rawG.as<int>(),
                             s->d_lk.as<double>(), s->max_tmpl, s->max_read, only_active, s->max_wide_radius);
        // A polish round needs the column totals of the active chunks, not their per-read tables: the totals come straight from
        // the row sums (sum_final_kernel), and only a chunk that turns out to have converged -- no edit selected -- gets its
        // table, once, from the row sums it still holds.  The last pass materialises the tables of whatever is still active.
        if (final_pass) {
            if (need_tables)
                launch_finalize(st, s->n_reads, reads, chunks, state, hmm2, s->d_raw.as<double>(), s->d_rawG.as<int>(),
                                s->d_lk.as<double>(), s->max_tmpl, only_active);
        } else
            launch_sum_final(st, s->n_chunks, reads, chunks, state, hmm2, s->d_raw.as<double>(), s->d_rawG.as<int>(),
                             s->d_lk.as<double>(), s->d_total.as<double>(), s->max_tmpl);
        tstop(s);
        tstart(s, JTK_K_POLISH);
        launch_polish_round(st, s->n_chunks, s->n_reads, reads, chunks, state, s->bufs, s->d_ey.as<uint8_t>(),
                            s->d_raw.as<double>(), s->d_total.as<double>(), s->d_edits.as<Edit>(),
                            s->d_newlen.as<uint32_t>(), s->max_tmpl, s->ignore_edge, final_pass,
                            s->d_nactive.as<uint32_t>() + round, s->h_nactive_dev + round);
        if (!final_pass)
            launch_band_prep(st, s->n_reads, reads, chunks, state, s->bufs, s->d_delta.as<uint64_t>(), 1, s->max_tmpl, s->max_read);
        tstop(s);
        if (!final_pass && !s->polish_only && need_tables) {  // the chunks that converged in this round: their tables, for the variant search
            tstart(s, JTK_K_PHMM);
            launch_finalize(st, s->n_reads, reads, chunks, state, hmm2, s->d_raw.as<double>(), s->d_rawG.as<int>(),
                            s->d_lk.as<double>(), s->max_tmpl, 0, round);
            tstop(s);
        }
        if (final_pass) break;
        // commit_kernel has stored the round's count in h_nactive[round] itself (mapped pinned memory): no read-back copy
        JTK_HIP_TRY(hipEventRecord(s->ev_round[round & 1], st));
        if (round >= 1) {
            JTK_HIP_TRY(hipEventSynchronize(s->ev_round[(round - 1) & 1]));
            if (s->h_nactive[round - 1] == 0) break;  // round `round` was already queued and finds nothing to do
        }
    }
    if (!s->polish_only) {
    tstart(s, JTK_K_FILTER);
    launch_filter(st, s->n_chunks, reads, chunks, state, s->bufs, s->d_params.as<jtk_lc_params_t>(),
                  s->d_raw.as<double>(), s->d_homop.as<uint16_t>(), s->d_homop_off.as<uint64_t>(),
                  s->d_aux.as<double>(), s->d_aux_off.as<uint64_t>(), s->d_cand.as<double>(), s->d_list.as<uint32_t>(),
                  s->d_sel.as<uint8_t>(), s->d_feat.as<double>(), s->d_vtype.as<uint32_t>(), s->d_pos.as<uint32_t>(),
                  s->max_tmpl, hmm2, s->d_rawG.as<int>(), s->d_lk.as<double>(), need_tables ? 0 : 1);
    tstop(s);
    tstart(s, JTK_K_MCMC);
    int mcmc_rc = 0;
    for (int j = 0; j < 2; j++) {
        const ChainClass &cc = s->chain_class[j];
        if (cc.count == 0 || mcmc_rc != 0) continue;
        // the class's own stretch of the split scratch: 2 + 2 * count words from 2 * first + 4 * j
        mcmc_rc = launch_mcmc(st, cc.count, chunks, state, s->d_params.as<jtk_lc_params_t>(), s->d_feat.as<double>(),
                              s->d_vtype.as<uint32_t>(), nullptr, 0, s->d_label.as<uint32_t>(), s->d_post.as<double>(),
                              s->post_stride, s->d_lg.as<double>(), s->d_lg_off.as<uint64_t>(), cc.lds_n, cc.lds_d, cc.lds_k,
                              s->resume_rng ? s->d_rng.as<uint64_t>() : nullptr, s->d_order.as<uint32_t>() + cc.first,
                              s->d_chain_split.as<uint32_t>() + 2 * cc.first + 4 * j, s->side, s->ev_chain[0], s->ev_chain[1]);
    }
    if (s->chain_class[2].count && mcmc_rc == 0) {
        const ChainClass &cc = s->chain_class[2];
        mcmc_rc = launch_mcmc_huge(st, cc.count, chunks, state, s->d_params.as<jtk_lc_params_t>(), s->d_feat.as<double>(),
                                   s->d_vtype.as<uint32_t>(), nullptr, 0, s->d_label.as<uint32_t>(), s->d_post.as<double>(),
                                   s->post_stride, s->d_lg.as<double>(), s->d_lg_off.as<uint64_t>(), cc.lds_n, cc.lds_d, cc.lds_k,
                                   s->resume_rng ? s->d_rng.as<uint64_t>() : nullptr, s->d_order.as<uint32_t>() + cc.first,
                                   s->d_chain_ws.as<uint8_t>(), s->d_chain_ws_off.as<uint64_t>());
    }
    tstop(s);
    if (mcmc_rc != 0) {
        (void)hipStreamSynchronize(st);
        return jtk_fail(JTK_ERR_INTERNAL, "the chain kernel could not be launched (jump table upload failed)");
    }
    s->ran = true;
    s->ran_fused = !need_tables;
    }  // !polish_only
    JTK_HIP_TRY(hipEventRecord(ev1, st));
    JTK_HIP_TRY(hipStreamSynchronize(st));
    JTK_HIP_TRY(hipGetLastError());
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ev0, ev1);
    g_timing.total_ms = ms;
    for (int j = 0; j < 2; j++) g_timing.chain_lds_bytes[j] = s->chain_class[j].count ? s->chain_class[j].lds_bytes : 0;
    (void)hipEventDestroy(ev0);
    (void)hipEventDestroy(ev1);
    for (auto &t : s->timers) {
        if (t.kind < 0 || t.kind >= JTK_K_COUNT) continue;
        float k = 0;
        (void)hipEventElapsedTime(&k, t.a, t.b);
        g_timing.kernel_ms[t.kind] += k;
        g_timing.kernel_launches[t.kind] += 1;
    }
    return 0;
}

int jtk_lc_session_run(jtk_lc_session_t *s, int skip_polish) {
    g_last_error.clear();
    if (!s) return jtk_fail(JTK_ERR_INVALID_ARG, "null session");
    int rc = run_batch(s, skip_polish);
    if (rc == 0 && s->has_split) rc = run_split(s);
    return rc;
}

// ---- the reference's trace! rows of one chunk (include/jtk_lc.h: jtk_lc_session_trace)
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
        const uint32_t k = std::min<uint32_t>(std::max<uint32_t>(cm.copy_num, 2u), JTK_MAX_COPY);
        const uint32_t dmax = std::min<uint32_t>(JTK_MAX_DIM, 3u * std::max<uint32_t>(cm.copy_num, 2u));
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

// A fetch in two halves, so that the slices of a one-shot call can write their variable-length outputs straight into the
// caller's arrays: fetch_begin copies the fixed-size results (labels, posteriors, per-chunk records) and learns the lengths of the
// variable ones; the caller then says where this session's consensus / ops start (one-shot slices: after the previous slice's),
// and fetch_finish packs them on the device (gather_kernel) and copies exactly those bytes to their final place.  Until round 5
// every buffer set some chunk's result lived in was downloaded whole into fresh host vectors (up to 3 x the ops + templates of the
// batch) and unpacked base by base on the host.
int fetch_begin(jtk_lc_session_t *s, FetchPlan &pl, uint32_t *label, double *log_post, jtk_lc_result_t *result, bool want_cons,
                bool want_ops) {
    JTK_HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = s->stream;
    JTK_HIP_TRY(hipEventCreate(&pl.ev0));
    JTK_HIP_TRY(hipEventRecord(pl.ev0, st));
    pl.want_cons = want_cons;
    pl.want_ops = want_ops;
    pl.state.resize(s->n_chunks);
    JTK_HIP_TRY(hipMemcpyAsync(pl.state.data(), s->d_state.p, pl.state.size() * sizeof(ChunkState), hipMemcpyDeviceToHost, st));
    if (want_cons || want_ops) {
        if (!s->d_out_len.p) {
            int rc;
            if ((rc = dev_alloc<uint32_t>(s->d_out_len, (size_t)s->n_reads + s->n_chunks))) return rc;
            if ((rc = dev_alloc<uint64_t>(s->d_out_off, (size_t)s->n_reads + s->n_chunks + 2))) return rc;
        }
        pl.len.resize((size_t)s->n_reads + s->n_chunks);
        launch_out_len(st, s->n_reads, s->n_chunks, s->d_reads.as<ReadMeta>(), s->d_state.as<ChunkState>(), s->bufs,
                       s->d_out_len.as<uint32_t>(), s->d_out_len.as<uint32_t>() + s->n_reads);
        if (!pl.len.empty())
            JTK_HIP_TRY(hipMemcpyAsync(pl.len.data(), s->d_out_len.p, pl.len.size() * 4, hipMemcpyDeviceToHost, st));
    }
    if (label) JTK_HIP_TRY(hipMemcpyAsync(label, s->d_label.p, (size_t)s->n_reads * 4, hipMemcpyDeviceToHost, st));
    if (log_post)
        JTK_HIP_TRY(hipMemcpyAsync(log_post, s->d_post.p, (size_t)s->n_reads * s->post_stride * 8, hipMemcpyDeviceToHost, st));
    JTK_HIP_TRY(hipStreamSynchronize(st));
    for (uint32_t c = 0; c < s->n_chunks; c++) {
        const ChunkState &cs = pl.state[c];
        if (cs.status != 0) {
            pl.any_fail = 1;
            // a failed chunk has no clustering: its reads get label 0 and zero posteriors, not whatever the device buffers held
            // (round 6: found by comparing a sliced call with the same call in one piece)
            const ChunkMeta &cm = s->h_chunks[c];
            for (uint32_t r = 0; r < cm.n_reads; r++) {
                if (label) label[cm.read_first + r] = 0;
                if (log_post)
                    for (uint32_t t = 0; t < s->post_stride; t++) log_post[(size_t)(cm.read_first + r) * s->post_stride + t] = 0.0;
            }
        }
        if (result) {
            result[c].score = cs.status == 0 ? cs.score : 0.0;
            result[c].cluster_num = cs.status == 0 ? cs.k : 1;
            result[c].status = cs.status;
            result[c].polish_rounds = cs.rounds;
            result[c].n_variants = cs.dim;
        }
    }
    if (want_ops)
        for (uint32_t g = 0; g < s->n_reads; g++) pl.ops_total += pl.len[g];
    if (want_cons)
        for (uint32_t c = 0; c < s->n_chunks; c++) pl.cons_total += pl.len[s->n_reads + c];
    return 0;
}

// cons_out / ops_out: the caller's arrays; cons_off / ops_out_off: the entries of THIS session's chunks / reads (n_chunks + 1 and
// n_reads + 1 of them are written); cons_base / ops_base: where this session's bytes start inside the arrays
int fetch_finish(jtk_lc_session_t *s, FetchPlan &pl, uint8_t *cons_out, uint64_t *cons_off, uint64_t cons_base, uint64_t cons_cap,
                 uint8_t *ops_out, uint64_t *ops_out_off, uint64_t ops_base, uint64_t ops_cap) {
    JTK_HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = s->stream;
    if (pl.want_cons && cons_base + pl.cons_total > cons_cap) return jtk_fail(JTK_ERR_INVALID_ARG, "cons_cap too small");
    if (pl.want_ops && ops_base + pl.ops_total > ops_cap) return jtk_fail(JTK_ERR_INVALID_ARG, "ops_cap too small");
    std::vector<uint64_t> off;   // (source of an asynchronous upload: lives until the stream has been waited for, below)
    if (pl.want_cons || pl.want_ops) {
        // offsets local to the session (the device packs from 0), written to the caller's arrays with the base added
        off.resize((size_t)s->n_reads + s->n_chunks + 2);
        uint64_t *ooff = off.data(), *coff = off.data() + s->n_reads + 1;
        uint64_t oo = 0, co = 0;
        for (uint32_t g = 0; g < s->n_reads; g++) {
            ooff[g] = oo;
            oo += pl.want_ops ? pl.len[g] : 0;
        }
        ooff[s->n_reads] = oo;
        for (uint32_t c = 0; c < s->n_chunks; c++) {
            coff[c] = co;
            co += pl.want_cons ? pl.len[s->n_reads + c] : 0;
        }
        coff[s->n_chunks] = co;
        int rc;
        if (pl.want_ops && !s->d_out_ops.p && (rc = dev_alloc<uint8_t>(s->d_out_ops, s->ops_bytes + 8))) return rc;
        if (pl.want_cons && !s->d_out_cons.p && (rc = dev_alloc<uint8_t>(s->d_out_cons, s->tmpl_bytes + 8))) return rc;
        JTK_HIP_TRY(hipMemcpyAsync(s->d_out_off.p, off.data(), off.size() * 8, hipMemcpyHostToDevice, st));
        launch_gather(st, s->n_reads, s->n_chunks, s->d_reads.as<ReadMeta>(), s->d_chunks.as<ChunkMeta>(), s->d_state.as<ChunkState>(),
                      s->bufs, s->d_out_off.as<uint64_t>(), s->d_out_off.as<uint64_t>() + s->n_reads + 1,
                      pl.want_ops ? s->d_out_ops.as<uint8_t>() : nullptr, pl.want_cons ? s->d_out_cons.as<uint8_t>() : nullptr);
        if (pl.want_ops && oo) JTK_HIP_TRY(hipMemcpyAsync(ops_out + ops_base, s->d_out_ops.p, oo, hipMemcpyDeviceToHost, st));
        if (pl.want_cons && co) JTK_HIP_TRY(hipMemcpyAsync(cons_out + cons_base, s->d_out_cons.p, co, hipMemcpyDeviceToHost, st));
        if (pl.want_ops)
            for (uint32_t g = 0; g <= s->n_reads; g++) ops_out_off[g] = ops_base + ooff[g];
        if (pl.want_cons)
            for (uint32_t c = 0; c <= s->n_chunks; c++) cons_off[c] = cons_base + coff[c];
    }
    hipEvent_t ev1;
    JTK_HIP_TRY(hipEventCreate(&ev1));
    JTK_HIP_TRY(hipEventRecord(ev1, st));
    JTK_HIP_TRY(hipStreamSynchronize(st));
    JTK_HIP_TRY(hipGetLastError());
    float ms = 0;
    (void)hipEventElapsedTime(&ms, pl.ev0, ev1);
    g_timing.d2h_ms = ms;
    (void)hipEventDestroy(pl.ev0);
    (void)hipEventDestroy(ev1);
    pl.ev0 = nullptr;
    return 0;
}

// chunks that went through clustering_recursive's split: the merged clustering replaces the first pass's
int fetch_split_results(jtk_lc_session_t *s, uint32_t *label, double *log_post, jtk_lc_result_t *result) {
    int any_fail = 0;
    for (uint32_t c = 0; c < s->n_chunks && c < s->split.size(); c++) {
        const SplitResult &sr = s->split[c];
        if (sr.k == 0) continue;
        const ChunkMeta &cm = s->h_chunks[c];
        if (sr.status != 0) any_fail = 1;
        if (result) {
            result[c].score = sr.status == 0 ? sr.score : 0.0;
            result[c].cluster_num = sr.status == 0 ? sr.k : 1;
            result[c].status = sr.status;
        }
        for (uint32_t r = 0; r < cm.n_reads; r++) {
            const uint32_t g = cm.read_first + r;
            if (label) label[g] = sr.status == 0 ? sr.asn[r] : 0;
            if (log_post)
                for (uint32_t t = 0; t < s->post_stride; t++)
                    log_post[(size_t)g * s->post_stride + t] = (sr.status == 0 && t < sr.k) ? sr.post[(size_t)r * sr.k + t] : 0.0;
        }
    }
    return any_fail;
}

int jtk_lc_session_fetch(jtk_lc_session_t *s, uint32_t *label, double *log_post, jtk_lc_result_t *result,
                         uint8_t *cons_out, uint64_t *cons_off, uint64_t cons_cap, uint8_t *ops_out,
                         uint64_t *ops_out_off, uint64_t ops_cap) {
    g_last_error.clear();
    if (!s) return jtk_fail(JTK_ERR_INVALID_ARG, "null session");
    FetchPlan pl;
    int rc = fetch_begin(s, pl, label, log_post, result, cons_out && cons_off, ops_out && ops_out_off);
    if (rc == 0) rc = fetch_finish(s, pl, cons_out, cons_off, 0, cons_cap, ops_out, ops_out_off, 0, ops_cap);
    if (pl.ev0) (void)hipEventDestroy(pl.ev0);
    if (rc) return rc;
    const int any_fail = pl.any_fail | fetch_split_results(s, label, log_post, result);
    return any_fail ? jtk_fail(JTK_ERR_CHUNK_FAILED, "at least one chunk failed; see result[].status") : 0;
}

int jtk_lc_session_destroy(jtk_lc_session_t *s) {
    if (!s) return 0;
    (void)hipSetDevice(s->device);
    delete s;
    return 0;
}

int jtk_lc_trim_cache(int device) {
    if (device < 0 || device >= JTK_POOL_DEVICES) return JTK_ERR_INVALID_ARG;
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess) return JTK_ERR_NO_DEVICE;
    (void)hipSetDevice(device);
    {
        std::lock_guard<std::mutex> lock(g_stripe_mutex);
        g_stripes[device].reset();  // running sessions keep the set they hold
    }
    g_pool.trim(device);
    (void)hipSetDevice(cur);
    return 0;
}

const char *jtk_lc_last_error(void) { return g_last_error.c_str(); }

int jtk_lc_last_timing(jtk_lc_timing_t *out) {
    if (!out) return JTK_ERR_INVALID_ARG;
    *out = g_timing;
    return 0;
}

int jtk_lc_device_ok(int device) {
    const std::string keep = g_last_error;
    const int rc = jtk_require_device(device);
    g_last_error = keep;
    return rc == 0 ? 1 : 0;
}
