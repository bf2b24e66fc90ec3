// session.hip -- the resident-batch session: its pools, the session object and the C-ABI entry points of include/jtk_lc.h that
// create, run, fetch and destroy one.
//
// One process drives one GPU.  A session validates and encodes the flat host batch (its layout is session_plan.h's: this file
// computes no offset, launch class or wave count of its own), uploads it once, allocates
// every workspace up front (sized for 288 GB of HBM: the full N x 14(L+1) tables of all chunks stay
// resident), and then runs the stage as a short sequence of kernel launches on its lane's stream (session_lanes.h):
//
//   band_prep -> [ phmm -> finalize -> polish_round ]* until no chunk is active -> filter -> mcmc
//
// (mod.rs:86-123 per chunk).  The last polishing pass that finds no edit has produced exactly the
// modification table `clustering` would recompute (same consensus, same ops, same radius: mod.rs:105 vs
// :112, pseudo_mcmc.rs:117), so it is reused instead of recomputed.
//
// The other entry points are built on the session (session_internal.h): the split branch of chunks with copy_num >= 8
// (session_split.hip), the one-shot stage calls and window polishing (session_stages.hip), the model refit and the
// modification table (session_refit.hip), the features-only chain (session_features.hip), the trace of a finished session
// (session_trace.hip).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <thread>

#include "session_internal.h"
#include "session_plan.h"

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

// ROCm maps streams onto GPU_MAX_HW_QUEUES hardware queues (4 by default) and streams that share a queue run in order: a
// slice's 300 ms chain kernel would then hold up another slice's pair-HMM launches.  So sessions do not own streams: they take
// them from the device's lanes (session_lanes.h), as many as the queues pay for, and the sessions of a lane launch their
// chains as one kernel.  Where nobody has chosen a queue count the library asks for 12 when it is loaded (the variable is read
// when the HIP runtime initialises): four lanes of two streams -- the chain's general kernel runs beside its light one -- and
// the host's own streams (the null stream as soon as anything uses it).  A host's own value is never overwritten: the lanes
// are fitted to it.
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

// The lanes, per device: made on demand, never destroyed (a stream that outlives its sessions costs nothing, and no session
// of a later call has to wait for hipStreamDestroy).
// Beside the streams, the lane's ledger (include/jtk_lc_debug.h): what each of the last calls of launch_lane_chains put into
// its two class launches, and the holds a test has taken on the lane's gather.
struct LaneLedger {
    std::mutex m;
    unsigned long long calls = 0;
    jtk_lc_debug_lane_launch_t ring[JTK_LANE_LEDGER] = {};  // call c at c % JTK_LANE_LEDGER, as LaneGather keeps its member counts
    int holds = 0;
};
static_assert(JTK_LANE_LEDGER == JTK_LC_DEBUG_LANE_RECORDS && JTK_LANE_MAX_SEGMENTS == 8, "jtk_lc_debug_lane_launch_t");
// The same for the lane's round launches (launch_lane_rounds): what each of the last calls carried.
struct RoundLedger {
    std::mutex m;
    unsigned long long calls = 0;
    jtk_lc_debug_round_launch_t ring[JTK_LC_DEBUG_ROUND_RECORDS] = {};
};
static_assert(JTK_ROUND_MAX_SEGMENTS == 8 && JTK_LANE_MAX_SEGMENTS <= JTK_ROUND_MAX_SEGMENTS, "jtk_lc_debug_round_launch_t");
struct LaneStreams {
    hipStream_t stream = nullptr, side = nullptr;
    hipEvent_t ev_chain[2] = {nullptr, nullptr};
    LaneLedger ledger;
    // the round launches that come through the lane's gather: phmm_kernel's never-reset ticket counter (device, zeroed once on
    // the lane's stream) and its host mirror, both touched only by launch_lane_rounds, which runs under the round gather's mutex
    uint32_t *d_round_counter = nullptr;
    uint32_t tk_round = 0;
    RoundLedger round_ledger;
    // which of {stream, side} carries rounds now, and the merged launches that members may still be waiting in
    // (session_lanes.h: the stream rule, LaneFlow); under `flow`
    std::mutex flow;
    LaneFlow flights;
};
typedef LaneTable<LaneStreams, jtk_lc_session> DeviceLanes;
std::mutex g_lanes_mutex;  // the map, and the late creation of a lane's side stream
std::map<int, DeviceLanes *> g_lanes;
DeviceLanes &device_lanes(int device) {
    std::lock_guard<std::mutex> lock(g_lanes_mutex);
    DeviceLanes *&t = g_lanes[device];
    if (!t) t = new DeviceLanes();
    return *t;
}

// The session's streams as its lane has them now: `stream` the lane's round stream, `side` (if the session uses one) the other.
// At the start of every pass and when the session has left a merged launch; returns the round stream's index.
int bind_lane_streams(jtk_lc_session *s, bool want_side) {
    LaneStreams &ls = device_lanes(s->device).lane(s->lane).streams;
    std::lock_guard<std::mutex> lock(ls.flow);
    hipStream_t two[2] = {ls.stream, ls.side};
    const int idx = ls.flights.round_stream(ls.side != nullptr);
    s->stream = two[idx];
    // (After a leave this is the stream that still carries the light chain the session left.  Only the launches of a session
    // that enters no gather read s->side, and such a session never leaves; anything else put there would queue behind that kernel.)
    if (want_side && ls.side) s->side = two[1 - idx];
    return idx;
}

// The session's streams: the least loaded lane of its device.  The lane count follows the hardware queues the process runs on
// -- the host's GPU_MAX_HW_QUEUES, or the 12 this library asked for -- unless JTK_LC_LANES gives it; JTK_LC_SIDE_STREAM says
// whether the session uses the lane's second stream.  Both are read here, when a session is created.
int take_lane(jtk_lc_session *s, bool want_side) {
    const char *fl = getenv("JTK_LC_LANES"), *fs = getenv("JTK_LC_SIDE_STREAM");
    const int queues = g_queues_by_library ? 12 : (g_host_queues > 0 ? g_host_queues : 4);
    const LanePlan lp = lane_plan(queues, fl ? atoi(fl) : 0, fs ? atoi(fs) : -1);
    DeviceLanes &t = device_lanes(s->device);
    const int lane = t.acquire(lp.max_lanes, [](LaneStreams &ls) { return hipStreamCreate(&ls.stream) == hipSuccess; });
    if (lane < 0) return jtk_fail(JTK_ERR_INTERNAL, "hipStreamCreate failed");
    DeviceLanes::Lane &L = t.lane(lane);
    s->lane = lane;
    s->gather = &L.gather;
    JTK_HIP_TRY(hipEventCreateWithFlags(&s->ev_done, hipEventDisableTiming));
    {
        std::lock_guard<std::mutex> lock(g_lanes_mutex);
        if (!L.streams.d_round_counter) {  // (kept with the lane for the life of the process, like its streams)
            uint32_t *c = nullptr;
            JTK_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&c), 4 * sizeof(uint32_t)));
            JTK_HIP_TRY(hipMemsetAsync(c, 0, 4 * sizeof(uint32_t), L.streams.stream));
            L.streams.d_round_counter = c;
        }
    }
    s->rounds = &L.rounds;
    if (want_side && lp.side) {
        std::lock_guard<std::mutex> lock(g_lanes_mutex);
        if (!L.streams.side) {
            hipStream_t side = nullptr;
            JTK_HIP_TRY(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
            JTK_HIP_TRY(hipEventCreateWithFlags(&L.streams.ev_chain[0], hipEventDisableTiming));
            JTK_HIP_TRY(hipEventCreateWithFlags(&L.streams.ev_chain[1], hipEventDisableTiming));
            std::lock_guard<std::mutex> flow(L.streams.flow);
            L.streams.side = side;
        }
        s->ev_chain[0] = L.streams.ev_chain[0];
        s->ev_chain[1] = L.streams.ev_chain[1];
    }
    (void)bind_lane_streams(s, want_side && lp.side);
    return 0;
}

}  // namespace

DevPtr::~DevPtr() {
    if (!p) return;
    if (dev < 0 || dev >= JTK_POOL_DEVICES || !g_pool.give(dev, p, cap)) (void)hipFree(p);
}

// The mapped pinned pages the polish rounds and the chain report into (JTK_PINNED_WORDS words per session): taken from and returned to
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
    if (hipHostMalloc(reinterpret_cast<void **>(&p), JTK_PINNED_WORDS * sizeof(uint32_t), hipHostMallocMapped | hipHostMallocPortable) != hipSuccess)
        return nullptr;
    return p;
}
static void pinned_page_give(uint32_t *p) {
    std::lock_guard<std::mutex> lock(g_pinned_mutex);
    g_pinned_free.push_back(p);
}

// The session's own work, not the stream: the lane's other sessions go on putting kernels behind it.  (Whatever the session
// ran on the side stream has been joined into `stream` by the launch that put it there.)
int session_wait(jtk_lc_session *s) {
    if (!s->ev_done) {
        JTK_HIP_TRY(hipStreamSynchronize(s->stream));
        return 0;
    }
    JTK_HIP_TRY(hipEventRecord(s->ev_done, s->stream));
    JTK_HIP_TRY(hipEventSynchronize(s->ev_done));
    return 0;
}

// A session that left a merged launch through its word has kernels of that launch still running -- on its lane-mates' chunks,
// never on its own buffers again.  Whatever frees, resizes or hands back those buffers waits for the launch as a whole all the same.
int session_chain_settled(jtk_lc_session *s) {
    if (s->flight && s->flight->end) JTK_HIP_TRY(hipEventSynchronize(s->flight->end));
    s->flight.reset();
    return 0;
}

// order stamps of the pass ledger (include/jtk_lc_debug.h)
static std::atomic<uint64_t> g_order{0};
static uint64_t order_stamp() { return ++g_order; }
static jtk_lc_debug_pass_t &pass_record(jtk_lc_session *s) { return s->pass_log[s->n_passes % JTK_LC_DEBUG_PASS_RECORDS]; }  // under pass_log_mutex

void timers_clear(std::vector<KernelTimer> &timers) {
    for (auto &t : timers) {
        if (t.shared) continue;
        if (t.a) (void)hipEventDestroy(t.a);
        if (t.b) (void)hipEventDestroy(t.b);
    }
    timers.clear();
}

jtk_lc_session::~jtk_lc_session() {
    (void)session_chain_settled(this);
    if (stream) (void)session_wait(this);  // blocks go back to the pool, not through hipFree's implicit sync
    timers_clear(timers);
    if (ev_done) (void)hipEventDestroy(ev_done);
    if (lane >= 0)   // the streams and the chain events stay with the lane
        device_lanes(device).release(lane);
    else if (stream)
        (void)hipStreamDestroy(stream);
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

// The steps of session_create_ex, in the order of their HIP calls on the session's stream.  Every offset, total, launch class
// and wave count they use comes from the plan (session_plan.h).  Host vectors that are the source of an asynchronous upload
// live in session_create_ex (the plan, the session's own) until it has waited for the stream.

// the metadata, the chain's launch order, the templates; the polish rounds' buffer sets and the row sums
static int upload_batch(jtk_lc_session *s, const BatchPlan &bp, const std::vector<jtk_lc_params_t> &pv, const std::vector<HmmDev> &hv,
                        const std::vector<uint8_t> &h_tmpl) {
    int rc;
    if ((rc = dev_upload(s, s->d_params, pv))) return rc;
    if ((rc = dev_upload(s, s->d_hmm2, hv))) return rc;
    if ((rc = dev_upload(s, s->d_chunks, s->h_chunks))) return rc;
    if (s->chain_class[2].count) {  // class 2: one workgroup per chunk, its own slice of a global workspace
        if ((rc = dev_alloc<uint8_t>(s->d_chain_ws, bp.chain.ws_bytes))) return rc;
        if ((rc = dev_upload(s, s->d_chain_ws_off, bp.chain.ws_off))) return rc;
    }
    if ((rc = dev_upload(s, s->d_order, bp.chain.order))) return rc;
    if ((rc = dev_upload(s, s->d_reads, s->h_reads))) return rc;
    if ((rc = dev_alloc<ChunkState>(s->d_state, s->n_chunks))) return rc;
    if ((rc = dev_upload(s, s->d_tmpl_init, h_tmpl))) return rc;
    if ((rc = dev_alloc<uint8_t>(s->d_ops_init, bp.ops))) return rc;
    if ((rc = dev_upload(s, s->d_opslen_init, bp.opslen))) return rc;
    // (+8: the polish kernels fetch templates / reads in aligned 8-byte blocks)
    if ((rc = dev_alloc<uint8_t>(s->d_tmpl0, h_tmpl.size() + 8))) return rc;
    if ((rc = dev_alloc<uint8_t>(s->d_tmpl1, h_tmpl.size() + 8))) return rc;
    if ((rc = dev_alloc<uint8_t>(s->d_ops0, bp.ops))) return rc;
    if ((rc = dev_alloc<uint8_t>(s->d_ops1, bp.ops))) return rc;
    if ((rc = dev_alloc<uint32_t>(s->d_opslen0, bp.n_reads))) return rc;
    if ((rc = dev_alloc<uint32_t>(s->d_opslen1, bp.n_reads))) return rc;
    if ((rc = dev_alloc<uint8_t>(s->d_ey, bp.ey + 8))) return rc;
    JTK_HIP_TRY(hipMemsetAsync(s->d_ey.as<uint8_t>() + bp.ey, 0, 8, s->stream));   // (the polish kernels fetch aligned 8-byte blocks)
    if ((rc = dev_alloc<uint64_t>(s->d_delta, bp.delta))) return rc;
    if ((rc = dev_alloc<double>(s->d_raw, bp.raw))) return rc;
    return 0;
}

// The reads and their ops, as the caller holds them (ASCII bases, one op per byte, back to back), straight from the
// caller's memory into the workspace the row sums will occupy later (296 KB per read against ~4 KB of input), then
// validated and recoded on the device by encode_reads_kernel (io_kernels.hip): no recoded copy on the host, no first-touch
// of fresh host vectors.  `raw_doubles`: what d_raw holds.
static int stage_reads(jtk_lc_session *s, uint64_t n_reads, const uint8_t *read_bases, const uint64_t *read_off, const uint8_t *ops,
                       const uint64_t *ops_off, uint64_t raw_doubles) {
    if (!n_reads) return 0;
    int rc;
    const uint64_t rb0 = read_off[0], rb_bytes = read_off[n_reads] - rb0, ob0 = ops_off[0], ob_bytes = ops_off[n_reads] - ob0;
    const uint64_t o_bases = 0, o_ops = (rb_bytes + 15) & ~15ull, o_boff = o_ops + ((ob_bytes + 15) & ~15ull),
                   o_ooff = o_boff + (n_reads + 1) * 8, o_flag = o_ooff + (n_reads + 1) * 8, need = o_flag + 16;
    DevPtr tmp;   // (only when the row sums' block is too small for it: pile-ups of very short templates)
    uint8_t *stage = s->d_raw.as<uint8_t>();
    if (need > raw_doubles * 8) {
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
    if ((rc = session_wait(s))) return rc;   // (also: `tmp` may go back to the pool)
    JTK_HIP_TRY(hipGetLastError());
    if (flags & 2u) return jtk_fail(JTK_ERR_INVALID_ARG, "non-ACGT base in a read");
    if (flags & 4u) return jtk_fail(JTK_ERR_INVALID_ARG, "bad op code");
    return 0;
}

// what every pass needs beside the buffer sets (no buffer for the tables: they live where the row sums were, d_raw)
static int alloc_polish_workspaces(jtk_lc_session *s, const BatchPlan &bp) {
    int rc;
    if ((rc = dev_alloc<int>(s->d_rawG, bp.row))) return rc;
    if ((rc = dev_alloc<double>(s->d_lk, bp.n_reads))) return rc;
    if ((rc = dev_alloc<double>(s->d_total, bp.total))) return rc;
    if ((rc = dev_alloc<Edit>(s->d_edits, bp.edit))) return rc;
    if ((rc = dev_alloc<uint32_t>(s->d_newlen, s->n_chunks))) return rc;
    if ((rc = dev_alloc<uint32_t>(s->d_counter, 4))) return rc;
    JTK_HIP_TRY(hipMemsetAsync(s->d_counter.p, 0, 4 * sizeof(uint32_t), s->stream));  // once: the ticket counters are never reset
    if ((rc = dev_alloc<uint32_t>(s->d_nactive, JTK_NACTIVE_SLOTS))) return rc;
    if ((rc = dev_alloc<uint32_t>(s->d_chain_split, 2 * (size_t)s->n_chunks + 8))) return rc;
    return 0;
}

// the filter's and the chain's workspaces
static int alloc_cluster_workspaces(jtk_lc_session *s, const BatchPlan &bp) {
    int rc;
    if ((rc = dev_alloc<uint16_t>(s->d_homop, bp.tmpl))) return rc;
    if ((rc = dev_upload(s, s->d_homop_off, bp.homop_off))) return rc;
    if ((rc = dev_alloc<double>(s->d_aux, bp.aux))) return rc;
    if ((rc = dev_upload(s, s->d_aux_off, bp.aux_off))) return rc;
    if ((rc = dev_alloc<double>(s->d_cand, bp.cand))) return rc;
    if ((rc = dev_alloc<uint32_t>(s->d_list, bp.cand))) return rc;
    if ((rc = dev_alloc<uint8_t>(s->d_sel, bp.cand))) return rc;
    if ((rc = dev_alloc<double>(s->d_feat, bp.feat))) return rc;
    if ((rc = dev_alloc<uint32_t>(s->d_vtype, (uint64_t)2 * s->n_chunks * JTK_MAX_DIM))) return rc;
    if ((rc = dev_alloc<uint32_t>(s->d_pos, (uint64_t)s->n_chunks * JTK_MAX_DIM))) return rc;
    if ((rc = dev_alloc<uint32_t>(s->d_label, bp.n_reads))) return rc;
    if ((rc = dev_alloc<double>(s->d_post, bp.n_reads * s->post_stride))) return rc;
    if ((rc = dev_alloc<double>(s->d_lg, bp.lg))) return rc;
    if ((rc = dev_upload(s, s->d_lg_off, bp.lg_off))) return rc;
    return 0;
}

// forward scratch: one stripe of `stride` doubles per resident wave, from the device's shared set of `n_stripes`
static int acquire_stripes(jtk_lc_session *s, uint64_t stride, uint32_t n_stripes, uint32_t n_waves) {
    const int device = s->device;
    int rc;
    std::lock_guard<std::mutex> lock(g_stripe_mutex);
    std::shared_ptr<StripePool> mine;
    // A session that launches far fewer waves than the device holds (one pile-up's modification table, the five training
    // pile-ups of the model refit) neither needs nor may grow the device's set: n_waves stripes of its own (a 60-read call
    // holds 0.3 GB, not the 19 GB of 4,096 stripes).  It uses the device's set if one of sufficient stride is already there.
    const bool small = (uint64_t)n_waves * 4u <= n_stripes &&
                       !(device < JTK_POOL_DEVICES && g_stripes[device] && g_stripes[device]->stride >= stride);
    std::shared_ptr<StripePool> &cur = (small || device >= JTK_POOL_DEVICES) ? mine : g_stripes[device];
    const uint32_t n_want = small ? n_waves : n_stripes;
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
        if ((rc = session_wait(s))) return rc;
        cur = p;
    }
    s->stripes = cur;
    return 0;
}

// the item list of phmm_pair_kernel and the scratch of phmm_wide_kernel, where the batch has chunks for them
static int upload_pair_and_wide(jtk_lc_session *s, const BatchPlan &bp) {
    int rc;
    if (s->n_pair_items && (rc = dev_upload(s, s->d_pair_items, bp.pair_items))) return rc;
    if (s->n_wide_reads) {
        if ((rc = dev_alloc<double>(s->d_wide_scratch, s->wide_stride * s->n_wide_waves))) return rc;
        if ((rc = dev_alloc<uint32_t>(s->d_wide_counter, 4))) return rc;
        JTK_HIP_TRY(hipMemsetAsync(s->d_wide_counter.p, 0, 4 * sizeof(uint32_t), s->stream));
    }
    return 0;
}

int session_create_ex(const jtk_lc_params_t *params, size_t n_chunks, const jtk_lc_chunk_t *chunks,
                      const uint8_t *tmpl_bases, const uint8_t *read_bases, const uint64_t *read_off,
                      const uint8_t *ops, const uint64_t *ops_off, const uint8_t *strand,
                      uint32_t post_stride, int device, const ChunkExtra *extra, uint32_t ignore_edge,
                      jtk_lc_session_t **out, bool polish_only) {
    // ---- the arguments
    g_last_error.clear();
    if (!params || !out || (n_chunks && (!chunks || !tmpl_bases || !read_bases || !read_off || !ops || !ops_off || !strand)))
        return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (post_stride == 0) return jtk_fail(JTK_ERR_INVALID_ARG, "post_stride must be >= 1");
    if (params->gains.max_homopolymer_len == 0 || params->gains.max_homopolymer_len > JTK_GAINS_MAX_HOMOP)
        return jtk_fail(JTK_ERR_INVALID_ARG, "gains.max_homopolymer_len out of range");
    int rc = jtk_require_device(device);
    if (rc) return rc;

    // ---- the plan: host-side layout + validation, the chain's launches, the sweeps' waves (session_plan.h)
    BatchPlan bp;
    WavePlan wp;
    std::string msg;
    if ((rc = plan_batch(*params, n_chunks, chunks, read_off, ops_off, strand, post_stride, extra, polish_only, bp, msg)))
        return jtk_fail(rc, msg);
    // Templates (a few MB) are recoded here; the reads and their ops -- the bulk of a stage call's input -- cross the bus as the
    // caller holds them (stage_reads).
    std::vector<uint8_t> h_tmpl;
    if (!recode_templates(bp, chunks, tmpl_bases, h_tmpl)) return jtk_fail(JTK_ERR_INVALID_ARG, "non-ACGT base in a template");
    hipDeviceProp_t prop;
    JTK_HIP_TRY(hipGetDeviceProperties(&prop, device));
    SweepSizes sizes = {phmm_lds_bytes(bp.max_tmpl, bp.max_read), 0, 0, 0};
    if (!bp.pair_items.empty()) sizes.phmm_pair_lds_bytes = phmm_pair_lds_bytes(bp.max_tmpl, bp.max_read);
    if (bp.n_wide_reads) {
        sizes.phmm_wide_lds_bytes = phmm_wide_lds_bytes(bp.max_tmpl, bp.max_read, bp.max_wide_radius);
        sizes.phmm_wide_scratch_doubles = phmm_wide_scratch_doubles(bp.max_tmpl, bp.max_read, bp.max_wide_radius);
    }
    if ((rc = plan_waves((uint32_t)prop.multiProcessorCount, sizes, bp, wp, msg))) return jtk_fail(rc, msg);

    jtk_lc_session *s = new jtk_lc_session();
    std::unique_ptr<jtk_lc_session> guard(s);
    s->device = device;
    s->params = *params;
    s->post_stride = post_stride;
    s->n_chunks = (uint32_t)n_chunks;
    s->n_reads = (uint32_t)bp.n_reads;
    s->ignore_edge = ignore_edge;
    s->polish_only = polish_only;  // no variant search, no chain: none of their limits or workspaces apply
    s->h_chunks = std::move(bp.chunks);
    s->h_reads = std::move(bp.reads);
    s->h_state0 = std::move(bp.state0);
    s->h_copy0 = std::move(bp.copy0);
    s->has_split = bp.has_split;
    s->max_tmpl = bp.max_tmpl;
    s->max_read = bp.max_read;
    s->max_n = bp.max_n;
    s->max_copy = bp.max_copy;
    s->n_wide_reads = bp.n_wide_reads;
    s->max_wide_radius = bp.max_wide_radius;
    s->tmpl_bytes = h_tmpl.size();
    s->ops_bytes = bp.ops;
    for (int q = 0; q < 3; q++) s->chain_class[q] = bp.chain.cls[q];
    s->n_waves = wp.n_waves;
    s->n_pair_items = (uint32_t)bp.pair_items.size();
    s->n_pair_waves = wp.n_pair_waves;
    s->n_wide_waves = wp.n_wide_waves;
    s->wide_stride = wp.wide_stride;
    if (s->has_split) {  // the sub-problems of the split branch are encoded from these again
        s->h_read_bases.assign(read_bases, read_bases + read_off[bp.n_reads]);
        s->h_read_off.assign(read_off, read_off + bp.n_reads + 1);
        s->h_strand.assign(strand, strand + bp.n_reads);
    }

    // ---- device allocation + upload
    if ((rc = take_lane(s, !polish_only))) return rc;
    tstart(s, -1);
    const std::vector<jtk_lc_params_t> pv(1, *params);
    const std::vector<HmmDev> hv = {hmm_to_dev(params->forward), hmm_to_dev(params->reverse)};
    std::vector<uint64_t> h_rng;
    if ((rc = upload_batch(s, bp, pv, hv, h_tmpl))) return rc;
    if ((rc = stage_reads(s, bp.n_reads, read_bases, read_off, ops, ops_off, bp.raw))) return rc;
    if ((rc = alloc_polish_workspaces(s, bp))) return rc;
    if (!polish_only) {
        if ((rc = alloc_cluster_workspaces(s, bp))) return rc;
    }
    if (extra) {
        h_rng.resize(4 * n_chunks);
        for (size_t c = 0; c < n_chunks; c++) memcpy(&h_rng[4 * c], extra[c].rng, 32);
        if ((rc = dev_upload(s, s->d_rng, h_rng))) return rc;
        s->resume_rng = true;
    }
    if ((rc = acquire_stripes(s, wp.stripe_stride, wp.n_stripes, wp.n_waves))) return rc;
    if ((rc = upload_pair_and_wide(s, bp))) return rc;
    // set 0 = the batch as uploaded (never written), sets 1 / 2 = what the polish rounds write (batch_types.h DevBufs)
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
    if ((rc = session_wait(s))) return rc;
    float ms = 0;
    (void)hipEventElapsedTime(&ms, s->timers.back().a, s->timers.back().b);
    memset(&g_timing, 0, sizeof g_timing);
    g_timing.h2d_ms = ms;
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

// The chain launch of `n` sessions of one lane (LaneGather::arrive calls it, under the lane's mutex, from the thread of the
// member that found the lane gathered): per chain class one merged launch with a segment for every member that has chunks of
// the class.  The second stream only if every member uses it.  What the two launches were given -- read from the segment
// tables themselves, not from the members -- goes into the lane's ledger when the call returns.
static int launch_lane_chains(jtk_lc_session *const *members, int n) {
    LaneStreams &ls = device_lanes(members[0]->device).lane(members[0]->lane).streams;
    bool all_side = true;
    for (int i = 0; i < n; i++) all_side = all_side && members[i]->side;
    // The light chain behind the members' rounds and filters, on the stream that carried them (every member of a gather was
    // bound to the same one: the lane's round stream moves only here, and nobody is in a pass now); the general chain on the
    // other stream -- unless a light chain that some lane-mate has not left yet runs there (a member that left it and came
    // round alone): then one behind the other.
    hipStream_t main_stream = members[0]->stream, side = nullptr;
    int idx;
    {
        std::lock_guard<std::mutex> lock(ls.flow);
        idx = ls.side && main_stream == ls.side ? 1 : 0;
        hipStream_t two[2] = {ls.stream, ls.side};
        if (ls.side && ls.flights.general_on_other(idx, all_side)) side = two[1 - idx];
    }
    jtk_lc_debug_lane_launch_t rec;
    memset(&rec, 0, sizeof rec);
    rec.members = (uint32_t)n;
    struct Keep {  // (a launch that fails is recorded with what it was given, too)
        jtk_lc_session *s;
        const jtk_lc_debug_lane_launch_t &rec;
        ~Keep() {
            LaneLedger &lg = device_lanes(s->device).lane(s->lane).streams.ledger;
            std::lock_guard<std::mutex> lock(lg.m);
            lg.ring[lg.calls++ % JTK_LANE_LEDGER] = rec;
        }
    } keep{members[0], rec};
    McmcSegment seg[2][JTK_LANE_MAX_SEGMENTS];
    int owner[2][JTK_LANE_MAX_SEGMENTS], n_seg[2] = {0, 0};
    uint32_t workgroups[JTK_LANE_MAX_SEGMENTS] = {};
    for (int j = 0; j < 2; j++) {
        for (int i = 0; i < n; i++) {
            jtk_lc_session *s = members[i];
            const ChainClass &cc = s->chain_class[j];
            if (cc.count == 0) continue;
            // the class's own stretch of the split scratch: 2 + 2 * count words from 2 * first + 4 * j
            owner[j][n_seg[j]] = i;
            seg[j][n_seg[j]] = McmcSegment{cc.count, s->d_chunks.as<ChunkMeta>(), s->d_state.as<ChunkState>(), s->d_params.as<jtk_lc_params_t>(),
                                           s->d_feat.as<double>(), s->d_vtype.as<uint32_t>(), nullptr, 0, s->d_label.as<uint32_t>(),
                                           s->d_post.as<double>(), s->post_stride, s->d_lg.as<double>(), s->d_lg_off.as<uint64_t>(),
                                           cc.lds_n, cc.lds_d, cc.lds_k, nullptr, s->d_order.as<uint32_t>() + cc.first,
                                           s->d_chain_split.as<uint32_t>() + 2 * cc.first + 4 * j};
            workgroups[i] += mcmc_chain_workgroups(seg[j][n_seg[j]]);
            n_seg[j]++;
        }
    }
    // every member's completion: the counter's value once both classes' kernels have counted its workgroups, and this pass's id
    for (int i = 0; i < n; i++) {
        jtk_lc_session *s = members[i];
        s->flight.reset();
        s->may_leave = false;
        if (!workgroups[i] || !s->h_nactive) continue;   // (nothing counts, nothing reports)
        s->chain_done.advance(workgroups[i]);
        __atomic_store_n(s->h_nactive + JTK_PINNED_CHAIN_WORD, 0u, __ATOMIC_RELEASE);
    }
    for (int j = 0; j < 2; j++)
        for (int k = 0; k < n_seg[j]; k++) {
            jtk_lc_session *s = members[owner[j][k]];
            if (!s->h_nactive) continue;
            seg[j][k].done = s->d_counter.as<uint32_t>() + 2;
            seg[j][k].done_word = s->h_nactive_dev + JTK_PINNED_CHAIN_WORD;
            seg[j][k].done_target = s->chain_done.target;
            seg[j][k].done_pass = s->chain_done.pass;
        }
    for (int j = 0; j < 2; j++) {
        rec.segments[j] = (uint32_t)n_seg[j];
        for (int i = 0; i < n_seg[j]; i++) {
            rec.seg_chunks[j][i] = seg[j][i].n_chunks;
            rec.chunks[j] += seg[j][i].n_chunks;
        }
        if (n_seg[j] && launch_mcmc_merged(main_stream, n_seg[j], seg[j], side, members[0]->ev_chain[0], members[0]->ev_chain[1]) != 0)
            return -1;
    }
    // More than one member, and a second stream for whoever leaves first: the members that may (lane_member_may_leave: not
    // those with a global-memory chain still to queue behind this launch) wait for their own words (run_batch), and the other
    // stream is the lane's round stream from here on, until every member's pass is over.
    bool may_fly = false;
    if (n > 1 && ls.side) {
        std::lock_guard<std::mutex> lock(ls.flow);
        may_fly = ls.flights.may_fly();  // (not while a lane-mate still waits in an earlier merged launch: LaneFlow)
    }
    if (may_fly) {
        auto f = std::make_shared<ChainFlight>();
        if (hipEventCreateWithFlags(&f->end, hipEventDisableTiming) != hipSuccess || hipEventRecord(f->end, main_stream) != hipSuccess)
            return 0;  // (nobody leaves early: every member waits for its own event, as a lone one does)
        f->members = n;
        f->light_stream = idx;
        for (int i = 0; i < n; i++) {
            members[i]->flight = f;
            members[i]->may_leave = lane_member_may_leave(workgroups[i], members[i]->h_nactive != nullptr, members[i]->chain_class[2].count);
        }
        f->waiting.store(n);
        std::lock_guard<std::mutex> lock(ls.flow);
        ls.flights.launched(f);
    }
    return 0;
}
static_assert(JTK_LANE_MAX_SEGMENTS <= JTK_MCMC_MAX_SEGMENTS, "a lane's launch must fit the kernels' segment table");

// include/jtk_lc_debug.h: the lane of a session, a hold on a lane's gather, and what the lane has launched
static DeviceLanes::Lane *existing_lane(int device, int lane) {
    DeviceLanes *t = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_lanes_mutex);
        auto it = g_lanes.find(device);
        if (it != g_lanes.end()) t = it->second;
    }
    if (!t || lane < 0 || lane >= t->size()) return nullptr;
    return &t->lane(lane);
}
int jtk_lc_debug_session_lane(jtk_lc_session_t *s) {
    g_last_error.clear();
    if (!s) return jtk_fail(JTK_ERR_INVALID_ARG, "null session");
    if (s->lane < 0) return jtk_fail(JTK_ERR_INVALID_ARG, "the session has no lane");
    return s->lane;
}
int jtk_lc_debug_lane_hold(int device, int lane, int hold) {
    g_last_error.clear();
    DeviceLanes::Lane *L = existing_lane(device, lane);
    if (!L) return jtk_fail(JTK_ERR_INVALID_ARG, "jtk_lc_debug_lane_hold: device " + std::to_string(device) + " has no lane " + std::to_string(lane));
    LaneLedger &lg = L->streams.ledger;
    {
        std::lock_guard<std::mutex> lock(lg.m);
        if (!hold && lg.holds == 0) return jtk_fail(JTK_ERR_INVALID_ARG, "jtk_lc_debug_lane_hold: release of a lane that is not held");
        lg.holds += hold ? 1 : -1;
    }
    if (hold) L->gather.enter();
    else L->gather.withdraw();
    return JTK_OK;
}
int jtk_lc_debug_lane_state(int device, int lane, jtk_lc_debug_lane_state_t *out) {
    g_last_error.clear();
    DeviceLanes::Lane *L = existing_lane(device, lane);
    if (!L || !out) return jtk_fail(JTK_ERR_INVALID_ARG, "jtk_lc_debug_lane_state: no such lane, or a null pointer");
    LaneLedger &lg = L->streams.ledger;
    // The member counts are the gather's, the class records the ledger's; both advance inside one call of the launch, under
    // the gather's mutex.  A launch between the two reads shows as different call counts: read again.
    for (int attempt = 0; attempt < 16; attempt++) {
        memset(out, 0, sizeof *out);
        int members[JTK_LANE_LEDGER], in_pass = 0, pending = 0;
        unsigned long long calls = 0;
        const int have = L->gather.recent(members, &in_pass, &pending, &calls);
        std::lock_guard<std::mutex> lock(lg.m);
        if (lg.calls != calls) continue;
        out->holds = (uint32_t)lg.holds;
        out->in_pass = (uint32_t)std::max(0, in_pass - lg.holds);
        out->pending = (uint32_t)pending;
        out->launch_calls = calls;
        out->n_records = (uint32_t)have;
        for (int i = 0; i < have; i++) {
            out->records[i] = lg.ring[(calls - have + i) % JTK_LANE_LEDGER];
            if (out->records[i].members != (uint32_t)members[i]) return jtk_fail(JTK_ERR_INTERNAL, "the lane's ledger and its gather disagree");
        }
        return JTK_OK;
    }
    return jtk_fail(JTK_ERR_INTERNAL, "jtk_lc_debug_lane_state: the lane kept launching; read it while it is held or idle");
}

// include/jtk_lc_debug.h: a hold on a lane's round gather, and what the lane's round launches carried
int jtk_lc_debug_round_hold(int device, int lane, int hold) {
    g_last_error.clear();
    DeviceLanes::Lane *L = existing_lane(device, lane);
    if (!L || hold < 0 || hold > 2)
        return jtk_fail(JTK_ERR_INVALID_ARG, "jtk_lc_debug_round_hold: device " + std::to_string(device) + " has no lane " + std::to_string(lane) + ", or an unknown request");
    if (hold == 1) L->rounds.hold();
    else if (hold == 2) L->rounds.step();
    else if (!L->rounds.release()) return jtk_fail(JTK_ERR_INVALID_ARG, "jtk_lc_debug_round_hold: release of a lane that is not held");
    return JTK_OK;
}
int jtk_lc_debug_round_state(int device, int lane, jtk_lc_debug_round_state_t *out) {
    g_last_error.clear();
    DeviceLanes::Lane *L = existing_lane(device, lane);
    if (!L || !out) return jtk_fail(JTK_ERR_INVALID_ARG, "jtk_lc_debug_round_state: no such lane, or a null pointer");
    memset(out, 0, sizeof *out);
    int members[JTK_LANE_LEDGER], in_rounds = 0, parked = 0, holds = 0;
    (void)L->rounds.recent(members, &in_rounds, &parked, nullptr, &holds);
    out->in_rounds = (uint32_t)in_rounds;
    out->parked = (uint32_t)parked;
    out->holds = (uint32_t)holds;
    RoundLedger &lg = L->streams.round_ledger;
    std::lock_guard<std::mutex> lock(lg.m);
    out->launch_calls = lg.calls;
    const unsigned long long have = std::min<unsigned long long>(lg.calls, JTK_LC_DEBUG_ROUND_RECORDS);
    out->n_records = (uint32_t)have;
    for (unsigned long long i = 0; i < have; i++) out->records[i] = lg.ring[(lg.calls - have + i) % JTK_LC_DEBUG_ROUND_RECORDS];
    return JTK_OK;
}

// ---- the polish rounds of a pass: one table of segments per launch, a lone session's included

// A session's step as a segment of the round kernels' table (device_common.h: RoundSegment) -- the opening of its pass (every
// chunk back to the batch as uploaded: buffer set 0 is never written, so there is nothing to copy; the per-round counters to
// zero; then the bands of every read) or polish round rq.round.
RoundSegment round_segment(const jtk_lc_session *s, const jtk_lc_session::RoundRequest &rq) {
    RoundSegment g;
    memset(&g, 0, sizeof g);
    g.n_chunks = s->n_chunks;
    g.n_reads = s->n_reads;
    g.reads = s->d_reads.as<ReadMeta>();
    g.chunks = s->d_chunks.as<ChunkMeta>();
    g.state = s->d_state.as<ChunkState>();
    g.state0 = s->d_state0.as<ChunkState>();
    g.bufs = s->bufs;
    g.ey = s->d_ey.as<uint8_t>();
    g.delta = s->d_delta.as<uint64_t>();
    g.hmm2 = s->d_hmm2.as<HmmDev>();
    g.raw = s->d_raw.as<double>();
    g.rawG = s->d_rawG.as<int>();
    g.lk = s->d_lk.as<double>();
    g.total = s->d_total.as<double>();
    g.edits = s->d_edits.as<Edit>();
    g.new_len = s->d_newlen.as<uint32_t>();
    g.n_active = s->d_nactive.as<uint32_t>();
    g.n_active_host = s->h_nactive_dev;  // commit_kernel stores the round's count there itself (mapped pinned memory)
    g.max_tmpl = s->max_tmpl;
    g.max_read = s->max_read;
    g.n_waves = s->n_waves;
    g.open = rq.open ? 1u : 0u;
    g.round = (uint32_t)rq.round;
    g.ignore_edge = s->ignore_edge;
    g.skip_le_radius = s->n_pair_items ? JTK_PAIR_MAX_RADIUS : 0;  // phmm_pair_kernel's chunks (such a session never shares a table)
    g.only_active = rq.only_active;
    g.final_pass = rq.final_pass;
    return g;
}

// a timed stretch of a round launch: one event pair on the stream, shared by the members it is booked to
struct SharedPair {
    hipEvent_t a = nullptr, b = nullptr;
    ~SharedPair() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
};
static std::shared_ptr<SharedPair> pair_start(hipStream_t st) {  // null: an event could not be made or recorded
    auto p = std::make_shared<SharedPair>();
    if (hipEventCreate(&p->a) != hipSuccess || hipEventCreate(&p->b) != hipSuccess || hipEventRecord(p->a, st) != hipSuccess) return nullptr;
    return p;
}
static void pair_book(jtk_lc_session *s, int kind, const std::shared_ptr<SharedPair> &p) {
    KernelTimer t;
    t.a = p->a;
    t.b = p->b;
    t.kind = kind;
    t.shared = p;
    s->timers.push_back(t);
}

// The round_request of `n` >= 1 sessions that share a stream, as one table and one launch per kernel: one segment per member,
// whatever step each is at.  The phmm / polish event pairs are the launch's, booked to every member they cover
// (kernel_launches counts a launch once per member it carried), and every member's own round event is recorded behind the
// sequence.  `lane`: the launch comes through the lane's round gather (under its mutex) -- the tickets are the lane's and what
// was launched goes into the lane's round ledger, read back from the table; otherwise the one member's own tickets, no record.
// Three kernels are outside the table and are queued for a table of ONE only, the sessions that need them never gather
// (run_batch): phmm_pair_kernel (its chunks are the segment's skip_le_radius), phmm_wide_kernel, and finalize_kernel where the
// per-read tables are the product (batch_needs_tables) -- the final pass's instead of sum_final, a clustering pass's after the
// round for the chunks that converged in it.
static int launch_round_table(jtk_lc_session *const *members, int n, LaneStreams *lane) {
    jtk_lc_session *m0 = members[0];  // the stream is every member's; for n == 1 the lone member, whose extras are queued below
    hipStream_t st = m0->stream;
    RoundSegTable t;
    memset(&t, 0, sizeof t);
    t.n = (uint32_t)n;
    bool any_open = false, any_round = false;
    uint32_t n_waves = 0;
    const StripePool *stripes = nullptr;
    for (int i = 0; i < n; i++) {
        const jtk_lc_session *m = members[i];
        t.seg[i] = round_segment(m, m->round_request);
        if (t.seg[i].open) {
            any_open = true;
            continue;
        }
        any_round = true;
        n_waves = std::max(n_waves, m->n_waves);
        // the forward scratch: the members' set with the longest stripes serves every segment
        const StripePool *sp = m->stripes.get();
        if (!stripes || sp->stride > stripes->stride || (sp->stride == stripes->stride && sp->n > stripes->n)) stripes = sp;
    }
    if (lane) {
        RoundLaunchInfo info;
        round_table_info(t, &info);
        jtk_lc_debug_round_launch_t rec;
        memset(&rec, 0, sizeof rec);
        rec.members = info.segments;
        rec.merged = n > 1;
        for (int i = 0; i < JTK_ROUND_MAX_SEGMENTS; i++) {
            rec.round[i] = info.round[i];
            rec.chunks[i] = info.chunks[i];
            rec.phmm_items[i] = info.phmm_items[i];
        }
        std::lock_guard<std::mutex> lock(lane->round_ledger.m);
        lane->round_ledger.ring[lane->round_ledger.calls++ % JTK_LC_DEBUG_ROUND_RECORDS] = rec;
    }
    const jtk_lc_session::RoundRequest &rq0 = m0->round_request;  // read only where lone_round holds: the lone member's step
    const bool lone_round = n == 1 && any_round, need_tables = batch_needs_tables(m0->polish_only, m0->max_n);
    const ReadMeta *reads = m0->d_reads.as<ReadMeta>();
    const ChunkMeta *chunks = m0->d_chunks.as<ChunkMeta>();
    const ChunkState *state = m0->d_state.as<ChunkState>();
    const HmmDev *hmm2 = m0->d_hmm2.as<HmmDev>();
    auto timed = [&](int kind, bool rounds_only, auto &&launches) -> int {
        auto p = pair_start(st);
        if (!p) return jtk_fail(JTK_ERR_INTERNAL, "hipEventCreate / hipEventRecord failed for a round launch");
        launches();
        JTK_HIP_TRY(hipEventRecord(p->b, st));
        for (int i = 0; i < n; i++)
            if (!rounds_only || !t.seg[i].open) pair_book(members[i], kind, p);
        return 0;
    };
    // A polish round needs the column totals of the active chunks, not their per-read tables: the totals come straight from
    // the row sums (sum_final_kernel).  Round 6: the variant filter takes its column statistics and the picked columns' entries
    // from the row sums too (column_filter_fused_kernel, filter_kernels.hip), so a clustering pass never materialises the
    // N x 14(L+1) table -- finalize_kernel runs only where the table itself is the product (window polishing's final pass;
    // the modification-table entry point has its own) or where a pile-up is too deep for the fused filter.
    auto sweeps_and_totals = [&] {
        launch_phmm(st, t, stripes->set(), std::min(n_waves, stripes->n), lane ? lane->d_round_counter : m0->d_counter.as<uint32_t>(),
                    lane ? &lane->tk_round : &m0->tk_phmm);  // (the cap binds only when sets differ: a lone session's waves fit its own set)
        if (lone_round && m0->n_pair_items)
            launch_phmm_pair(st, m0->n_pair_items, m0->d_pair_items.as<uint32_t>(), reads, chunks, state, m0->bufs,
                             m0->d_ey.as<uint8_t>(), m0->d_delta.as<uint64_t>(), hmm2, m0->stripes->set(), m0->n_pair_waves,
                             m0->d_counter.as<uint32_t>() + 1, &m0->tk_pair, m0->d_raw.as<double>(), m0->d_rawG.as<int>(),
                             m0->d_lk.as<double>(), m0->max_tmpl, m0->max_read, rq0.only_active);
        if (lone_round && m0->n_wide_reads)
            launch_phmm_wide(st, m0->n_reads, reads, chunks, state, m0->bufs, m0->d_ey.as<uint8_t>(), m0->d_delta.as<uint64_t>(),
                             hmm2, m0->d_wide_scratch.as<double>(), m0->wide_stride, m0->n_wide_waves,
                             m0->d_wide_counter.as<uint32_t>(), &m0->tk_wide, m0->d_raw.as<double>(), m0->d_rawG.as<int>(),
                             m0->d_lk.as<double>(), m0->max_tmpl, m0->max_read, rq0.only_active, m0->max_wide_radius);
        launch_sum_final(st, t);  // (not of a final pass)
        if (lone_round && rq0.final_pass && need_tables)  // the last pass materialises the tables of whatever is still active
            launch_finalize(st, m0->n_reads, reads, chunks, state, hmm2, m0->d_raw.as<double>(), m0->d_rawG.as<int>(),
                            m0->d_lk.as<double>(), m0->max_tmpl, rq0.only_active);
    };
    auto edits_and_bands = [&] {
        if (any_round) launch_polish_round(st, t);
        launch_band_prep(st, t);
    };
    // the chunks that converged in this round -- no edit selected -- get their tables, once, from the row sums they still hold
    auto converged_tables = [&] {
        launch_finalize(st, m0->n_reads, reads, chunks, state, hmm2, m0->d_raw.as<double>(), m0->d_rawG.as<int>(), m0->d_lk.as<double>(),
                        m0->max_tmpl, 0, rq0.round);
    };
    int rc;
    if (any_open) launch_reset_pass(st, t);
    if (any_round && (rc = timed(JTK_K_PHMM, true, sweeps_and_totals))) return rc;
    if ((rc = timed(JTK_K_POLISH, false, edits_and_bands))) return rc;
    if (lone_round && !rq0.final_pass && !m0->polish_only && need_tables && (rc = timed(JTK_K_PHMM, true, converged_tables))) return rc;
    for (int i = 0; i < n; i++) {
        const jtk_lc_session::RoundRequest &q = members[i]->round_request;
        if (!q.open && !q.final_pass) JTK_HIP_TRY(hipEventRecord(members[i]->ev_round[q.round & 1], st));
    }
    return 0;
}

// The round launch of `n` sessions of one lane (RoundGather::arrive calls it, under the gather's mutex, from the thread of
// the member that found the lane's rounds gathered).
static int launch_lane_rounds(jtk_lc_session *const *members, int n) {
    LaneStreams *lane = &device_lanes(members[0]->device).lane(members[0]->lane).streams;
    uint64_t chunk_rows = 0;
    for (int i = 0; i < n; i++) chunk_rows += members[i]->n_chunks;
    int rc = 0;
    if (chunk_rows > 65535u)  // (sum_final's grid has the chunks of all members in one dimension): each as its own table of one
        for (int i = 0; i < n && !rc; i++) rc = launch_round_table(members + i, 1, lane);
    else
        rc = launch_round_table(members, n, lane);
    // the launch runs on ONE member's thread and g_last_error is per thread: a failure's text is left with every member it
    // carried, and each puts it into its own thread's g_last_error when arrive() returns (run_batch)
    for (int i = 0; i < n; i++) members[i]->round_error = rc ? g_last_error : std::string();
    return rc;
}

// Lane-mates' rounds go out in one launch per kernel unless JTK_LC_MERGE_ROUNDS=0 (read at every pass).
static bool merge_rounds_enabled() {
    const char *e = getenv("JTK_LC_MERGE_ROUNDS");
    return !e || atoi(e) != 0;
}

// one pass of the kernel sequence over the resident batch
int run_batch(jtk_lc_session_t *s, int skip_polish) {
    JTK_HIP_TRY(hipSetDevice(s->device));
    // From here to its chain launch the session is "in its pass" for the sessions it shares a lane with: they hold their
    // chains back until it arrives or leaves (any return below).  A session that resumes RNG streams (a sub-problem of the
    // split branch) launches alone, as does one that has no chain at all.
    LanePass<jtk_lc_session> pass(!s->polish_only && !s->resume_rng ? s->gather : nullptr);
    // The pass's streams (session_lanes.h: the stream rule).  After enter(): no merged launch of the lane, and so no change of
    // its round stream, can come before this session's own chain point.
    const auto host_t0 = std::chrono::steady_clock::now();
    const int round_idx = s->lane >= 0 ? bind_lane_streams(s, s->side != nullptr) : 0;
    {
        std::lock_guard<std::mutex> lock(s->pass_log_mutex);
        s->n_passes++;
        jtk_lc_debug_pass_t &pr = pass_record(s);
        memset(&pr, 0, sizeof pr);
        pr.pass = s->n_passes;
        pr.round_stream = pr.next_round_stream = (uint32_t)round_idx;
    }
    const double h2d = g_timing.h2d_ms;
    memset(&g_timing, 0, sizeof g_timing);
    g_timing.h2d_ms = h2d;
    timers_clear(s->timers);
    hipStream_t st = s->stream;
    const ReadMeta *reads = s->d_reads.as<ReadMeta>();
    const ChunkMeta *chunks = s->d_chunks.as<ChunkMeta>();
    ChunkState *state = s->d_state.as<ChunkState>();
    const HmmDev *hmm2 = s->d_hmm2.as<HmmDev>();
    auto host_launched = host_t0;
    hipEvent_t ev0, ev1;
    JTK_HIP_TRY(hipEventCreate(&ev0));
    JTK_HIP_TRY(hipEventCreate(&ev1));
    JTK_HIP_TRY(hipEventRecord(ev0, st));
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
    // The rounds go through the lane's round gather (session_lanes.h): lane-mates that are in their polish phase at the same
    // time get one launch per kernel for all of them; a session that is alone there goes out as a table of one.  Sessions
    // whose rounds hold kernels the segment tables do not cover never park there and queue their own tables of one: pair
    // items, wide reads, per-read tables, and the passes that enter no chain gather either.
    const bool gathers = pass.g && s->rounds && !skip_polish && !s->n_pair_items && !s->n_wide_reads &&
                         !batch_needs_tables(s->polish_only, s->max_n) && merge_rounds_enabled();
    RoundPass<jtk_lc_session> rounds(gathers ? s->rounds : nullptr);
    auto queue = [&](int open, int round, int only_active, int final_pass) -> int {
        s->round_request.open = open;
        s->round_request.round = round;
        s->round_request.only_active = only_active;
        s->round_request.final_pass = final_pass;
        if (!rounds.g) return launch_round_table(&s, 1, nullptr);
        const int arc = rounds.g->arrive(s, launch_lane_rounds);
        if (arc) g_last_error = s->round_error;   // (the launch may have run on a lane-mate's thread)
        return arc;
    };
    int rc = queue(1, 0, 0, 0);
    if (rc) return rc;
    const bool need_tables = batch_needs_tables(s->polish_only, s->max_n);
    const int max_rounds = skip_polish ? 1 : JTK_POLISH_MAX_ROUNDS + 1;
    for (int round = 0; round < max_rounds; round++) {
        const int only_active = round > 0;
        const int final_pass = skip_polish || round == JTK_POLISH_MAX_ROUNDS;
        if ((rc = queue(0, round, only_active, final_pass))) return rc;
        if (final_pass) break;
        if (round >= 1) {
            JTK_HIP_TRY(hipEventSynchronize(s->ev_round[(round - 1) & 1]));
            if (round == 1) {
                std::lock_guard<std::mutex> lock(s->pass_log_mutex);
                pass_record(s).stamp_round0 = order_stamp();
            }
            if (s->h_nactive[round - 1] == 0) break;  // round `round` was already queued and finds nothing to do
        }
    }
    rounds.leave();  // before the chain point: the lane-mates' rounds do not wait for this session any more
    // the merged launch this pass may leave through its word (launch_lane_chains gives it); every way out of this function
    // takes the session out of it
    std::shared_ptr<ChainFlight> flight;
    LaneFlightLeave leaving(nullptr);
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
        if (pass.g) {  // with the lane's other sessions, or at once if none is in a pass
            mcmc_rc = pass.arrive(s, launch_lane_chains);
            flight = s->flight;
            leaving.f = flight.get();
        }
        for (int j = 0; j < 2 && !pass.g; j++) {
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
        host_launched = std::chrono::steady_clock::now();
        if (mcmc_rc != 0) {
            s->flight.reset();
            (void)session_wait(s);
            return jtk_fail(JTK_ERR_INTERNAL, "the chain kernel could not be launched (jump table upload failed)");
        }
        s->ran = true;
        s->ran_fused = !need_tables;
    }  // !polish_only
    JTK_HIP_TRY(hipEventRecord(ev1, st));
    // A merged launch of several lane-mates (s->flight): the session waits for its OWN chunks -- the word of its pinned page
    // that the chain kernels write when the last workgroup of its segments has counted -- asleep between looks, with the
    // launch's end event as the fallback, and leaves while the launch still runs for its mates.  Otherwise, and where the word
    // does not move, the event: the session's last kernel, not the stream.
    int how = JTK_LEAVE_EVENT;
    jtk_lc_debug_pass_t left;
    memset(&left, 0, sizeof left);
    left.members = 1;
    if (flight && s->may_leave) {
        const uint32_t *word = s->h_nactive + JTK_PINNED_CHAIN_WORD;
        const uint32_t id = s->chain_done.pass;
        how = lane_leave_wait([&] { return __atomic_load_n(word, __ATOMIC_ACQUIRE) == id; },
                              [&] {
                                  const hipError_t e = hipEventQuery(flight->end);
                                  return e == hipSuccess ? 1 : (e == hipErrorNotReady ? 0 : -1);
                              },
                              [] { std::this_thread::sleep_for(std::chrono::microseconds(100)); });
        left.event_pending = hipEventQuery(flight->end) == hipErrorNotReady;
        (void)hipGetLastError();  // ("not ready" is an answer, not a failure of the pass)
    }
    const auto host_left = std::chrono::steady_clock::now();
    if (how == JTK_LEAVE_ERROR) {
        (void)hipEventDestroy(ev0);
        (void)hipEventDestroy(ev1);
        return jtk_fail(JTK_ERR_INTERNAL, "the chain launch's end event failed and the session's completion word did not move");
    }
    if (how == JTK_LEAVE_EVENT) {
        JTK_HIP_TRY(hipEventSynchronize(ev1));
        JTK_HIP_TRY(hipGetLastError());
    }
    if (flight) {
        left.members = (uint32_t)flight->members;
        left.still_waiting = (uint32_t)leaving.leave();
        if (how != JTK_LEAVE_WORD) s->flight.reset();  // (nothing of the launch runs on: ev1 is behind all of it)
    }
    left.how = how == JTK_LEAVE_WORD ? JTK_LC_DEBUG_LEFT_BY_WORD : JTK_LC_DEBUG_LEFT_BY_EVENT;
    left.stamp_left = order_stamp();
    // from here on the session's work goes to the stream the launch it left does not run on
    left.next_round_stream = s->lane >= 0 && how == JTK_LEAVE_WORD ? (uint32_t)bind_lane_streams(s, s->side != nullptr) : (uint32_t)round_idx;
    // The times.  hipEventElapsedTime needs two completed events: a pass that left through its word takes total_ms and the
    // chain family's figure from the host clock (the call's start, and the return of the chain launch, to the moment the word
    // was seen); every other figure is an event pair that precedes the session's chain on its stream.
    const auto host_ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
        return std::chrono::duration<double, std::milli>(b - a).count();
    };
    float ms = 0;
    if (how == JTK_LEAVE_EVENT) (void)hipEventElapsedTime(&ms, ev0, ev1);
    g_timing.total_ms = how == JTK_LEAVE_EVENT ? (double)ms : host_ms(host_t0, host_left);
    for (int j = 0; j < 2; j++) g_timing.chain_lds_bytes[j] = s->chain_class[j].count ? s->chain_class[j].lds_bytes : 0;
    (void)hipEventDestroy(ev0);
    (void)hipEventDestroy(ev1);
    for (auto &t : s->timers) {
        if (t.kind < 0 || t.kind >= JTK_K_COUNT) continue;
        float k = 0;
        if (how == JTK_LEAVE_WORD && t.kind == JTK_K_MCMC) k = (float)host_ms(host_launched, host_left);
        else (void)hipEventElapsedTime(&k, t.a, t.b);
        g_timing.kernel_ms[t.kind] += k;
        g_timing.kernel_launches[t.kind] += 1;
    }
    {
        std::lock_guard<std::mutex> lock(s->pass_log_mutex);
        jtk_lc_debug_pass_t &pr = pass_record(s);
        pr.how = left.how;
        pr.event_pending = left.event_pending;
        pr.members = left.members;
        pr.still_waiting = left.still_waiting;
        pr.next_round_stream = left.next_round_stream;
        pr.stamp_left = left.stamp_left;
        pr.stamp_returned = order_stamp();
    }
    return 0;
}

int jtk_lc_debug_session_passes(jtk_lc_session_t *s, jtk_lc_debug_pass_t *out, size_t cap) {
    g_last_error.clear();
    if (!s || (!out && cap)) return jtk_fail(JTK_ERR_INVALID_ARG, "jtk_lc_debug_session_passes: null argument");
    std::lock_guard<std::mutex> lock(s->pass_log_mutex);
    const uint64_t have = std::min<uint64_t>(std::min<uint64_t>(s->n_passes, JTK_LC_DEBUG_PASS_RECORDS), cap);
    for (uint64_t i = 0; i < have; i++) out[i] = s->pass_log[(s->n_passes - have + 1 + i) % JTK_LC_DEBUG_PASS_RECORDS];
    return (int)have;
}

int jtk_lc_session_run(jtk_lc_session_t *s, int skip_polish) {
    g_last_error.clear();
    if (!s) return jtk_fail(JTK_ERR_INVALID_ARG, "null session");
    int rc = run_batch(s, skip_polish);
    if (rc == 0 && s->has_split) rc = run_split(s);
    return rc;
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
    if (int rc = session_wait(s)) return rc;
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
    JTK_HIP_TRY(hipEventSynchronize(ev1));
    JTK_HIP_TRY(hipGetLastError());
    float ms = 0;
    (void)hipEventElapsedTime(&ms, pl.ev0, ev1);
    g_timing.d2h_ms = ms;
    (void)hipEventDestroy(pl.ev0);
    (void)hipEventDestroy(ev1);
    pl.ev0 = nullptr;
    if (s->n_passes) {
        std::lock_guard<std::mutex> lock(s->pass_log_mutex);
        pass_record(s).stamp_fetched = order_stamp();
    }
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
