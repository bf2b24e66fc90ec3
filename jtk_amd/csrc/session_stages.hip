// session_stages.hip -- the one-shot stage entry points of include/jtk_lc.h: a batch cut into slices that run side by side as
// independent sessions (run_once), dealt to several GPUs (jtk_lc_cluster_chunks_multi), and window polishing.
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>

#include "session_internal.h"

// what a slice / a device's share measured, added to the call's record: the parts run side by side
static void timing_accumulate(jtk_lc_timing_t &into, const jtk_lc_timing_t &part) {
    into.h2d_ms += part.h2d_ms;
    into.d2h_ms += part.d2h_ms;
    into.total_ms = std::max(into.total_ms, part.total_ms);
    for (int j = 0; j < 2; j++) into.chain_lds_bytes[j] = std::max(into.chain_lds_bytes[j], part.chain_lds_bytes[j]);
    for (int k = 0; k < JTK_K_COUNT; k++) {
        into.kernel_ms[k] += part.kernel_ms[k];
        into.kernel_launches[k] += part.kernel_launches[k];
    }
}

static int run_slice(const jtk_lc_params_t *params, size_t n_chunks, const jtk_lc_chunk_t *chunks,
                     const uint8_t *tmpl_bases, const uint8_t *read_bases, const uint64_t *read_off, const uint8_t *ops,
                     const uint64_t *ops_off, const uint8_t *strand, int skip_polish, uint32_t *label, double *log_post,
                     uint32_t post_stride, jtk_lc_result_t *result, uint8_t *cons_out, uint64_t *cons_off,
                     uint64_t cons_cap, uint8_t *ops_out, uint64_t *ops_out_off, uint64_t ops_cap, int device) {
    jtk_lc_session_t *s = nullptr;
    int rc = jtk_lc_session_create(params, n_chunks, chunks, tmpl_bases, read_bases, read_off, ops, ops_off, strand,
                                   post_stride, device, &s);
    if (rc) return rc;
    rc = jtk_lc_session_run(s, skip_polish);
    if (rc == 0)
        rc = jtk_lc_session_fetch(s, label, log_post, result, cons_out, cons_off, cons_cap, ops_out, ops_out_off, ops_cap);
    const std::string keep = g_last_error;
    jtk_lc_session_destroy(s);
    g_last_error = keep;
    return rc;
}

// The one-shot entry points on a large batch: up to four slices of the batch run as independent sessions on their own streams
// and host threads, so that one slice's pair-HMM passes fill the CUs another slice's chain kernel leaves idle during
// its tail (the overlap bench.py gets from four resident batches, §6 of DESIGN.md).  Chunks are independent (the RNG
// is seeded per chunk), so the results do not depend on the slicing.  A slice keeps >= 500 chunks: below that the
// tail of its own chain kernel is all there is to hide.  JTK_LC_SLICES overrides the count (tests, tuning).
static int run_once(const jtk_lc_params_t *params, size_t n_chunks, const jtk_lc_chunk_t *chunks,
                    const uint8_t *tmpl_bases, const uint8_t *read_bases, const uint64_t *read_off, const uint8_t *ops,
                    const uint64_t *ops_off, const uint8_t *strand, int skip_polish, uint32_t *label, double *log_post,
                    uint32_t post_stride, jtk_lc_result_t *result, uint8_t *cons_out, uint64_t *cons_off,
                    uint64_t cons_cap, uint8_t *ops_out, uint64_t *ops_out_off, uint64_t ops_cap, const int *devices,
                    size_t n_devices) {
    // several devices: the same slicing, consecutive slices dealt to consecutive devices (a device's slices overlap
    // each other as on one GPU; devices share nothing)
    if (!devices || n_devices == 0) return jtk_fail(JTK_ERR_INVALID_ARG, "no device given");
    size_t per_dev = std::min<size_t>(4, n_chunks / n_devices / 500);  // 2500 chunks: 2.08 / 1.80 / 2.08 / 2.17 s in 3 / 4 / 5 / 6 slices
    if (const char *e = getenv("JTK_LC_SLICES")) per_dev = (size_t)atoi(e);
    if (per_dev < 1) per_dev = 1;
    // per_dev slices of a device run side by side.  A batch whose workspaces do not fit beside each other that way (deep
    // pile-ups: 296 KB of row sums / tables per read of a 2 kbp chunk) is cut into MORE slices, which the per_dev worker threads
    // of the device take one after the other: the workspace in use stays bounded by what per_dev slices need, and the
    // blocks a finished slice returns to the pool are what the next one takes.
    size_t slices_per_dev = per_dev;
    if (chunks && n_chunks) {
        uint64_t est = 0, max_len = 0, max_rd = 0;
        for (size_t c = 0; c < n_chunks; c++) {
            const uint64_t cap = chunks[c].tmpl_len + chunks[c].tmpl_len / 8 + 64;
            est += (uint64_t)chunks[c].n_reads * (cap + 1) * (JTK_ACC_N * 8 + 16);  // row sums / tables + ops / deltas
            max_len = std::max<uint64_t>(max_len, cap);
            if (read_off) {
                const uint64_t r0 = chunks[c].read_first, r1 = r0 + chunks[c].n_reads;
                if (r1 > r0) max_rd = std::max<uint64_t>(max_rd, (read_off[r1] - read_off[r0]) / (r1 - r0) + 64);
            }
        }
        size_t free_b = 0, total_b = 0;
        int cur = 0;
        (void)hipGetDevice(&cur);
        if (hipSetDevice(devices[0]) == hipSuccess && hipMemGetInfo(&free_b, &total_b) == hipSuccess && total_b > 0) {
            const uint64_t stripes = 4096ull * (max_len + max_rd + 32) * 64 * 16;   // the device's shared pair-HMM stripe set
            const double budget = (0.80 * (double)total_b - (double)stripes) / (double)per_dev;  // pooled blocks count as free
            if (budget > 0) {
                const size_t need = (size_t)std::ceil((double)est / (double)n_devices / budget);
                if (need > slices_per_dev) slices_per_dev = need;
            }
        }
        (void)hipSetDevice(cur);
    }
    size_t n_slices = slices_per_dev * n_devices;
    if (n_slices > n_chunks) n_slices = n_chunks;
    if (n_slices < 2 || !params || !chunks || !read_off || !ops_off || !label || !log_post || !result)
        return run_slice(params, n_chunks, chunks, tmpl_bases, read_bases, read_off, ops, ops_off, strand, skip_polish, label,
                         log_post, post_stride, result, cons_out, cons_off, cons_cap, ops_out, ops_out_off, ops_cap, devices[0]);
    g_last_error.clear();
    uint64_t n_reads = 0;
    if (int bad = check_contiguous(chunks, n_chunks, &n_reads)) return bad;
    // slice boundaries: equal shares of the reads
    std::vector<size_t> first(n_slices + 1, n_chunks);
    first[0] = 0;
    {
        size_t sl = 1;
        uint64_t seen = 0;
        for (size_t c = 0; c < n_chunks && sl < n_slices; c++) {
            seen += chunks[c].n_reads;
            if (seen * n_slices >= n_reads * sl) first[sl++] = c + 1;
        }
    }
    const bool want_cons = cons_out && cons_off, want_ops = ops_out && ops_out_off;
    // Every slice writes its results straight into the caller's arrays.  Where a slice's consensus / ops start depends on the
    // lengths of the slices before it: a slice learns its own lengths (fetch_begin), waits for its predecessor to publish where it
    // ends, publishes its own end and only then packs and copies (fetch_finish) -- no per-slice staging vectors, no stitching pass.
    struct Slice {
        std::vector<jtk_lc_chunk_t> chunks;
        int rc = 0;
        std::string error;
        jtk_lc_timing_t timing;
    };
    std::vector<Slice> slices(n_slices);
    std::vector<std::function<void()>> jobs(n_slices);
    std::mutex base_mutex;
    std::condition_variable base_cv;
    std::vector<uint64_t> cons_base(n_slices + 1, 0), ops_base(n_slices + 1, 0);
    std::vector<char> base_known(n_slices + 1, 0);
    base_known[0] = 1;
    for (size_t sl = 0; sl < n_slices; sl++) {
        Slice &S = slices[sl];
        const size_t c0 = first[sl], c1 = first[sl + 1];
        memset(&S.timing, 0, sizeof S.timing);
        const uint64_t r0 = c0 < c1 ? chunks[c0].read_first : n_reads;
        const uint64_t r1 = c0 < c1 ? chunks[c1 - 1].read_first + chunks[c1 - 1].n_reads : n_reads;
        if (c0 < c1) {
            S.chunks.assign(chunks + c0, chunks + c1);
            for (auto &ch : S.chunks) ch.read_first -= r0;
        }
        const int device = devices[std::min(sl / slices_per_dev, n_devices - 1)];
        jobs[sl] = ([=, &S, &base_mutex, &base_cv, &cons_base, &ops_base, &base_known]() {
            jtk_lc_session_t *s = nullptr;
            FetchPlan pl;
            if (c0 < c1) {
                S.rc = jtk_lc_session_create(params, c1 - c0, S.chunks.data(), tmpl_bases, read_bases, read_off + r0, ops, ops_off + r0,
                                             strand + r0, post_stride, device, &s);
                if (S.rc == 0) S.rc = jtk_lc_session_run(s, skip_polish);
                if (S.rc == 0)
                    S.rc = fetch_begin(s, pl, label + r0, log_post + r0 * post_stride, result + c0, want_cons, want_ops);
            }
            const bool ok = c0 < c1 && S.rc == 0;
            uint64_t cb = 0, ob = 0;
            {   // (also on failure: the slices behind this one are waiting for its end)
                std::unique_lock<std::mutex> lock(base_mutex);
                base_cv.wait(lock, [&]() { return base_known[sl] != 0; });
                cb = cons_base[sl];
                ob = ops_base[sl];
                cons_base[sl + 1] = cb + (ok ? pl.cons_total : 0);
                ops_base[sl + 1] = ob + (ok ? pl.ops_total : 0);
                base_known[sl + 1] = 1;
            }
            base_cv.notify_all();
            if (ok) {
                S.rc = fetch_finish(s, pl, cons_out, want_cons ? cons_off + c0 : nullptr, cb, cons_cap, ops_out,
                                    want_ops ? ops_out_off + r0 : nullptr, ob, ops_cap);
                if (S.rc == 0 && (pl.any_fail | fetch_split_results(s, label + r0, log_post + r0 * post_stride, result + c0)))
                    S.rc = jtk_fail(JTK_ERR_CHUNK_FAILED, "at least one chunk failed; see result[].status");
            } else {   // nothing from this slice: its chunks and reads get empty ranges
                if (want_cons)
                    for (size_t c = c0; c <= c1 && c <= n_chunks; c++) cons_off[c] = cb;
                if (want_ops)
                    for (uint64_t g = r0; g <= r1; g++) ops_out_off[g] = ob;
            }
            if (pl.ev0) (void)hipEventDestroy(pl.ev0);
            S.error = g_last_error;   // thread-local in the slice's thread
            S.timing = g_timing;
            if (s) jtk_lc_session_destroy(s);
        });
    }
    {   // per device: per_dev worker threads take the device's slices in order (a slice only ever waits for an EARLIER slice's
        // lengths, and those are taken first: no cycle)
        std::vector<std::thread> threads;
        std::vector<std::atomic<size_t>> next(n_devices);
        for (size_t d = 0; d < n_devices; d++) next[d] = d * slices_per_dev;
        for (size_t d = 0; d < n_devices; d++) {
            const size_t end = std::min(n_slices, (d + 1) * slices_per_dev);
            for (size_t w = 0; w < per_dev && d * slices_per_dev + w < end; w++)
                threads.emplace_back([&, d, end]() {
                    for (size_t sl = next[d].fetch_add(1); sl < end; sl = next[d].fetch_add(1))
                        if (jobs[sl]) jobs[sl]();
                });
        }
        for (auto &t : threads) t.join();
    }
    int rc = 0;
    memset(&g_timing, 0, sizeof g_timing);
    for (size_t sl = 0; sl < n_slices; sl++) {
        Slice &S = slices[sl];
        if (first[sl] >= first[sl + 1]) continue;
        if (S.rc != 0 && (rc == 0 || rc == JTK_ERR_CHUNK_FAILED)) {
            rc = S.rc;
            g_last_error = S.error;
        }
        timing_accumulate(g_timing, S.timing);
    }
    return rc;
}

int jtk_lc_cluster_chunks(const jtk_lc_params_t *params, size_t n_chunks, const jtk_lc_chunk_t *chunks,
                          const uint8_t *tmpl_bases, const uint8_t *read_bases, const uint64_t *read_off,
                          const uint8_t *ops, const uint64_t *ops_off, const uint8_t *strand, uint32_t *label,
                          double *log_post, uint32_t post_stride, jtk_lc_result_t *result, uint8_t *cons_out,
                          uint64_t *cons_off, uint64_t cons_cap, uint8_t *ops_out, uint64_t *ops_out_off,
                          uint64_t ops_cap, int device) {
    return run_once(params, n_chunks, chunks, tmpl_bases, read_bases, read_off, ops, ops_off, strand, 0, label,
                    log_post, post_stride, result, cons_out, cons_off, cons_cap, ops_out, ops_out_off, ops_cap, &device, 1);
}

// The same stage call over several GPUs of one node from ONE host process.  The chunks are dealt to the listed devices by
// longest-processing-time-first over the cost model of jtk_amd/sharding.py (`chunk_cost`: pair-HMM cells of the polishing
// passes + Metropolis steps per candidate k), the partition `bench.py --gpus N` uses between ranks: a device's share is in
// general NOT a contiguous range, so it is gathered into its own flat batch (templates stay where they are: chunks carry
// offsets), run as on a single device (sliced and overlapped), and its results are scattered back to the caller's order.
// The path has no exchange step, so there is no collective: this is SURVEY 8(b)'s `device_mask` as an explicit list.
static double chunk_cost(const jtk_lc_chunk_t &c) {
    const double n_k = (double)std::max<uint32_t>(1, std::min<uint32_t>(c.copy_num, 7) - (c.copy_num ? 1 : 0));
    return (double)c.n_reads * (double)c.tmpl_len * 3 * 61 * 2 + 20.0 * 2000.0 * (double)c.n_reads * n_k * 40.0;
}

int jtk_lc_cluster_chunks_multi(const jtk_lc_params_t *params, size_t n_chunks, const jtk_lc_chunk_t *chunks,
                                const uint8_t *tmpl_bases, const uint8_t *read_bases, const uint64_t *read_off,
                                const uint8_t *ops, const uint64_t *ops_off, const uint8_t *strand, uint32_t *label,
                                double *log_post, uint32_t post_stride, jtk_lc_result_t *result, uint8_t *cons_out,
                                uint64_t *cons_off, uint64_t cons_cap, uint8_t *ops_out, uint64_t *ops_out_off,
                                uint64_t ops_cap, const int *devices, size_t n_devices) {
    g_last_error.clear();
    if (!devices || n_devices == 0) return jtk_fail(JTK_ERR_INVALID_ARG, "no device given");
    if (n_devices == 1 || n_chunks < 2 * n_devices || !params || !chunks || !read_bases || !read_off || !ops || !ops_off ||
        !strand || !label || !log_post || !result)  // one device, a tiny batch, or arguments the single-device path reports on
        return run_once(params, n_chunks, chunks, tmpl_bases, read_bases, read_off, ops, ops_off, strand, 0, label,
                        log_post, post_stride, result, cons_out, cons_off, cons_cap, ops_out, ops_out_off, ops_cap, devices, 1);
    uint64_t n_reads = 0;
    if (int bad = check_contiguous(chunks, n_chunks, &n_reads)) return bad;
    // LPT: costliest chunk first (ties: input order), each to the device with the least load so far (ties: first listed)
    std::vector<size_t> by_cost(n_chunks);
    std::vector<double> cost(n_chunks);
    for (size_t c = 0; c < n_chunks; c++) {
        by_cost[c] = c;
        cost[c] = chunk_cost(chunks[c]);
    }
    std::stable_sort(by_cost.begin(), by_cost.end(), [&](size_t a, size_t b) { return cost[a] > cost[b]; });
    std::vector<double> load(n_devices, 0.0);
    std::vector<std::vector<size_t>> share(n_devices);
    for (size_t c : by_cost) {
        const size_t d = (size_t)(std::min_element(load.begin(), load.end()) - load.begin());
        share[d].push_back(c);
        load[d] += cost[c];
    }
    const bool want_cons = cons_out && cons_off, want_ops = ops_out && ops_out_off;
    struct Share {
        std::vector<jtk_lc_chunk_t> chunks;
        std::vector<uint8_t> read_bases, ops, strand, cons, ops_o;
        std::vector<uint64_t> read_off, ops_off, cons_off, ops_o_off;
        std::vector<uint32_t> label;
        std::vector<double> post;
        std::vector<jtk_lc_result_t> result;
        int rc = 0;
        std::string error;
        jtk_lc_timing_t timing;
    };
    std::vector<Share> shares(n_devices);
    std::vector<std::thread> threads;
    for (size_t d = 0; d < n_devices; d++) {
        std::sort(share[d].begin(), share[d].end());  // a device's chunks keep the caller's order
        threads.emplace_back([&, d]() {
            Share &S = shares[d];
            const std::vector<size_t> &ids = share[d];
            memset(&S.timing, 0, sizeof S.timing);
            if (ids.empty()) return;
            uint64_t nr = 0, nb = 0, no = 0, cons_need = 64, ops_need = 64;
            for (size_t c : ids) {
                const uint64_t r0 = chunks[c].read_first, r1 = r0 + chunks[c].n_reads;
                nr += r1 - r0;
                nb += read_off[r1] - read_off[r0];
                no += ops_off[r1] - ops_off[r0];
                cons_need += chunks[c].tmpl_len + chunks[c].tmpl_len / 4 + 64;
                ops_need += (uint64_t)chunks[c].n_reads * (chunks[c].tmpl_len / 4 + 72);
            }
            ops_need += no;
            S.chunks.reserve(ids.size());
            S.read_bases.resize(nb ? nb : 1);
            S.ops.resize(no ? no : 1);
            S.strand.resize(nr ? nr : 1);
            S.read_off.resize(nr + 1);
            S.ops_off.resize(nr + 1);
            S.label.resize(nr ? nr : 1);
            S.post.resize(nr ? nr * (size_t)post_stride : 1);
            S.result.resize(ids.size());
            if (want_cons) {
                S.cons.resize(cons_need);
                S.cons_off.resize(ids.size() + 1);
            }
            if (want_ops) {
                S.ops_o.resize(ops_need);
                S.ops_o_off.resize(nr + 1);
            }
            uint64_t r = 0, b = 0, o = 0;
            for (size_t c : ids) {
                jtk_lc_chunk_t ch = chunks[c];
                const uint64_t r0 = ch.read_first, r1 = r0 + ch.n_reads;
                ch.read_first = r;
                S.chunks.push_back(ch);
                memcpy(S.read_bases.data() + b, read_bases + read_off[r0], read_off[r1] - read_off[r0]);
                memcpy(S.ops.data() + o, ops + ops_off[r0], ops_off[r1] - ops_off[r0]);
                memcpy(S.strand.data() + r, strand + r0, r1 - r0);
                for (uint64_t g = r0; g < r1; g++, r++) {
                    S.read_off[r] = b + (read_off[g] - read_off[r0]);
                    S.ops_off[r] = o + (ops_off[g] - ops_off[r0]);
                }
                b += read_off[r1] - read_off[r0];
                o += ops_off[r1] - ops_off[r0];
            }
            S.read_off[nr] = b;
            S.ops_off[nr] = o;
            S.rc = run_once(params, ids.size(), S.chunks.data(), tmpl_bases, S.read_bases.data(), S.read_off.data(), S.ops.data(),
                            S.ops_off.data(), S.strand.data(), 0, S.label.data(), S.post.data(), post_stride, S.result.data(),
                            want_cons ? S.cons.data() : nullptr, want_cons ? S.cons_off.data() : nullptr, S.cons.size(),
                            want_ops ? S.ops_o.data() : nullptr, want_ops ? S.ops_o_off.data() : nullptr, S.ops_o.size(),
                            &devices[d], 1);
            S.error = g_last_error;  // thread-local in the share's thread
            S.timing = g_timing;
        });
    }
    for (auto &t : threads) t.join();
    // scatter the shares back into the caller's order
    int rc = 0;
    memset(&g_timing, 0, sizeof g_timing);
    std::vector<uint32_t> dev_of(n_chunks), idx_of(n_chunks);
    for (size_t d = 0; d < n_devices; d++) {
        const Share &S = shares[d];
        if (S.rc != 0 && (rc == 0 || rc == JTK_ERR_CHUNK_FAILED)) {
            rc = S.rc;
            g_last_error = S.error;
        }
        timing_accumulate(g_timing, S.timing);
        for (size_t i = 0; i < share[d].size(); i++) {
            dev_of[share[d][i]] = (uint32_t)d;
            idx_of[share[d][i]] = (uint32_t)i;
        }
    }
    if (rc != 0 && rc != JTK_ERR_CHUNK_FAILED) return rc;
    uint64_t co = 0, oo = 0;
    for (size_t c = 0; c < n_chunks; c++) {
        const Share &S = shares[dev_of[c]];
        const size_t i = idx_of[c];
        const uint64_t r0 = chunks[c].read_first, nr = chunks[c].n_reads, g0 = S.chunks[i].read_first;
        result[c] = S.result[i];
        memcpy(label + r0, S.label.data() + g0, nr * sizeof(uint32_t));
        memcpy(log_post + r0 * post_stride, S.post.data() + g0 * post_stride, nr * post_stride * sizeof(double));
        if (want_cons) {
            const uint64_t a = S.cons_off[i], len = S.cons_off[i + 1] - a;
            if (co + len > cons_cap) return jtk_fail(JTK_ERR_INVALID_ARG, "cons_cap too small");
            memcpy(cons_out + co, S.cons.data() + a, len);
            cons_off[c] = co;
            co += len;
        }
        if (want_ops) {
            const uint64_t a = S.ops_o_off[g0], len = S.ops_o_off[g0 + nr] - a;
            if (oo + len > ops_cap) return jtk_fail(JTK_ERR_INVALID_ARG, "ops_cap too small");
            memcpy(ops_out + oo, S.ops_o.data() + a, len);
            for (uint64_t g = 0; g < nr; g++) ops_out_off[r0 + g] = oo + (S.ops_o_off[g0 + g] - a);
            oo += len;
        }
    }
    if (want_cons) cons_off[n_chunks] = co;
    if (want_ops) ops_out_off[n_reads] = oo;
    return rc;
}

int jtk_lc_cluster_polished(const jtk_lc_params_t *params, size_t n_chunks, const jtk_lc_chunk_t *chunks,
                            const uint8_t *tmpl_bases, const uint8_t *read_bases, const uint64_t *read_off,
                            const uint8_t *ops, const uint64_t *ops_off, const uint8_t *strand, uint32_t *label,
                            double *log_post, uint32_t post_stride, jtk_lc_result_t *result, int device) {
    return run_once(params, n_chunks, chunks, tmpl_bases, read_bases, read_off, ops, ops_off, strand, 1, label,
                    log_post, post_stride, result, nullptr, nullptr, 0, nullptr, nullptr, 0, &device, 1);
}

// kiley polish_until_converge_antidiagonal(template, seqs, ops, strands, HMMPolishConfig::new(radius, take_num, ignore_edge))
// for a batch of independent windows: what consensus::polish_seg (haplotyper/src/consensus/mod.rs:445-496, :476-483) and
// polish_segments.rs run on 2 kbp windows of contigs -- the same kernels as the stage's own polishing step.
int jtk_lc_polish_chunks(const jtk_lc_params_t *params, size_t n_chunks, const jtk_lc_chunk_t *chunks,
                         const uint8_t *tmpl_bases, const uint8_t *read_bases, const uint64_t *read_off,
                         const uint8_t *ops, const uint64_t *ops_off, const uint8_t *strand, uint32_t radius,
                         uint32_t take_num, uint32_t ignore_edge, uint8_t *cons_out, uint64_t *cons_off, uint64_t cons_cap,
                         uint8_t *ops_out, uint64_t *ops_out_off, uint64_t ops_cap, jtk_lc_result_t *result, int device) {
    g_last_error.clear();
    if (!params) return jtk_fail(JTK_ERR_INVALID_ARG, "null params");
    if (n_chunks && (!chunks || !tmpl_bases || !read_bases || !read_off || !ops || !ops_off || !strand))
        return jtk_fail(JTK_ERR_INVALID_ARG, "null input");
    if (!cons_out || !cons_off || !ops_out || !ops_out_off) return jtk_fail(JTK_ERR_INVALID_ARG, "null output");
    std::vector<ChunkExtra> extra(n_chunks);
    std::vector<jtk_lc_chunk_t> ch(chunks, chunks + (chunks ? n_chunks : 0));
    for (size_t c = 0; c < n_chunks; c++) {
        memset(&extra[c], 0, sizeof extra[c]);
        // radius 0: derive it from the window length like the stage does (mod.rs:96,105)
        extra[c].radius = radius ? radius : (uint32_t)std::ceil((double)ch[c].tmpl_len * params->band_frac) / 2;
        extra[c].take_num = take_num;
        ch[c].copy_num = 1;  // no clustering happens; keeps every posterior row a single entry
    }
    jtk_lc_params_t pp = *params;
    if (pp.gains.max_homopolymer_len == 0) pp.gains.max_homopolymer_len = 1;  // polishing does not use the gains
    jtk_lc_session_t *s = nullptr;
    int rc = session_create_ex(&pp, n_chunks, ch.data(), tmpl_bases, read_bases, read_off, ops, ops_off, strand, 1, device,
                               extra.data(), ignore_edge, &s, true);
    if (rc) return rc;
    std::unique_ptr<jtk_lc_session> guard(s);
    s->resume_rng = false;
    if ((rc = run_batch(s, 0))) return rc;
    return jtk_lc_session_fetch(s, nullptr, nullptr, result, cons_out, cons_off, cons_cap, ops_out, ops_out_off, ops_cap);
}
