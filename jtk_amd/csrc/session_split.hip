// session_split.hip -- clustering_recursive's split branch (mod.rs:138-189), driven from the host.
//
// Chunks with copy_num >= 8 take the split branch: the batch pass clusters them into at most four groups, and run_split()
// then drives the sub-problems -- polish the group's consensus, cluster it with its share of the copies, recurse -- as
// further resident batches, one sub-problem per chunk and round because a chunk's calls share one RNG stream in depth-first
// order.
#include <cmath>
#include <cstring>

#include "session_internal.h"

namespace {

const uint32_t UPPER_COPY_NUM = JTK_MAX_COPY + 1;  // mod.rs:85
const uint32_t BRANCH_NUM = 4;                     // mod.rs:139

// One clustering_recursive call of a chunk, waiting for its clustering() or for its sub-calls.
struct SplitFrame {
    std::vector<uint8_t> tmpl;              // bases the call starts from (a sub-call polishes them first, mod.rs:153-155)
    std::vector<uint32_t> rid;              // its reads: indices into the session's batch
    std::vector<std::vector<uint8_t>> ops;  // their ops against tmpl
    uint32_t copy_num = 0;
    bool have = false;                      // the device pass of this call has run:
    SplitResult own;                        //   clustering() with min(copy_num, BRANCH_NUM-or-itself) clusters
    std::vector<uint8_t> cons;              //   the consensus it clustered on
    std::vector<std::vector<uint8_t>> cops; //   and the ops re-threaded onto it
    std::vector<uint32_t> copy_numbers;     // estim_copy_num of the split
    std::vector<SplitResult> kids;          // finished sub-calls, in cluster order
};
struct SplitChunk {
    uint32_t chunk = 0;
    uint64_t rng[4];
    std::vector<SplitFrame> stack;
    bool done = false;
};

void seed_from_u64(uint64_t seed, uint64_t out[4]) {  // rand_core SeedableRng::seed_from_u64 for a 32-byte seed: SplitMix64
    for (int i = 0; i < 4; i++) {
        seed += 0x9e3779b97f4a7c15ULL;
        uint64_t z = seed;
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
        out[i] = z ^ (z >> 31);
    }
}
void rng_skip(uint64_t s[4], uint64_t draws) {  // the xoshiro256 state after `draws` outputs
    for (uint64_t i = 0; i < draws; i++) {
        const uint64_t t = s[1] << 17;
        s[2] ^= s[0];
        s[3] ^= s[1];
        s[1] ^= s[2];
        s[0] ^= s[3];
        s[2] ^= t;
        s[3] = (s[3] << 45) | (s[3] >> 19);
    }
}

// estim_copy_num (mod.rs:223-243): one copy per cluster, every further copy to the cluster whose read count is
// farthest from coverage * copies (max_by keeps the last maximum)
std::vector<uint32_t> estim_copy_num(const std::vector<uint32_t> &asn, uint32_t k, uint32_t copy_num, double coverage) {
    std::vector<double> counts(k, 0.0);
    for (uint32_t a : asn) counts[a] += 1.0;
    std::vector<uint32_t> cp(k, 1);
    for (uint32_t it = k; it < copy_num; it++) {
        uint32_t arg = 0;
        double best = 0.0;
        for (uint32_t c = 0; c < k; c++) {
            const double d = counts[c] - coverage * (double)cp[c], v = d * d;
            if (c == 0 || !(v < best)) {
                best = v;
                arg = c;
            }
        }
        cp[arg] += 1;
    }
    return cp;
}

// the merge of mod.rs:161-187
SplitResult merge_split(const SplitFrame &f) {
    const uint32_t k = f.own.k;
    std::vector<uint32_t> offsets(k), pointers(k, 0);
    uint32_t total = 0;
    for (uint32_t c = 0; c < k; c++) {
        offsets[c] = total;
        total += f.kids[c].k;
    }
    SplitResult r;
    r.k = total;
    double sub = 0.0;
    for (uint32_t c = 0; c < k; c++) sub += f.kids[c].score;
    r.score = sub + f.own.score;
    const size_t n = f.own.asn.size();
    r.asn.resize(n);
    r.post.resize(n * total);
    for (size_t i = 0; i < n; i++) {
        const uint32_t a = f.own.asn[i], pt = pointers[a]++;
        const SplitResult &kid = f.kids[a];
        double *po = &r.post[i * total];
        uint32_t w = 0;
        for (uint32_t c = 0; c < k; c++) {
            const double lk = f.own.post[i * k + c] - jtk_log((double)f.kids[c].k);
            for (uint32_t t = 0; t < f.kids[c].k; t++) po[w++] = lk;
        }
        for (uint32_t t = 0; t < kid.k; t++) po[t + offsets[a]] += kid.post[(size_t)pt * kid.k + t] + jtk_log((double)kid.k);
        double sum = 0.0;
        for (uint32_t t = 0; t < total; t++) sum += jtk_exp(po[t]);
        if (!(std::fabs(1.0 - sum) < 0.0001)) r.status = JTK_ERR_CHUNK_FAILED;  // the reference asserts (mod.rs:184)
        r.asn[i] = offsets[a] + kid.asn[pt];
    }
    return r;
}

}  // namespace

int run_split(jtk_lc_session_t *s) {
    jtk_lc_timing_t acc = g_timing;
    // ---- what the batch pass left for the split chunks: labels, posteriors, consensus, ops, draws
    std::vector<uint32_t> label(s->n_reads);
    std::vector<double> post((size_t)s->n_reads * s->post_stride);
    std::vector<jtk_lc_result_t> res(s->n_chunks);
    std::vector<uint8_t> cons(s->tmpl_bytes + 8), ops_out(s->ops_bytes + 8);
    std::vector<uint64_t> cons_off(s->n_chunks + 1), ops_off(s->n_reads + 1);
    std::vector<ChunkState> state(s->n_chunks);
    s->split.clear();  // fetch below must see the batch pass's own results
    int rc = jtk_lc_session_fetch(s, label.data(), post.data(), res.data(), cons.data(), cons_off.data(), cons.size(),
                                  ops_out.data(), ops_off.data(), ops_out.size());
    if (rc != 0 && rc != JTK_ERR_CHUNK_FAILED) return rc;
    JTK_HIP_TRY(hipMemcpy(state.data(), s->d_state.p, state.size() * sizeof(ChunkState), hipMemcpyDeviceToHost));
    acc.d2h_ms = 0;
    s->split.assign(s->n_chunks, SplitResult());
    std::vector<SplitChunk> work;
    for (uint32_t c = 0; c < s->n_chunks; c++) {
        if (s->h_copy0[c] < UPPER_COPY_NUM) continue;
        const ChunkMeta &cm = s->h_chunks[c];
        if (res[c].status != 0) {
            s->split[c].k = 1;
            s->split[c].status = res[c].status;
            continue;
        }
        if (res[c].cluster_num > s->post_stride) {  // (unreachable since session_create checks copy_num; per chunk anyway)
            s->split[c].k = 1;
            s->split[c].status = JTK_ERR_INVALID_ARG;
            continue;
        }
        SplitChunk w;
        w.chunk = c;
        seed_from_u64(cm.chunk_id * 3490ULL, w.rng);  // mod.rs:97
        rng_skip(w.rng, state[c].draws);
        SplitFrame f;
        f.copy_num = s->h_copy0[c];
        f.have = true;
        f.own.k = res[c].cluster_num;
        f.own.score = res[c].score;
        f.cons.assign(cons.begin() + cons_off[c], cons.begin() + cons_off[c + 1]);
        for (uint32_t r = 0; r < cm.n_reads; r++) {
            const uint32_t g = cm.read_first + r;
            f.rid.push_back(g);
            f.own.asn.push_back(label[g]);
            for (uint32_t t = 0; t < f.own.k; t++) f.own.post.push_back(post[(size_t)g * s->post_stride + t]);
            f.cops.emplace_back(ops_out.begin() + ops_off[g], ops_out.begin() + ops_off[g + 1]);
        }
        w.stack.push_back(std::move(f));
        work.push_back(std::move(w));
    }
    // ---- rounds: advance every chunk to its next clustering() call, run those calls as one resident batch
    for (;;) {
        std::vector<SplitChunk *> waiting;
        for (SplitChunk &w : work) {
            while (!w.done) {
                SplitFrame &f = w.stack.back();
                if (!f.have) break;
                SplitResult out;
                bool finished = false;
                if (f.own.status != 0) {
                    out.k = 1;
                    out.status = f.own.status;
                    w.stack.resize(1);  // the chunk fails as a whole
                    finished = true;
                } else if (f.copy_num < UPPER_COPY_NUM || f.own.k <= 1) {  // mod.rs:136-137, :146-148
                    out = std::move(f.own);
                    finished = true;
                } else if (f.kids.size() == f.own.k) {
                    out = merge_split(f);
                    finished = true;
                } else {
                    if (f.copy_numbers.empty())
                        f.copy_numbers = estim_copy_num(f.own.asn, f.own.k, f.copy_num, s->params.haploid_coverage);
                    const uint32_t c = (uint32_t)f.kids.size(), cp = f.copy_numbers[c];
                    SplitFrame kid;  // filter_sub_clusters (mod.rs:198-221)
                    for (size_t i = 0; i < f.rid.size(); i++)
                        if (f.own.asn[i] == c) {
                            kid.rid.push_back(f.rid[i]);
                            kid.ops.push_back(f.cops[i]);
                        }
                    if (cp < 2 || kid.rid.empty()) {
                        // clustering() returns at once, with no draw (pseudo_mcmc.rs:86-88): the polish before it
                        // (mod.rs:153-155) cannot reach the result and is not run
                        SplitResult t;
                        t.k = 1;
                        t.asn.assign(kid.rid.size(), 0);
                        t.post.assign(kid.rid.size(), 0.0);
                        f.kids.push_back(std::move(t));
                        continue;
                    }
                    kid.tmpl = f.cons;
                    kid.copy_num = cp;
                    w.stack.push_back(std::move(kid));
                    continue;
                }
                if (finished) {
                    w.stack.pop_back();
                    if (w.stack.empty()) {
                        // the merged clustering has up to copy_num clusters: the caller's rows must hold them
                        if (out.status == 0 && out.k > s->post_stride) out.status = JTK_ERR_INVALID_ARG;
                        s->split[w.chunk] = std::move(out);
                        w.done = true;
                    } else if (out.status != 0) {
                        w.stack.back().own.status = out.status;
                    } else {
                        w.stack.back().kids.push_back(std::move(out));
                    }
                }
            }
            if (!w.done) waiting.push_back(&w);
        }
        if (waiting.empty()) break;
        // pack the waiting calls
        const size_t nb = waiting.size();
        std::vector<jtk_lc_chunk_t> chunks(nb);
        std::vector<ChunkExtra> extra(nb);
        std::vector<uint8_t> tmpl, reads, opsv, strand;
        std::vector<uint64_t> roff(1, 0), ooff(1, 0);
        for (size_t b = 0; b < nb; b++) {
            const SplitChunk &w = *waiting[b];
            const SplitFrame &f = w.stack.back();
            const ChunkMeta &cm = s->h_chunks[w.chunk];
            chunks[b].chunk_id = cm.chunk_id;
            chunks[b].copy_num = f.copy_num;
            chunks[b].n_reads = (uint32_t)f.rid.size();
            chunks[b].tmpl_off = tmpl.size();
            chunks[b].tmpl_len = f.tmpl.size();
            chunks[b].read_first = strand.size();
            extra[b].radius = cm.radius;
            extra[b].local_coverage = cm.local_coverage;
            memcpy(extra[b].rng, w.rng, 32);
            extra[b].take_num = 0;
            tmpl.insert(tmpl.end(), f.tmpl.begin(), f.tmpl.end());
            for (size_t i = 0; i < f.rid.size(); i++) {
                const uint32_t g = f.rid[i];
                reads.insert(reads.end(), s->h_read_bases.begin() + s->h_read_off[g], s->h_read_bases.begin() + s->h_read_off[g + 1]);
                roff.push_back(reads.size());
                opsv.insert(opsv.end(), f.ops[i].begin(), f.ops[i].end());
                ooff.push_back(opsv.size());
                strand.push_back(s->h_strand[g]);
            }
        }
        const uint32_t stride = JTK_MAX_COPY;
        jtk_lc_session_t *sub = nullptr;
        rc = session_create_ex(&s->params, nb, chunks.data(), tmpl.data(), reads.data(), roff.data(), opsv.data(), ooff.data(),
                               strand.data(), stride, s->device, extra.data(), 0 /* mod.rs:153 */, &sub);
        if (rc) return rc;
        std::unique_ptr<jtk_lc_session> guard(sub);
        if ((rc = run_batch(sub, 0))) return rc;
        for (int k = 0; k < JTK_K_COUNT; k++) {
            acc.kernel_ms[k] += g_timing.kernel_ms[k];
            acc.kernel_launches[k] += g_timing.kernel_launches[k];
        }
        acc.total_ms += g_timing.total_ms;
        const uint32_t nr = (uint32_t)strand.size();
        std::vector<uint32_t> lab(nr);
        std::vector<double> pst((size_t)nr * stride);
        std::vector<jtk_lc_result_t> rs(nb);
        std::vector<uint8_t> cs(sub->tmpl_bytes + 8), os(sub->ops_bytes + 8);
        std::vector<uint64_t> coff(nb + 1), ofo(nr + 1);
        std::vector<ChunkState> sst(nb);
        rc = jtk_lc_session_fetch(sub, lab.data(), pst.data(), rs.data(), cs.data(), coff.data(), cs.size(), os.data(),
                                  ofo.data(), os.size());
        if (rc != 0 && rc != JTK_ERR_CHUNK_FAILED) return rc;
        JTK_HIP_TRY(hipMemcpy(sst.data(), sub->d_state.p, sst.size() * sizeof(ChunkState), hipMemcpyDeviceToHost));
        for (size_t b = 0; b < nb; b++) {
            SplitChunk &w = *waiting[b];
            SplitFrame &f = w.stack.back();
            f.have = true;
            f.own.status = rs[b].status;
            if (rs[b].status != 0) continue;
            rng_skip(w.rng, sst[b].draws);
            f.own.k = rs[b].cluster_num;
            f.own.score = rs[b].score;
            f.cons.assign(cs.begin() + coff[b], cs.begin() + coff[b + 1]);
            const uint32_t first = (uint32_t)chunks[b].read_first;
            for (uint32_t r = 0; r < chunks[b].n_reads; r++) {
                f.own.asn.push_back(lab[first + r]);
                for (uint32_t t = 0; t < f.own.k; t++) f.own.post.push_back(pst[(size_t)(first + r) * stride + t]);
                f.cops.emplace_back(os.begin() + ofo[first + r], os.begin() + ofo[first + r + 1]);
            }
        }
    }
    g_timing = acc;
    return 0;
}
