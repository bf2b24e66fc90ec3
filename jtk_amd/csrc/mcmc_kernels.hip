// mcmc_kernels.hip -- the read-clustering loop on the device: one workgroup of two wavefronts per chunk.
//
// Follows, statement by statement, haplotyper/src/local_clustering/pseudo_mcmc.rs
//   cluster_filtered_variants :213-274   mcmc_clustering :649-670   mcmc_with_filter :704-762
//   flip :764-783   get_lk :785-795   LKCount :797-845   get_used_columns :847-869
//   get_read_lk_gains :381-408   get_likelihood_gain :353-379   use_highest_gain :673-693
//   expected_gains :286-306   clustering tail :98-105   to_posterior_probability :342-347
// and haplotyper/src/misc.rs  kmeans :231-259, suggest_first :315-341, logsumexp :84-92,
// with the rand 0.8.5 / rand_xoshiro 0.6.0 sampling restated exactly as in oracle/rng.c.
//
// The chain is strictly sequential per chunk (one RNG stream threads through k-means, 20 restarts and every
// candidate k, local_clustering/mod.rs:97).  A lone wavefront on CDNA4 issues a dependent instruction every
// ~8 cycles and pays ~30 for a value that crosses from the vector to the scalar side, so the chain is bound by the
// length of the dependent chain of a step, not by bandwidth.  What buys speed without changing a bit of the result:
//  * PIPELINE: wave 1 ("producer") runs xoshiro256** lane-parallel (GF(2) jump-ahead) into an LDS ring and, for the
//    diploid chain, parses the proposal that would start at every stream position into a 32-bit record; wave 0
//    ("consumer") runs the algorithm and takes every random draw -- k-means initialisation, proposals, Bernoulli
//    tests -- from that ring, in stream order.  The stream never depends on the chain, so nothing is speculated.
//  * THE DIPLOID CHAIN (K == 2, n <= 127, D <= 8) keeps, per read, the exact likelihood of the state with that read
//    flipped (rebuilt lane-parallel after every move) and walks over the proposals that are certainly rejected and
//    leave no rounding residue; everything else is settled from the read's lane (mcmc_chain_k2).
//  * THE GENERIC CHAIN keeps LKCount[c][d] in registers (lane = column, K a template parameter), the counts as
//    integers (num_pos and 3*num_pos - 7*num_neg, which decides is_informative exactly), labels / sizes / >0 masks
//    as wave-uniform scalars, and commits or undoes a proposal with the reference's own arithmetic
//    ((tg - x) + x, not a restore); get_lk's left-to-right sum visits only the non-zero terms.
// Sums that the reference evaluates left to right are evaluated left to right here -- integer labels only
// match if every f64 rounding matches.
// The parts, each a header that this file alone includes (one translation unit: the device code is forceinline or template
// throughout): chain_stats.h the statistics build, chain_layout.h the work area's array list and its sizes, chain_rng.h the
// consumer's draws, chain_lds.h the carve, chain_common.h k-means and the chains' shared helpers, chain_producer.h the producer
// wave, chain_generic.h / chain_tab.h / chain_k2.h the three chains, chain_jump_table.h the producer's table on the host.
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "device_common.h"
#include "chain_stats.h"
#include "chain_layout.h"
#include "chain_rng.h"
#include "chain_lds.h"
#include "chain_common.h"
#include "chain_producer.h"
#include "chain_jump_table.h"
#include "chain_generic.h"
#include "chain_tab.h"
#include "chain_k2.h"

namespace {

// get_lk (:785-795) of the labels in `assign` from freshly filled counters (reads in order, :752-758): what the
// reference compares the tracked maximum with before returning it (`assert!((max - lk).abs() < 0.0001)`, :759-760).
template <int K, bool HUGE>
__device__ __noinline__ double fresh_lk(LdsShape shape, uint32_t n_in, uint32_t D_in, double cov_in, uint32_t lane) {
    const uint32_t n = uni(n_in), D = uni(D_in);
    const double cov = unif64(cov_in);
    const Lds m = lds_carve<HUGE>(shape);
    const uint8_t *assign = m.assign;
    Counts<K> q;
    int clusters[K];
    fill_counts<K>(m, n, D, assign, q, clusters, lane);
    const unsigned long long usedm = __ballot(lane < D && column_used<K>(q));
    double S = 0.0;
#pragma unroll
    for (int c = 0; c < K; c++) {
        const uint32_t x = uni((uint32_t)clusters[c]);
        double mx = -__builtin_inf();
        for (int cc = 1; cc <= K; cc++) {
            const double lam = cov * (double)cc;
            mx = jtk_fmax(mx, (double)x * jtk_log(lam) - lam - m.lfact[x]);
        }
        S += unif64(mx);
    }
#pragma unroll
    for (int c = 0; c < K; c++) {
        unsigned long long mm = usedm;
        while (mm) {
            const uint32_t d = (uint32_t)__builtin_ctzll(mm);
            mm &= mm - 1;
            S += jtk_fmax(readlane_f64(q.tg[c], d), 0.0);
        }
    }
    return S;
}

template <int K, bool LIGHT, bool HUGE>
__device__ __forceinline__ double mcmc_chain_dispatch(const Lds &m, uint32_t n, uint32_t D, double cov, Rng &rng, uint32_t lane);

// mcmc_with_filter (:704-762): the chain, then the reference's closing self-check.  NaN = the reference panics.
template <int K, bool LIGHT, bool HUGE>
__device__ __forceinline__ double mcmc_with_filter(const Lds &m, uint32_t n, uint32_t D, double cov, Rng &rng, uint32_t lane) {
    const double max = mcmc_chain_dispatch<K, LIGHT, HUGE>(m, n, D, cov, rng, lane);
    const double fresh = fresh_lk<K, HUGE>(m.shape, n, D, cov, lane);
    if (!ubool(fabs(max - fresh) < 0.0001)) return __builtin_nan("");
    return max;
}

template <int K, bool LIGHT, bool HUGE>
__device__ __forceinline__ double mcmc_chain_dispatch(const Lds &m, uint32_t n, uint32_t D, double cov, Rng &rng, uint32_t lane) {
    if (HUGE) return mcmc_chain<K, false>(m, n, D, cov, rng, lane);  // the work area is in global memory (mcmc_kernel_huge)
    if (LIGHT) {
        // the light kernel (mcmc_kernel_light) holds only the chain variants that fit 168 registers; chain_split_kernel
        // sends it nothing else.  NaN = the chunk fails, loudly, should that ever not hold.
        if (!(K == 2 && n <= JTK_LIGHT_MAX_READS && D >= 1 && D <= JTK_LIGHT_MAX_DIM)) return __builtin_nan("");
        rng_set_parse_mode(rng, PM_K2, lane);
        const K2Mem km = {m.data, m.lfact, m.assign, m.fbuf, m.k2_stats};
        if (n <= 63) {
            if (D == 1) return mcmc_chain_k2<1, 1>(km, n, D, cov, &rng, lane);
            return mcmc_chain_k2<2, 1>(km, n, D, cov, &rng, lane);
        }
        if (D == 1) return mcmc_chain_k2<1, 2>(km, n, D, cov, &rng, lane);  // 64 .. 127 reads: two table registers
        return mcmc_chain_k2<2, 2>(km, n, D, cov, &rng, lane);
    }
    if (K == 2 && n <= 127 && D >= 1 && D <= 8) {
        rng_set_parse_mode(rng, PM_K2, lane);
        const K2Mem km = {m.data, m.lfact, m.assign, m.fbuf, m.k2_stats};
        if (n <= 63) {
            if (D == 1) return mcmc_chain_k2<1, 1>(km, n, D, cov, &rng, lane);
            if (D == 2) return mcmc_chain_k2<2, 1>(km, n, D, cov, &rng, lane);
            if (D == 3) return mcmc_chain_k2<3, 1>(km, n, D, cov, &rng, lane);
            if (D == 4) return mcmc_chain_k2<4, 1>(km, n, D, cov, &rng, lane);
            return mcmc_chain_k2<8, 1>(km, n, D, cov, &rng, lane);
        }
        if (D <= 2) return mcmc_chain_k2<2, 2>(km, n, D, cov, &rng, lane);
        if (D <= 4) return mcmc_chain_k2<4, 2>(km, n, D, cov, &rng, lane);
        return mcmc_chain_k2<8, 2>(km, n, D, cov, &rng, lane);
    }
    rng_set_parse_mode(rng, (uint32_t)K, lane);
    return mcmc_chain_tab<K>(m.shape, n, D, cov, &rng, lane);
}

// get_read_lk_gains (:381-408): used columns -> used[], per-read gain -> fbuf[]
template <int K>
__device__ __forceinline__ void get_read_lk_gains(const Lds &m, uint32_t n, uint32_t D, const uint8_t *assign, uint8_t *used,
                                  uint32_t lane) {
    Counts<K> q;
    int clusters[K];
    fill_counts<K>(m, n, D, assign, q, clusters, lane);
    const bool u = lane < D && column_used<K>(q);
    if (lane < D) used[lane] = u ? 1 : 0;
#pragma unroll
    for (int c = 0; c < K; c++)
        if (lane < D) m.val[c * D + lane] = (u && JTK_POS_THR < q.tg[c]) ? 1.0 : 0.0;  // column counts for cluster c
    wsync();
    for (uint32_t i = lane; i < n; i += 64) {
        const uint32_t a = assign[i];
        double s = 0.0;
        for (uint32_t d = 0; d < D; d++)
            if (m.val[a * D + d] != 0.0) s += m.data[i * D + d];
        m.fbuf[i] = s;
    }
    wsync();
}

// get_likelihood_gain (:353-379): out[i*K + c]
template <int K>
__device__ __forceinline__ void get_likelihood_gain(const Lds &m, uint32_t n, uint32_t D, const uint8_t *assign, double *out,
                                    uint32_t lane) {
    Counts<K> q;
    int clusters[K];
    fill_counts<K>(m, n, D, assign, q, clusters, lane);
    const bool u = lane < D && column_used<K>(q);
#pragma unroll
    for (int c = 0; c < K; c++)
        if (lane < D) m.val[c * D + lane] = (u && JTK_POS_THR < q.tg[c]) ? 1.0 : 0.0;
    wsync();
    for (uint32_t i = lane; i < n; i += 64)
        for (int c = 0; c < K; c++) {
            double s = 0.0;
            for (uint32_t d = 0; d < D; d++)
                if (m.val[c * D + d] != 0.0) s += m.data[i * D + d];
            out[i * K + c] = s;
        }
    wsync();
}

// mcmc_clustering (:649-670): labels -> m.best, per-read gains -> m.fbuf, used columns -> m.used
template <int K, bool LIGHT, bool HUGE>
__device__ __forceinline__ bool mcmc_clustering(const Lds &m, uint32_t n, uint32_t D, double cov, Rng &rng, double *score,
                                uint32_t lane) {
    double best = 0.0;
    bool have = false;
    for (int it = 0; it < 20; it++) {
        if (!kmeans(m, n, D, K, rng, lane)) return false;
        const double lk = mcmc_with_filter<K, LIGHT, HUGE>(m, n, D, cov, rng, lane);
        if (ubool(lk != lk)) return false;  // the reference panicked inside mcmc_with_filter
        if (!have || !(lk < best)) {  // max_by: the last maximum wins
            best = lk;
            have = true;
            for (uint32_t i = lane; i < n; i += 64) m.best[i] = m.assign[i];
            wsync();
        }
    }
    get_read_lk_gains<K>(m, n, D, m.best, m.used, lane);
    // cluster_lk = sum_c max_poisson_lk(count_c, cov, 1, K)
    double cluster_lk = 0.0;
    for (int c = 0; c < K; c++) {
        uint32_t cnt = 0;
        for (uint32_t i = 0; i < n; i++) cnt += m.best[i] == c ? 1u : 0u;
        double mx = -__builtin_inf();
        for (int cc = 1; cc <= K; cc++) {
            const double lam = cov * (double)cc;
            mx = jtk_fmax(mx, (double)cnt * jtk_log(lam) - lam - m.lfact[cnt]);
        }
        cluster_lk += mx;
    }
    *score = best - cluster_lk;
    return true;
}

// out of line: one candidate cluster count per call keeps the kernel body (k-means, model selection, posteriors) small
template <int K, bool LIGHT, bool HUGE = false>
__device__ __attribute__((noinline)) bool run_k(LdsShape shape, uint32_t n_in, uint32_t D_in, double cov_in, Rng &rng, double *score,
                                                uint32_t lane) {
    const uint32_t n = uni(n_in), D = uni(D_in);
    const double cov = unif64(cov_in);
    const Lds m = lds_carve<HUGE>(shape);
    return mcmc_clustering<K, LIGHT, HUGE>(m, n, D, cov, rng, score, lane);
}

template <bool LIGHT, bool HUGE>
__device__ __forceinline__ bool run_k_dyn(uint32_t k, LdsShape m, uint32_t n, uint32_t D, double cov, Rng &rng, double *score,
                          uint32_t lane) {
    if (LIGHT) return k == 2 ? run_k<2, true>(m, n, D, cov, rng, score, lane) : false;
    switch (k) {
        case 2: return run_k<2, false, HUGE>(m, n, D, cov, rng, score, lane);
        case 3: return run_k<3, false, HUGE>(m, n, D, cov, rng, score, lane);
        case 4: return run_k<4, false, HUGE>(m, n, D, cov, rng, score, lane);
        case 5: return run_k<5, false, HUGE>(m, n, D, cov, rng, score, lane);
        case 6: return run_k<6, false, HUGE>(m, n, D, cov, rng, score, lane);
        case 7: return run_k<7, false, HUGE>(m, n, D, cov, rng, score, lane);
        default: return false;
    }
}

template <bool LIGHT>
__device__ __forceinline__ void likelihood_gain_dyn(uint32_t k, const Lds &m, uint32_t n, uint32_t D, const uint8_t *assign,
                                    double *out, uint32_t lane) {
    if (LIGHT) {  // copy number 2: one or two clusters
        if (k == 1) get_likelihood_gain<1>(m, n, D, assign, out, lane);
        else get_likelihood_gain<2>(m, n, D, assign, out, lane);
        return;
    }
    switch (k) {
        case 1: get_likelihood_gain<1>(m, n, D, assign, out, lane); break;
        case 2: get_likelihood_gain<2>(m, n, D, assign, out, lane); break;
        case 3: get_likelihood_gain<3>(m, n, D, assign, out, lane); break;
        case 4: get_likelihood_gain<4>(m, n, D, assign, out, lane); break;
        case 5: get_likelihood_gain<5>(m, n, D, assign, out, lane); break;
        case 6: get_likelihood_gain<6>(m, n, D, assign, out, lane); break;
        default: get_likelihood_gain<7>(m, n, D, assign, out, lane); break;
    }
}

// (trace instantiation only) get_read_lk_gains for a run-time cluster count 2 .. 7
__device__ __forceinline__ void read_lk_gains_dyn(uint32_t k, const Lds &m, uint32_t n, uint32_t D, const uint8_t *assign, uint8_t *used,
                                                  uint32_t lane) {
    switch (k) {
        case 2: get_read_lk_gains<2>(m, n, D, assign, used, lane); break;
        case 3: get_read_lk_gains<3>(m, n, D, assign, used, lane); break;
        case 4: get_read_lk_gains<4>(m, n, D, assign, used, lane); break;
        case 5: get_read_lk_gains<5>(m, n, D, assign, used, lane); break;
        case 6: get_read_lk_gains<6>(m, n, D, assign, used, lane); break;
        default: get_read_lk_gains<7>(m, n, D, assign, used, lane); break;
    }
}

__device__ __forceinline__ double gains_expected(const jtk_gains_t *g, uint32_t homop_len, int dt) {
    if (homop_len == 0) homop_len = 1;
    const uint32_t h = homop_len < g->max_homopolymer_len ? homop_len : g->max_homopolymer_len;
    return dt == JTK_DIFF_SUBST ? g->subst[h - 1].gain
                                : (dt == JTK_DIFF_DEL ? g->deletions[h - 1].gain : g->insertions[h - 1].gain);
}

// one workgroup of two waves per chunk: wave 0 runs the algorithm, wave 1 feeds it proposals
// Register budget: two waves per SIMD (<= 256 registers; the kernel needs 248).  A chain workgroup is two latency-bound waves
// that leave their SIMDs idle most of the time: at 360 registers (the legacy chain inlined) a chain wave had its SIMD to itself
// and 625 workgroups shut every other kernel out of the machine; at 248 two of them share a SIMD, or one sits beside a
// pair-HMM wave of another batch (152 registers) -- bench.py overlaps batches: 1,680 -> 1,820 chunks/s.
//
// Two entry points share the body.  `mcmc_kernel` holds every chain variant (248 registers).  `mcmc_kernel_light` holds only
// what a diploid pile-up of <= 127 reads (JTK_LIGHT_MAX_READS) with one or two variant columns needs -- 80 % of the headline's chunks have D <= 1,
// 97 % D <= 2 -- and fits 168 registers: three of its waves share a SIMD, or one of them sits beside TWO pair-HMM waves of
// another batch (168 + 2 x 168 <= 512) where a 248-register chain wave leaves room for one.  Which chunk goes where is
// decided on the device (chain_split_kernel: D is known only after the filter), with no host round trip.
#ifndef JTK_MCMC_WAVES
#define JTK_MCMC_WAVES 2
#endif
// TRACE = true (mcmc_kernel_trace, jtk_lc_session_trace): the same clustering once more for ONE chunk, leaving what the reference's
// trace! rows of cluster_filtered_variants need in `trace` (doubles): [0] = first k, [1] = last k of the RANGE row (:236), [2] = number
// of records; record r at [8 + 16 r]: k, score, expected_gain, improved_reads (the LK rows :250,:256), accepted?, then the k cluster
// sizes (COUNTS :262); from [JTK_TRACE_OLD] the n per-read gains of the accepted clustering (read_lk_gains :229, which feeds only
// improved_reads).  The product instantiations compile none of it.
#define JTK_TRACE_REC 8
#define JTK_TRACE_REC_LEN 16
#define JTK_TRACE_OLD (JTK_TRACE_REC + 8 * JTK_TRACE_REC_LEN)
template <bool LIGHT, bool HUGE = false, bool TRACE = false>
__device__ __forceinline__ void mcmc_body(uint32_t blk, const ChunkMeta *chunks, ChunkState *state,
                                                  const jtk_lc_params_t *params, const double *feat_all,
                                                  const uint32_t *vtype_all, const uint64_t *vt_off_all,
                                                  uint32_t vt_stride_mode, uint32_t *label_all, double *post_all,
                                                  uint32_t post_stride, double *lg_all, const uint64_t *lg_off,
                                                  uint32_t lds_n, uint32_t lds_d, uint32_t lds_k, uint32_t seg_log_in,
                                                  uint32_t flags, const uint64_t *rng_resume, const uint32_t *order,
                                                  const uint32_t *order_count, unsigned char *ws_base = nullptr,
                                                  const uint64_t *ws_off = nullptr, double *trace = nullptr) {
    // `blk`: the workgroup's index among those of its session (blockIdx.x, less the segment's first workgroup in a merged launch;
    // the global-workspace kernels are never merged and read blockIdx.x itself: their code stays what it was).
    // workgroups are dispatched in blockIdx order: `order` lists the chunks with the longest chains first (their
    // length is 20 x 2000 x n proposals per candidate k), so that on ragged batches the kernel does not end on a
    // long chain that started late.  `order_count`, if given, is the device-side length of the list (the grid is the
    // upper bound the host knows).
    if (order_count && (HUGE ? blockIdx.x : blk) >= uni(*order_count)) return;
    const uint32_t seg_log = uni(seg_log_in);  // the ring's geometry: JTK_SEG_LOG_LIGHT / _GENERAL
    const uint32_t ci = order ? order[HUGE ? blockIdx.x : blk] : (HUGE ? blockIdx.x : blk), lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    ChunkState *st = &state[ci];
    if (st->status != 0) return;
    const ChunkMeta cm = chunks[ci];
    // everything that steers control flow is made provably wave-uniform (scalar registers, scalar branches)
    const uint32_t n = uni(cm.n_reads), D = uni(st->dim), copy_num = uni(cm.copy_num);
    const double coverage = unif64(params->haploid_coverage);
    uint32_t *label = label_all + cm.read_first;
    double *post = post_all + (uint64_t)cm.read_first * post_stride;
    // ---- trivial outcomes (pseudo_mcmc.rs:86-88, :221-225)
    if (copy_num < 2 || D == 0 || n <= copy_num) {
        if (wave != 0) return;
        for (uint32_t i = lane; i < n; i += 64) {
            label[i] = 0;
            for (uint32_t c = 0; c < post_stride; c++) post[(uint64_t)i * post_stride + c] = 0.0;
        }
        if (lane == 0) {
            st->score = 0.0;
            st->k = 1;
            st->draws = 0;
        }
        return;
    }
    if (copy_num > JTK_MAX_COPY || copy_num > lds_k || (!HUGE && n > JTK_MAX_PILEUP) || n > lds_n || D > lds_d) {
        if (threadIdx.x == 0) st->status = JTK_ERR_UNSUPPORTED;
        return;
    }
    // ---- LDS carve (again after every out-of-line call: the pointers are cheaper to re-make than to keep alive across it)
    (void)flags;
    // (mcmc_kernel_huge: lds_n / lds_d / lds_k are this chunk's own sizes and size its slice of the global workspace)
    const LdsShape shape = {HUGE ? n : lds_n, HUGE ? D : lds_d, HUGE ? (copy_num < 2 ? 2u : copy_num) : lds_k, seg_log,
                            HUGE ? (uint64_t)(uintptr_t)(ws_base + ws_off[blockIdx.x]) : 0ull};
    Lds m = lds_carve<HUGE>(shape);
    if (threadIdx.x == 0) {
        lds_st32(&m.ctl->rd, 0);
        lds_st32(&m.ctl->quit, 0);
        lds_st32(&m.ctl->wr, 0);
        lds_st32(&m.ctl->wp, 0);
        lds_st32(&m.ctl->parse_n, n);
        lds_st32(&m.ctl->parse_from, 0);
        lds_st32(&m.ctl->pmode, 0);      // no records until a chain asks for them (rng_set_parse_mode)
        lds_st32(&m.ctl->wp_epoch, 0);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    if (wave == 1) {  // Xoshiro256StarStar::seed_from_u64(chunk.id * 3490)  (local_clustering/mod.rs:97)
        producer_main(m.ctl, m.ring, m.rec, seg_log, uni64(cm.chunk_id) * 3490ULL,
                      rng_resume ? rng_resume + 4 * (uint64_t)ci : nullptr, lane);
        return;
    }
    const double *feat = feat_all + cm.feat_off;
    // LKCount::{add,sub} assert `x.abs() < POS_THR` for a value that is neither above POS_THR nor below -POS_THR
    // (:830,:841: exactly +-POS_THR, or NaN), and mcmc_with_filter asserts that its size table has no NaN (:714-715:
    // x ln(lambda) - lambda - ln x! is NaN at x = 0 unless 0 < lambda < inf): the reference panics, the chunk fails.
    bool bad_value = false;
    for (uint32_t e = lane; e < n * D; e += 64) {
        const double x = feat[e];
        m.data[e] = x;
        bad_value = bad_value || (!(JTK_POS_THR < x) && !(x < -JTK_POS_THR) && !(fabs(x) < JTK_POS_THR));
    }
    if (ubool(__ballot(bad_value) != 0ull) || !(coverage > 0.0 && coverage < __builtin_inf())) {
        if (lane == 0) {
            lds_st32(&m.ctl->quit, 1);
            st->status = JTK_ERR_CHUNK_FAILED;
        }
        return;
    }
    // lfact[x] = sum_{c=1..x} ln c, summed left to right as poisson_lk does (:636-638)
    if (lane == 0) {
        double s = 0.0;
        m.lfact[0] = 0.0;
        for (uint32_t c = 1; c <= n; c++) {
            s += jtk_log((double)c);
            m.lfact[c] = s;
        }
    }
    for (uint32_t d = lane; d < D; d += 64) m.prev_used[d] = 0;
    for (uint32_t i = lane; i < n; i += 64) m.accepted[i] = 0;
    if (lane < K2_STAT_SLOTS) m.k2_stats[lane] = 0;
    const unsigned long long chain_t0 = __builtin_readcyclecounter();
    wsync();
    const uint32_t *vt = vtype_all + 2 * ((uint64_t)ci * JTK_MAX_DIM);
    if (vt_stride_mode) vt = vtype_all + 2 * vt_off_all[ci];
    // ---- per-chunk RNG (local_clustering/mod.rs:97): the consumer's position in the producer's stream
    Rng rng;
    rng.pos = 0;
    rng.wr_seen = 0;
    rng.wp_seen = 0;
    rng.pmode = 0;
    rng.win_base = 0xffffff00u;  // nothing held yet
    rng.seg_log = seg_log;
    rng.win = 0;
    JTK_STAT(rng.waits = 0;)
    rng.ctl = m.ctl;
    rng.ring = m.ring;
    rng.rec = m.rec;
    // ---- cluster_filtered_variants (:213-274)
    const double per_cluster_cov = unif64(cm.local_coverage);
    double max = 0.0;
    uint32_t max_k = 1;
    const uint32_t end = copy_num < 1 + 2 * D ? copy_num : 1 + 2 * D;
    const uint32_t start = (end > 5 ? end : 5) - 3;
    bool failed = false;
    uint32_t trace_n = 0;  // (TRACE) records written
    if constexpr (TRACE) {
        if (lane == 0) {
            trace[0] = (double)start;
            trace[1] = (double)end;
            trace[2] = 0.0;
        }
        for (uint32_t i = lane; i < n; i += 64) trace[JTK_TRACE_OLD + i] = 0.0;
        wsync();
    }
    for (uint32_t k = start; k <= end; k++) {
        double score;
        const bool ran = run_k_dyn<LIGHT, HUGE>(k, shape, n, D, coverage, rng, &score, lane);
        m = lds_carve<HUGE>(shape);
        if (!ran) {
            failed = true;
            break;
        }
        // result of this k: labels m.best, gains m.fbuf (unused downstream), used columns m.used
        if (k == 2) {
            // use_highest_gain (:673-693)
            double gbest = 0.0;
            uint32_t max_idx = 0;
            for (uint32_t d = 0; d < D; d++) {
                double gsum = 0.0;
                for (uint32_t i = 0; i < n; i++) gsum += jtk_fmax(m.data[i * D + d], 0.0);
                if (d == 0 || !(gsum < gbest)) {
                    gbest = gsum;
                    max_idx = d;
                }
            }
            for (uint32_t i = lane; i < n; i += 64) m.tmp_asn[i] = 0.0 < m.data[i * D + max_idx] ? 1 : 0;
            wsync();
            // keep the mcmc result aside: fbuf is overwritten by get_read_lk_gains
            get_read_lk_gains<2>(m, n, D, m.tmp_asn, m.tmp_used, lane);
            double hscore = 0.0;
            for (uint32_t i = 0; i < n; i++) hscore += m.fbuf[i];
            if (score < hscore) {
                score = hscore;
                for (uint32_t i = lane; i < n; i += 64) m.best[i] = m.tmp_asn[i];
                for (uint32_t d = lane; d < D; d += 64) m.used[d] = m.tmp_used[d];
                wsync();
            }
        }
        // expected_gains (:286-306)
        bool no_new = true;
        for (uint32_t d = 0; d < D; d++) no_new = no_new && (m.prev_used[d] == m.used[d]);
        double expt = 0.0;
        for (uint32_t d = 0; d < D; d++) {
            const bool check = ((!m.prev_used[d]) && m.used[d]) || no_new;
            const double v = check ? gains_expected(&params->gains, vt[2 * d], (int)vt[2 * d + 1]) : 0.0000001;
            if (d == 0 || !(v < expt)) expt = v;
        }
        const double expected_gain = jtk_fmax(0.8 * expt, 0.1) * per_cluster_cov + 0.1;
        if constexpr (TRACE) {
            // new_lk_gains of the clustering this k ended with (at k == 2 fbuf may hold the other candidate's): get_read_lk_gains of
            // m.best once more, then min_gain (:276-284: first minimum, the value only) and count_improved_reads (:308-312)
            read_lk_gains_dyn(k, m, n, D, m.best, m.tmp_used, lane);
            double min_gain = 1.0;
            bool have_min = false;
            for (uint32_t d = 0; d < D; d++)
                if (m.used[d]) {
                    const double v = gains_expected(&params->gains, vt[2 * d], (int)vt[2 * d + 1]) / 3.0;
                    if (!have_min || v < min_gain) min_gain = v;
                    have_min = true;
                }
            uint32_t improved = 0;
            for (uint32_t i = 0; i < n; i++) improved += trace[JTK_TRACE_OLD + i] + min_gain < m.fbuf[i] ? 1u : 0u;
            const bool accept = expected_gain < score - max;
            double *rec = trace + JTK_TRACE_REC + (uint64_t)trace_n * JTK_TRACE_REC_LEN;
            if (lane == 0 && trace_n < 8) {
                rec[0] = (double)k;
                rec[1] = score;
                rec[2] = expected_gain;
                rec[3] = (double)improved;
                rec[4] = accept ? 1.0 : 0.0;
                for (uint32_t c = 0; c < k; c++) {
                    uint32_t cnt = 0;
                    for (uint32_t i = 0; i < n; i++) cnt += m.best[i] == c ? 1u : 0u;
                    rec[5 + c] = (double)cnt;
                }
                trace[2] = (double)(trace_n + 1);
            }
            trace_n++;
            if (accept)
                for (uint32_t i = lane; i < n; i += 64) trace[JTK_TRACE_OLD + i] = m.fbuf[i];
            wsync();
        }
        if (expected_gain < score - max) {
            wsync();
            for (uint32_t i = lane; i < n; i += 64) m.accepted[i] = m.best[i];
            for (uint32_t d = lane; d < D; d += 64) m.prev_used[d] = m.used[d];
            max = score;
            max_k = k;
            wsync();
        } else {
            break;
        }
    }
    // stop the producer wave
    if (lane == 0) {
        lds_st32(&m.ctl->quit, 1);
        st->draws = rng.pos;  // stream positions consumed: where the chunk's next clustering() call resumes
        st->chain_cycles = __builtin_readcyclecounter() - chain_t0;
        st->chain_events = (uint32_t)m.k2_stats[16];
    }
    JTK_STAT(if (lane == 0) printf("K2WAIT chunk %u waits %u\n", ci, rng.waits);)
    JTK_STAT(if (lane == 0) printf("K2STAT chunk %u n %u D %u cyc %llu walk %llu win %llu event %llu rebuild %llu steps %llu windows %llu events %llu accepts %llu changed %llu head %llu bern %llu book %llu tables %llu hops %llu exact %llu\n",
                    ci, n, D, m.k2_stats[0], m.k2_stats[1], m.k2_stats[2], m.k2_stats[3], m.k2_stats[4], m.k2_stats[5], m.k2_stats[6],
                    m.k2_stats[7], m.k2_stats[8], m.k2_stats[9], m.k2_stats[10], m.k2_stats[11], m.k2_stats[12], m.k2_stats[13], m.k2_stats[14], m.k2_stats[15]);)
    if (failed) {
        if (lane == 0) st->status = JTK_ERR_CHUNK_FAILED;
        return;
    }
    // ---- likelihood gains of the accepted clustering, re-assignment, posterior (:272, :98-105, :342-347)
    double *lg = lg_all + lg_off[ci];  // n x max_k
    likelihood_gain_dyn<LIGHT>(max_k, m, n, D, m.accepted, lg, lane);
    __threadfence_block();
    for (uint32_t i = lane; i < n; i += 64) {
        double *lks = lg + (uint64_t)i * max_k;
        uint32_t asn = m.accepted[i], bi = 0;
        for (uint32_t c = 1; c < max_k; c++)
            if (!(lks[c] < lks[bi])) bi = c;
        if (lks[asn] + 0.001 < lks[bi]) asn = bi;
        // logsumexp (misc.rs:84-92)
        double mx = lks[0];
        for (uint32_t c = 1; c < max_k; c++)
            if (!(lks[c] < mx)) mx = lks[c];
        double sum = 0.0;
        for (uint32_t c = 0; c < max_k; c++) sum += jtk_exp(lks[c] - mx);
        const double total = mx + jtk_log(sum);
        label[i] = asn;
        for (uint32_t c = 0; c < post_stride; c++)
            post[(uint64_t)i * post_stride + c] = c < max_k ? lks[c] - total : 0.0;
    }
    if (lane == 0) {
        st->score = max;
        st->k = max_k;
    }
}

#define MCMC_KERNEL_PARAMS                                                                                                  \
    const ChunkMeta *chunks, ChunkState *state, const jtk_lc_params_t *params, const double *feat_all,                      \
        const uint32_t *vtype_all, const uint64_t *vt_off_all, uint32_t vt_stride_mode, uint32_t *label_all,                \
        double *post_all, uint32_t post_stride, double *lg_all, const uint64_t *lg_off, uint32_t lds_n, uint32_t lds_d,     \
        uint32_t lds_k, uint32_t seg_log, uint32_t flags, const uint64_t *rng_resume, const uint32_t *order,                \
        const uint32_t *order_count
#define MCMC_KERNEL_ARGS                                                                                                    \
    chunks, state, params, feat_all, vtype_all, vt_off_all, vt_stride_mode, label_all, post_all, post_stride, lg_all,       \
        lg_off, lds_n, lds_d, lds_k, seg_log, flags, rng_resume, order, order_count
// The LDS chain kernels take their arguments as a table of segments, by value: one segment per session of a merged launch
// (launch_mcmc_merged), each MCMC_KERNEL_PARAMS of that session plus the launch's first workgroup that belongs to it.  A
// workgroup finds its segment by a scan of the (at most JTK_MCMC_MAX_SEGMENTS) first workgroups -- scalar loads from the
// kernel-argument segment -- and runs mcmc_body on that segment's pointers, with its index inside the segment as `blk`.
// lds_n / lds_d / lds_k describe the LAYOUT of the work area and stay per segment; the launch's dynamic LDS is the largest need.
struct ChainSeg {
    const ChunkMeta *chunks;
    ChunkState *state;
    const jtk_lc_params_t *params;
    const double *feat_all;
    const uint32_t *vtype_all;
    const uint64_t *vt_off_all;
    uint32_t *label_all;
    double *post_all;
    double *lg_all;
    const uint64_t *lg_off;
    const uint64_t *rng_resume;
    const uint32_t *order, *order_count;
    uint32_t vt_stride_mode, post_stride, lds_n, lds_d, lds_k, wg0;
    // Completion of the segment by itself (McmcSegment, device_common.h): every workgroup of the segment adds one to *done as
    // its last act; the one that brings it to done_target stores done_pass to *done_word, a word of the session's pinned page.
    // done == null: nobody counts.
    uint32_t *done, *done_word;
    uint32_t done_target, done_pass;
};
struct ChainSegTable {
    ChainSeg seg[JTK_MCMC_MAX_SEGMENTS];
    uint32_t n, seg_log, flags;
};
template <bool LIGHT>
__device__ __forceinline__ void mcmc_segment_body(const ChainSegTable &t) {
    uint32_t i = 0;
    for (uint32_t j = 1; j < JTK_MCMC_MAX_SEGMENTS; j++)
        if (j < t.n && blockIdx.x >= t.seg[j].wg0) i = j;
    const ChainSeg &g = t.seg[i];
    mcmc_body<LIGHT>(blockIdx.x - g.wg0, g.chunks, g.state, g.params, g.feat_all, g.vtype_all, g.vt_off_all, g.vt_stride_mode,
                     g.label_all, g.post_all, g.post_stride, g.lg_all, g.lg_off, g.lds_n, g.lds_d, g.lds_k, t.seg_log, t.flags,
                     g.rng_resume, g.order, g.order_count);
    // Every path out of the body ends here, both waves, the workgroups past the device-side list length too: the workgroup's
    // stores are out at system scope, then it counts once.  Nothing waits for the count; all of it is read again from the
    // kernel-argument segment, where the body's registers are dead.
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0 && g.done) {
        const uint32_t before = __hip_atomic_fetch_add(g.done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (before + 1u == g.done_target) __hip_atomic_store(g.done_word, g.done_pass, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
__global__ __launch_bounds__(128, JTK_MCMC_WAVES) void mcmc_kernel(const ChainSegTable t) { mcmc_segment_body<false>(t); }
// Pile-ups whose work area does not fit a CU's LDS, or of more than JTK_MAX_PILEUP reads: the per-read arrays live in a
// global-memory workspace (ws_base + ws_off[block]), the chain is the one-proposal-per-iteration one.  One wave per SIMD: the
// seven inlined instantiations of that chain need ~360 registers, and nothing here is built for speed.
__global__ __launch_bounds__(128, 1) void mcmc_kernel_huge(MCMC_KERNEL_PARAMS, unsigned char *ws_base, const uint64_t *ws_off) {
    mcmc_body<false, true>(blockIdx.x, MCMC_KERNEL_ARGS, ws_base, ws_off);
}
// jtk_lc_session_trace: ONE chunk through the global-workspace body (any pile-up size), with the trace records
__global__ __launch_bounds__(128, 1) void mcmc_kernel_trace(MCMC_KERNEL_PARAMS, unsigned char *ws_base, const uint64_t *ws_off,
                                                            double *trace) {
    mcmc_body<false, true, true>(blockIdx.x, MCMC_KERNEL_ARGS, ws_base, ws_off, trace);
}
#ifndef JTK_MCMC_LIGHT_WAVES
#ifdef JTK_MCMC_STATS
#define JTK_MCMC_LIGHT_WAVES 2  // the statistics build prints from the kernel body: it does not fit 168 registers
#else
#define JTK_MCMC_LIGHT_WAVES 3
#endif
#endif
__global__ __launch_bounds__(128, JTK_MCMC_LIGHT_WAVES) void mcmc_kernel_light(const ChainSegTable t) { mcmc_segment_body<true>(t); }

// One wave splits a launch's chunk list (order[] or 0 .. count-1) into the chunks the light kernel can run and the rest,
// keeping the order (longest chain first) in both: out = counts[2] | light[count] | heavy[count].  Chunks with a trivial
// outcome (no variant column, failed earlier, copy number < 2) go to the light list: they return at once in either kernel.
// One workgroup per segment of a merged launch.
struct SplitSeg {
    uint32_t count;
    const uint32_t *order;
    const ChunkMeta *chunks;
    const ChunkState *state;
    uint32_t *out;
};
struct SplitSegTable {
    SplitSeg seg[JTK_MCMC_MAX_SEGMENTS];
};
__global__ __launch_bounds__(64) void chain_split_kernel(const SplitSegTable t) {
    const SplitSeg &g = t.seg[blockIdx.x];
    const uint32_t count = g.count;
    const uint32_t *order = g.order;
    const ChunkMeta *chunks = g.chunks;
    const ChunkState *state = g.state;
    uint32_t *out = g.out;
    const uint32_t lane = threadIdx.x;
    uint32_t *light = out + 2, *heavy = out + 2 + count;
    uint32_t nl = 0, nh = 0;
    for (uint32_t base = 0; base < count; base += 64) {
        const uint32_t idx = base + lane;
        const bool valid = idx < count;
        uint32_t ci = 0;
        bool is_light = false;
        if (valid) {
            ci = order ? order[idx] : idx;
            const uint32_t n = chunks[ci].n_reads, copy_num = chunks[ci].copy_num, D = state[ci].dim;
            const bool trivial = state[ci].status != 0 || copy_num < 2 || D == 0 || n <= copy_num;
            is_light = trivial || (copy_num == 2 && n <= JTK_LIGHT_MAX_READS && D <= JTK_LIGHT_MAX_DIM);
        }
        const uint64_t ml = __ballot(valid && is_light), mh = __ballot(valid && !is_light);
        const uint64_t below = (1ull << lane) - 1ull;
        if (valid) {
            if (is_light) light[nl + __popcll(ml & below)] = ci;
            else heavy[nh + __popcll(mh & below)] = ci;
        }
        nl += __popcll(ml);
        nh += __popcll(mh);
    }
    if (lane == 0) {
        out[0] = nl;
        out[1] = nh;
    }
}

}  // namespace

// One chain launch for the segments of `seg` (device_common.h: McmcSegment): per segment `split` is 2 + 2 * n_chunks words of
// device scratch, or null.  With it the launch is two kernels: the light one (168 registers, the diploid chunks of <= 127
// reads (JTK_LIGHT_MAX_READS) with <= 2 variant columns) and the general one for the rest; without it (or with rng_resume,
// either only in a launch of ONE segment) the general kernel runs everything.  `side` (with its two events), if given, is a
// second stream the general kernel runs on, beside the light one instead of before it.
int launch_mcmc_merged(hipStream_t s, int n_seg, const McmcSegment *seg, hipStream_t side, hipEvent_t ev_fork, hipEvent_t ev_join) {
    if (n_seg < 1 || n_seg > JTK_MCMC_MAX_SEGMENTS) return -1;
    bool plain = false;
    for (int i = 0; i < n_seg; i++) plain = plain || !seg[i].split || seg[i].rng_resume;
    if (plain && n_seg != 1) return -1;
    ChainSegTable general, light;
    SplitSegTable sp;
    memset(&general, 0, sizeof general);
    memset(&sp, 0, sizeof sp);
    uint32_t grid = 0;
    size_t lds = 0, lds_light = 0;
    for (int i = 0; i < n_seg; i++) {
        const McmcSegment &x = seg[i];
        const uint32_t lds_k = clamp_k(x.lds_k);
        ChainSeg &g = general.seg[i];
        g = ChainSeg{x.chunks, x.state, x.params, x.feat, x.vtype, x.vt_off, x.label, x.post, x.lg, x.lg_off, x.rng_resume, x.order,
                     nullptr, x.vt_stride_mode, x.post_stride, x.lds_n, x.lds_d, lds_k, grid, x.done, x.done_word, x.done_target, x.done_pass};
        lds = std::max(lds, mcmc_lds_core(x.lds_n, x.lds_d, lds_k, JTK_SEG_LOG_GENERAL));  // the general kernel: a 12 KiB ring
        grid += x.n_chunks;
    }
    general.n = (uint32_t)n_seg;
    general.seg_log = JTK_SEG_LOG_GENERAL;
    if (grid == 0) return 0;
    if (mcmc_upload_jump_table() != 0) return -1;  // the caller fails the call: nothing was launched
    if (plain) {
        mcmc_kernel<<<grid, 128, lds, s>>>(general);
        return 0;
    }
    light = general;
    light.seg_log = JTK_SEG_LOG_LIGHT;
    for (int i = 0; i < n_seg; i++) {
        const McmcSegment &x = seg[i];
        sp.seg[i] = SplitSeg{x.n_chunks, x.order, x.chunks, x.state, x.split};
        ChainSeg &g = general.seg[i], &l = light.seg[i];
        g.rng_resume = l.rng_resume = nullptr;
        g.order = x.split + 2 + x.n_chunks;
        g.order_count = x.split + 1;
        l.order = x.split + 2;
        l.order_count = x.split;
        l.lds_n = std::min<uint32_t>(x.lds_n, JTK_LIGHT_MAX_READS);
        l.lds_d = std::min<uint32_t>(x.lds_d, JTK_LIGHT_MAX_DIM);
        l.lds_k = 2u;
        lds_light = std::max(lds_light, mcmc_lds_bytes(l.lds_n, l.lds_d, 2));
    }
    chain_split_kernel<<<n_seg, 64, 0, s>>>(sp);
    hipStream_t hs = s;
    if (side && ev_fork && ev_join && hipEventRecord(ev_fork, s) == hipSuccess &&
        hipStreamWaitEvent(side, ev_fork, 0) == hipSuccess)
        hs = side;
    mcmc_kernel<<<grid, 128, lds, hs>>>(general);
    mcmc_kernel_light<<<grid, 128, lds_light, s>>>(light);
    if (hs != s) {
        if (hipEventRecord(ev_join, hs) != hipSuccess || hipStreamWaitEvent(s, ev_join, 0) != hipSuccess) return -1;
    }
    return 0;
}

int launch_mcmc(hipStream_t s, uint32_t n_chunks, const ChunkMeta *chunks, ChunkState *state,
                const jtk_lc_params_t *params, const double *feat, const uint32_t *vtype, const uint64_t *vt_off,
                uint32_t vt_stride_mode, uint32_t *label, double *post, uint32_t post_stride, double *lg,
                const uint64_t *lg_off, uint32_t lds_n, uint32_t lds_d, uint32_t lds_k, const uint64_t *rng_resume,
                const uint32_t *order, uint32_t *split, hipStream_t side, hipEvent_t ev_fork, hipEvent_t ev_join) {
    const McmcSegment seg = {n_chunks, chunks, state, params, feat, vtype, vt_off, vt_stride_mode, label, post, post_stride, lg,
                             lg_off, lds_n, lds_d, lds_k, rng_resume, order, split};
    return launch_mcmc_merged(s, 1, &seg, side, ev_fork, ev_join);
}

// The chunks listed in `order` (one workgroup each) through mcmc_kernel_huge; ws_off[i] = offset of order[i]'s slice of `ws`
// (mcmc_ws_bytes of ITS reads, columns and copy number).
int launch_mcmc_huge(hipStream_t s, uint32_t n_chunks, const ChunkMeta *chunks, ChunkState *state, const jtk_lc_params_t *params,
                     const double *feat, const uint32_t *vtype, const uint64_t *vt_off, uint32_t vt_stride_mode, uint32_t *label,
                     double *post, uint32_t post_stride, double *lg, const uint64_t *lg_off, uint32_t max_n, uint32_t max_d,
                     uint32_t max_k, const uint64_t *rng_resume, const uint32_t *order, unsigned char *ws, const uint64_t *ws_off) {
    if (n_chunks == 0) return 0;
    if (mcmc_upload_jump_table() != 0) return -1;
    mcmc_kernel_huge<<<n_chunks, 128, mcmc_lds_fixed() + JTK_HUGE_LDS, s>>>(chunks, state, params, feat, vtype, vt_off, vt_stride_mode, label, post,
                                                             post_stride, lg, lg_off, max_n, max_d, clamp_k(max_k), JTK_SEG_LOG_LIGHT, 0u,
                                                             rng_resume, order, nullptr, ws, ws_off);
    return 0;
}

// jtk_lc_session_trace: the chunk listed in order[0] once more through mcmc_kernel_trace (its results come out as they were);
// `trace` = mcmc_trace_doubles(n) doubles, `ws` = mcmc_ws_bytes of the chunk, ws_off[0] = 0.
size_t mcmc_trace_doubles(uint32_t n_reads) { return (size_t)JTK_TRACE_OLD + n_reads; }
int launch_mcmc_trace(hipStream_t s, const ChunkMeta *chunks, ChunkState *state, const jtk_lc_params_t *params, const double *feat,
                      const uint32_t *vtype, uint32_t *label, double *post, uint32_t post_stride, double *lg, const uint64_t *lg_off,
                      uint32_t n, uint32_t d, uint32_t k, const uint32_t *order, unsigned char *ws, const uint64_t *ws_off,
                      double *trace) {
    if (mcmc_upload_jump_table() != 0) return -1;
    mcmc_kernel_trace<<<1, 128, mcmc_lds_fixed() + JTK_HUGE_LDS, s>>>(chunks, state, params, feat, vtype, nullptr, 0u, label, post, post_stride,
                                                                     lg, lg_off, n, d, clamp_k(k), JTK_SEG_LOG_LIGHT, 0u, nullptr,
                                                                     order, nullptr, ws, ws_off, trace);
    return 0;
}
