// chain_k2.h -- included by mcmc_kernels.hip alone: mcmc_chain_k2, the diploid chain, its hop words and walk_rejected.
#pragma once

namespace {

// ---- the diploid chain (round 5).
//
// Lane i of the consumer holds READ i (and read 64 + i when NR == 2): its row, signed by the direction of its flip, and --
// rebuilt lane-parallel after every move of the state -- the EXACT likelihood of the state with that read flipped (get_lk's
// own left-to-right sum) and whether flip + flip-back would leave a rounding residue.  Both go to a 16-byte entry per read
// in LDS.  A window is 64 consecutive stream positions (lane l = position base + l): the producer's record of the proposal
// that WOULD start there (read index, length, 19 bits of its Bernoulli draw); per window the known bits of the draw become
// two thresholds in the log domain, and the hop word of a position follows from its read's entry: diff = proposed - lk below
// the one: certainly rejected, above the other: certainly accepted.  The walk follows the hop words over proposals that are
// certainly rejected and leave nothing behind; everything else is an event, settled from the hop word (the exact exp only
// inside the guard bands) and the read's lane.  The state (LKCount[c][d] of the two clusters) is wave-uniform and replicated
// in every lane: neither the event nor the re-evaluation needs a cross-lane operation.  Size-only moves (all-zero rows) are
// not a special case: the size terms are where every lane's sum starts.
//
// The hop word of window position l (one v_readlane per hop yields all of it):
//   bits 0..5 nxt[l] | 64 skip: inside the window, certainly rejected, no residue | 128 certainly accepted
//   | 256 accepted without a draw | 512 certainly rejected | 1024 not in this window | 2048 a rejected flip leaves a residue
#define HW_SKIP 64u
#define HW_ACC 128u
#define HW_NODRAW 256u
#define HW_REJ 512u
#define HW_OUT 1024u
#define HW_PERT 2048u
#define HW_CROSS 4096u   // (round 6) the proposal ends in the NEXT block of 64 positions: bits 0..5 are its end there
#define HW_SKIPX 8192u   // ... and is certainly rejected without a residue (== HW_SKIP << 7: never both)
typedef __attribute__((address_space(3))) const volatile double lds_cvf64;
typedef __attribute__((address_space(3))) const volatile u32x4_t lds_cvu32x4;
typedef __attribute__((address_space(3))) volatile u32x4_t lds_vu32x4;
__device__ __forceinline__ uint32_t lds_addr(const void *p) {  // LDS byte address (a generic pointer indexed per lane costs a
    return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const char *)p;  // 64-bit add and a null check per access)
}
// Walks from window position p over skippable proposals; returns the number of steps taken (<= limit) and the hop word it
// stopped at.  Straight-line hops with forward exits: a taken branch costs a lone wave far more than the hop itself.
__device__ __forceinline__ uint32_t walk_rejected(uint32_t hopw, uint32_t &p, uint32_t limit, uint32_t &hv_out) {
    uint32_t hv = 0;
    if (limit >= 24) {  // a window holds at most 21 proposals: no need to watch the step budget
        uint32_t steps = 22;
#pragma unroll
        for (uint32_t k = 0; k < 22; k++) {
            hv = uni((uint32_t)__builtin_amdgcn_readlane((int)hopw, (int)p));
            if (!(hv & HW_SKIP)) {
                steps = k;
                break;
            }
            p = hv & 63u;
        }
        hv_out = hv;
        return steps;
    }
    uint32_t steps = 0;
    while (steps < limit) {
        hv = uni((uint32_t)__builtin_amdgcn_readlane((int)hopw, (int)p));
        if (!(hv & HW_SKIP)) break;
        p = hv & 63u;
        steps++;
    }
    hv_out = hv;
    return steps;
}
// One proposal taken with scalar draws (a start the producer could not parse): the read index and the stream
// position of the draw a Bernoulli test would compare.
__device__ __forceinline__ void scalar_proposal(Rng &rng, uint32_t start, uint32_t n, uint32_t &idx, uint32_t &pos_v) {
    rng.pos = start;
    idx = (uint32_t)gen_range_usize(rng, n);
    (void)gen_index(rng, 1);  // choose() over the single other cluster (pseudo_mcmc.rs:732)
    pos_v = rng.pos;
}

// Out of line on purpose: inlined into the kernel, the chain inherits the register pressure of everything that is
// live around it and spills scalar registers inside its loop (each reload is a v_readlane on the critical path).
struct K2Mem {
    const double *data;  // n x D likelihood gains
    const double *lfact;
    uint8_t *assign;
    double *tab;         // 16 n bytes: one entry per read (the k-means scratch fbuf + cum: idle during a chain)
    unsigned long long *k2_stats;
};
template <typename T>
__device__ __forceinline__ T *uni_ptr(T *p) { return reinterpret_cast<T *>((uintptr_t)uni64((uint64_t)(uintptr_t)p)); }
// NR: registers per per-read / per-size table: 1 serves n <= 63, 2 serves n <= 127 (read or size 64 r + lane)
template <int DMAX, int NR>
__device__ __attribute__((noinline)) double mcmc_chain_k2(K2Mem m_in, uint32_t n_in, uint32_t D_in, double cov_in, Rng *rng_io,
                                                          uint32_t lane) {
    // Arguments of an out-of-line function arrive in vector registers and the compiler then treats everything derived from
    // them -- the step counter, the window position, every branch of the event -- as divergent (exec-mask regions instead
    // of scalar branches): all of it is re-made wave-uniform here.
    const uint32_t n = uni(n_in), D = uni(D_in);
    const double cov = unif64(cov_in);
    const K2Mem m = {uni_ptr(m_in.data), uni_ptr(m_in.lfact), uni_ptr(m_in.assign), uni_ptr(m_in.tab), uni_ptr(m_in.k2_stats)};
    Rng rng = *rng_io;
    rng.pos = uni(rng.pos);
    rng.wr_seen = uni(rng.wr_seen);
    rng.wp_seen = uni(rng.wp_seen);
    rng.pmode = uni(rng.pmode);
    rng.win_base = uni(rng.win_base);
    rng.seg_log = uni(rng.seg_log);
    const uint32_t rn_mask = RN_OF(rng.seg_log) - 1u;
    rng.ctl = uni_ptr(rng.ctl);
    rng.ring = uni_ptr(rng.ring);
    rng.rec = uni_ptr(rng.rec);
    const uint32_t rec_lds = uni(lds_addr(rng.rec)), data_lds = uni(lds_addr(m.data)), tab_lds = uni(lds_addr(m.tab));
    // pair table: lane c0 holds (0.0 + size_to_lk[c0]) + size_to_lk[n - c0]   (get_lk :788)
    double pair_v[NR];
    auto tab64 = [&](const double *tab, uint32_t i) -> double {  // entry i of a per-lane table of NR registers
        return NR == 2 && i >= 64 ? readlane_f64(tab[NR - 1], i & 63u) : readlane_f64(tab[0], i & 63u);
    };
    auto bit128 = [&](const unsigned long long *mk, uint32_t i) -> bool {
        return ((NR == 2 && i >= 64 ? mk[NR - 1] : mk[0]) >> (i & 63u)) & 1ull;
    };
    {
        auto size_lk = [&](uint32_t x) {
            double mx = -__builtin_inf();
            for (int c = 1; c <= 2; c++) {
                const double lam = cov * (double)c;
                mx = jtk_fmax(mx, (double)x * jtk_log(lam) - lam - m.lfact[x]);
            }
            return mx;
        };
#pragma unroll
        for (int r = 0; r < NR; r++) {
            const uint32_t c = lane + 64 * r, cc = c <= n ? c : n;
            pair_v[r] = (0.0 + size_lk(cc)) + size_lk(n - cc);
        }
    }
    // ---- exact state LKCount[c][d]; columns >= D are all-zero, never used and add +0.0.  The two counters travel
    //      packed: pk = num_pos + 65536 * (3*num_pos - 7*num_neg), so pk > 0xffff <=> the second one is positive.
    double tg0[DMAX], tg1[DMAX];
    int pk0[DMAX], pk1[DMAX], tp2[DMAX];
#pragma unroll
    for (int d = 0; d < DMAX; d++) {
        tg0[d] = tg1[d] = 0.0;
        pk0[d] = pk1[d] = tp2[d] = 0;
    }
    uint32_t c0 = 0;
    unsigned long long lab[NR];
#pragma unroll
    for (int r = 0; r < NR; r++) lab[r] = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t c = uni(m.assign[i]);
#pragma unroll
        for (int d = 0; d < DMAX; d++) {
            Elem el = {0.0, 0, 0};
            if ((uint32_t)d < D) el = elem_of(unif64(m.data[i * D + d]));
            tp2[d] += 2 * el.dp;  // 2 x reads with a positive value in this column: constant along the chain
            if (c == 0) {
                tg0[d] += el.x;
                pk0[d] += el.dp + 65536 * el.pw;
            } else {
                tg1[d] += el.x;
                pk1[d] += el.dp + 65536 * el.pw;
            }
        }
        if (c == 0)
            c0++;
        else if (NR == 2 && i >= 64)
            lab[NR - 1] |= 1ull << (i & 63u);
        else
            lab[0] |= 1ull << (i & 63u);
    }
    // ---- the rows of reads lane, 64 + lane, signed by the direction of their flip: sx[r][d] is what cluster 0 would gain
    double sx[NR][DMAX];
    int spk[NR][DMAX];
#pragma unroll
    for (int r = 0; r < NR; r++) {
        const uint32_t ri = lane + 64 * r < n ? lane + 64 * r : 0;
        const bool a = bit128(lab, ri);
#pragma unroll
        for (int d = 0; d < DMAX; d++) {
            Elem el = {0.0, 0, 0};
            if ((uint32_t)d < D) el = elem_of(*(lds_cvf64 *)(uintptr_t)(data_lds + ((ri * D + (uint32_t)d) << 3)));
            const int kk = el.dp + 65536 * el.pw;
            sx[r][d] = a ? el.x : -el.x;
            spk[r][d] = a ? kk : -kk;
        }
    }
    wsync();
    auto pair_at = [&](uint32_t c) -> double { return tab64(pair_v, c <= n ? c : n); };
    // get_lk (:785-795) of the state in which a read with the signed row (x, k), sitting in cluster 1 iff `a`, is flipped --
    // exactly: the size terms, then clusters outer / columns inner, left to right -- and whether flip + flip-back (:746)
    // would leave a rounding residue in the sums
    double pair_up, pair_dn;
    auto flipped_lk = [&](const double *x, const int *k, bool a, double &S_out, bool &pert_out) {
        double t1[DMAX];
        double S = a ? pair_up : pair_dn;
        bool pert = false;
#pragma unroll
        for (int d = 0; d < DMAX; d++) {
            const double T0 = tg0[d] + x[d], T1 = tg1[d] - x[d];  // s - x == s + (-x) bit for bit
            const int K0 = pk0[d] + k[d], K1 = pk1[d] - k[d];
            const bool pos0 = 0.0 < T0, pos1 = 0.0 < T1;
            const int m0 = pos0 ? K0 : 0, m1 = pos1 ? K1 : 0;
            // get_used_columns (:847-869): some cluster is informative, and the positives sit where the gain is
            const bool used = (m0 > m1 ? m0 : m1) > 0xffff && 3 * ((m0 + m1) & 0xffff) > tp2[d];
            S += (used && pos0) ? T0 : 0.0;
            t1[d] = (used && pos1) ? T1 : 0.0;
            pert = pert || (T0 - x[d] != tg0[d]) || (T1 + x[d] != tg1[d]);
        }
#pragma unroll
        for (int d = 0; d < DMAX; d++) S += t1[d];
        S_out = S;
        pert_out = pert;
    };
    // get_lk of the start state: the same sum with nothing flipped
    double lk;
    {
        double t0[DMAX], t1[DMAX];
#pragma unroll
        for (int d = 0; d < DMAX; d++) {
            const bool pos0 = 0.0 < tg0[d], pos1 = 0.0 < tg1[d];
            const int in_use = ((pos0 ? pk0[d] : 0) + (pos1 ? pk1[d] : 0)) & 0xffff;
            const bool any = (pos0 && pk0[d] > 0xffff) || (pos1 && pk1[d] > 0xffff);
            const bool used = any && 3 * in_use > tp2[d];
            t0[d] = (used && pos0) ? tg0[d] : 0.0;
            t1[d] = (used && pos1) ? tg1[d] : 0.0;
        }
        double S = pair_at(c0);
#pragma unroll
        for (int d = 0; d < DMAX; d++) S += t0[d];
#pragma unroll
        for (int d = 0; d < DMAX; d++) S += t1[d];
        lk = unif64(S);
    }
    pair_up = pair_at(c0 + 1);
    pair_dn = pair_at(c0 > 0 ? c0 - 1 : 0);
    // ---- per read, for the current state: prop_l = get_lk with the read flipped; its entry in LDS: diff = prop_l - lk (the
    //      quantity `0f64 < diff || rng.gen_bool(diff.exp())` (:736) decides on, as f32), the hop-word bits that hold if the draw is
    //      above exp(diff) (.z), and those that hold anyway (.w: gen_bool(1.0) draws nothing, and exp(diff) == 1.0 exactly
    //      when diff >= -2^-54; the residue flag)
    double prop_l[NR];
    auto evaluate = [&]() {
#pragma unroll
        for (int r = 0; r < NR; r++) {
            bool pert;
            flipped_lk(sx[r], spk[r], __builtin_amdgcn_inverse_ballot_w64(lab[r]), prop_l[r], pert);
            const double diff = prop_l[r] - lk;
            u32x4_t e;
            e.x = __float_as_uint((float)diff);  // (rounded: within 3e-6 of diff wherever a threshold can lie -- the guard bands are 2e-3)
            e.y = 0;
            e.z = pert ? HW_REJ : HW_REJ | HW_SKIP;
            e.w = (diff >= -0x1p-54 ? HW_NODRAW : 0u) | (pert ? HW_PERT : 0u);
            if (lane + 64 * r < n) *(lds_vu32x4 *)(uintptr_t)(tab_lds + ((lane + 64 * r) << 4)) = e;
        }
    };
    // ---- the window.  Round 6: a window is a BLOCK of 64 consecutive stream positions, and the next block follows at + 64 whatever
    //      the proposals do (rounds 1-5: the next window started where the first proposal that did not end inside the window
    //      began, so nothing of it could be fetched before the walk had got there).  A proposal that starts in a block and ends in
    //      the next one is described by its own record like any other; its hop word carries HW_CROSS and, where it could have
    //      been stepped over, HW_SKIPX instead of HW_SKIP: the walk stops at it, counts it and goes on in the next block.  A
    //      block's look-up of its reads' entries is in flight while its two logarithms are computed, every position of the
    //      stream belongs to exactly one block (a window used to re-read the tail of its predecessor), and the move itself is
    //      ~60 instructions.  Solo chains -7 .. -10 % (profiles/r06_chain_solo.txt); requesting the next block's records a block
    //      ahead adds nothing: the chain is now bound by its producer wave (and the general kernel, whose ring holds 1,024
    //      positions, loses 9 %: its consumer then waits for the producer 64 positions earlier in every superblock).
    uint32_t w_base = 0;          // stream position of lane 0
    uint32_t w_idx = 0, w_w0 = 0; // per lane: the read the proposal starting here picks; its end (mod 64) | HW_CROSS, or HW_OUT
    float w_lrej = 0.0f, w_lacc = 0.0f;  // per lane: diff below w_lrej: certainly rejected; above w_lacc: certainly accepted
    uint32_t hopw = 0;
    uint32_t n_blocks = 0;        // (statistics build: windows loaded)
    auto hop_finish = [&](const u32x4_t tv) {
        const float diff = __uint_as_float(tv.x);
        // (tv.y is always 0 (evaluate).  It is OR-ed in so that all four registers of the 16-byte load stay live until the entry is
        // used: the compiler otherwise hands the dead one to the arithmetic that follows the load's issue, and the hardware then
        // has to wait for the load before that arithmetic may start)
        const uint32_t h = w_w0 | tv.w | tv.y | (diff < w_lrej ? tv.z : 0u) | (diff > w_lacc ? HW_ACC : 0u);
        hopw = (h & HW_CROSS) ? ((h & ~HW_SKIP) | ((h & HW_SKIP) << 7)) : h;
    };
    auto hop_words = [&]() { hop_finish(*(lds_cvu32x4 *)(uintptr_t)(tab_lds + (w_idx << 4))); };
    // the block whose records are `r`: per-lane registers and hop words (the entries of the block's reads are requested first,
    // the thresholds are computed while they are on their way)
    auto block_setup = [&](const uint32_t r) {
        w_idx = r & 127u;
        const u32x4_t tv = *(lds_cvu32x4 *)(uintptr_t)(tab_lds + (w_idx << 4));
        const uint32_t len = (r >> 7) & 63u, nxt = lane + len;
        const bool parsed = len != 0;
        w_w0 = parsed ? ((nxt & 63u) | (nxt >= 64u ? HW_CROSS : 0u)) : HW_OUT;
        // The 19 known bits u of the Bernoulli draw (its true value / 2^64 lies in [u, u + 2^-19)) against exp(diff), in the
        // log domain, with guard bands far wider than the errors of the hardware logarithm (v_log_f32: 1 ulp of a number below
        // 100, then one multiplication: < 2e-5) and of diff's rounding to f32 (< 3e-6 where a threshold can lie):
        //   diff < ln(u - 1.3e-6) - 2e-3  =>  exp(diff) * 1.002 < u - 1.3e-6: the draw is above p: rejected;  below -44.39
        //                                     exp(diff) * 2^64 < 1 (2^64 = e^44.3614), p_int == 0: rejected whatever the draw
        //   diff > ln(u + 2^-19 + 3e-7) + 2e-3  =>  exp(diff) > 1.002 (u + 2^-19 + 3e-7): the draw is below p: accepted
        const float u = (float)(r >> 13) * 0x1p-19f;
        const float lr = __builtin_amdgcn_logf(fmaxf(u - 1.3e-6f, 1e-30f)) * 0.6931472f - 2e-3f;  // (operands are normal numbers)
        const float la = __builtin_amdgcn_logf(u + (0x1p-19f + 3e-7f)) * 0.6931472f + 2e-3f;
        w_lrej = parsed ? fmaxf(lr, -44.39f) : -__builtin_inff();
        w_lacc = parsed ? la : __builtin_inff();
        hop_finish(tv);
    };
    // the records of [base, base + 128) exist and may not be overwritten
    auto block_claim = [&](uint32_t base) {
        rng.pos = base;
        rng_release(rng, lane);
        rng_wait_rec(rng, base + 64u);  // the block's own records, read when it is entered
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        w_base = base;
    };
    auto block_first = [&](uint32_t base) {   // the chain's first block, or the one behind a proposal with scalar draws that went far
        block_claim(base);
        const uint32_t r = *(lds_vu32 *)(uintptr_t)(rec_lds + (((base + lane) & rn_mask) << 2));
        block_setup(r);
        n_blocks++;
    };
    auto block_advance = [&]() {              // on to the block at w_base + 64
        block_claim(w_base + 64u);
        const uint32_t r = *(lds_vu32 *)(uintptr_t)(rec_lds + (((w_base + lane) & rn_mask) << 2));
        block_setup(r);
        n_blocks++;
    };
    double max = lk;
    unsigned long long argmax[NR];
#pragma unroll
    for (int r = 0; r < NR; r++) argmax[r] = lab[r];
    evaluate();
    const uint32_t total = 2000u * n;
    uint32_t t = 0, p = 0;
    uint32_t n_events = 0;  // (reported per chunk: jtk_lc_debug_chain_profile)
    ST_T0();
    block_first(rng.pos);
    for (;;) {
        // ---- the walk, across blocks, up to the next proposal that cannot be skipped.  An inner loop of its own: it
        //      writes the window's registers and nothing of the chain's state, so the event below meets the back edge
        //      without a block of register moves between them.
        uint32_t hv = 0;
        bool done = false;
        for (;;) {
            if (t >= total) {
                done = true;
                break;
            }
            t += walk_rejected(hopw, p, total - t, hv);
            if (t >= total) {
                done = true;
                break;
            }
            if (!(hv & HW_SKIPX)) break;
            t++;             // certainly rejected, nothing left behind, ends in the next block: counted, and the walk goes on there
            p = hv & 63u;
            block_advance();
        }
        if (done) break;
        JTK_STAT(const unsigned long long g0c = __builtin_readcyclecounter();)
        ST_MARK0();
        uint32_t e_idx, pos_v;  // the read it picks; stream position of the draw a Bernoulli test would compare
        if (!(hv & HW_OUT)) {
            e_idx = uni((uint32_t)__builtin_amdgcn_readlane((int)w_idx, (int)p));
            pos_v = w_base + (hv & 63u) + ((hv & HW_CROSS) ? 64u : 0u) - 1;
        } else {
            // the producer could not parse this one (it needs more look-ahead than it has, p ~ 2^-14): scalar draws and the
            // exact Bernoulli test
            scalar_proposal(rng, w_base + p, n, e_idx, pos_v);
            const u32x4_t tv = *(lds_cvu32x4 *)(uintptr_t)(tab_lds + (e_idx << 4));
            hv = HW_OUT | uni(tv.w);
        }
        // the read's lane: the likelihood of the flipped state and the read's signed row
        double proposed, x0[DMAX];
        int k0[DMAX];
        if (NR == 2 && e_idx >= 64) {
            proposed = readlane_f64(prop_l[NR - 1], e_idx & 63u);
#pragma unroll
            for (int d = 0; d < DMAX; d++) {
                x0[d] = readlane_f64(sx[NR - 1][d], e_idx & 63u);
                k0[d] = __builtin_amdgcn_readlane(spk[NR - 1][d], (int)(e_idx & 63u));
            }
        } else {
            proposed = readlane_f64(prop_l[0], e_idx & 63u);
#pragma unroll
            for (int d = 0; d < DMAX; d++) {
                x0[d] = readlane_f64(sx[0][d], e_idx & 63u);
                k0[d] = __builtin_amdgcn_readlane(spk[0][d], (int)(e_idx & 63u));
            }
        }
        ST_MARK(10);
        n_events++;
        uint32_t accept = (hv & (HW_NODRAW | HW_ACC)) ? 1u : 0u;
        if (!(hv & (HW_NODRAW | HW_ACC | HW_REJ))) {  // inside the guard bands (or a start without a record): the exact test
            rng_wait(rng, pos_v + 1);
            accept = ubool(bernoulli_exact(uni64(lds_ld64(&rng.ring[ring_slot(pos_v, rng.seg_log)])), proposed - lk)) ? 1u : 0u;  // (an out-of-line call returns in a vector register)
            ST_CNT(15, 1);
        }
        ST_MARK(11);
        uint32_t moved = 0;
        if (accept) {
#pragma unroll
            for (int d = 0; d < DMAX; d++) {
                tg0[d] = tg0[d] + x0[d];
                tg1[d] = tg1[d] - x0[d];
                pk0[d] += k0[d];
                pk1[d] -= k0[d];
            }
            const unsigned long long bit = 1ull << (e_idx & 63u);
            if (NR == 2 && e_idx >= 64) {
                c0 = (lab[NR - 1] & bit) ? c0 + 1 : c0 - 1;
                lab[NR - 1] ^= bit;
            } else {
                c0 = (lab[0] & bit) ? c0 + 1 : c0 - 1;  // the read sat in cluster 1: cluster 0 grows
                lab[0] ^= bit;
            }
            pair_up = pair_at(c0 + 1);
            pair_dn = pair_at(c0 > 0 ? c0 - 1 : 0);
            lk = proposed;
            if (ubool(max < lk)) {
                max = proposed;
#pragma unroll
                for (int r = 0; r < NR; r++) argmax[r] = lab[r];
            }
#pragma unroll
            for (int r = 0; r < NR; r++) {  // the read now flips the other way
                const bool mine = lane + 64 * r == e_idx;
#pragma unroll
                for (int d = 0; d < DMAX; d++) {
                    sx[r][d] = mine ? -sx[r][d] : sx[r][d];
                    spk[r][d] = mine ? -spk[r][d] : spk[r][d];
                }
            }
            moved = 1;
        } else if (hv & HW_PERT) {
            // flip back (:746) keeps the rounding residue: the sums move although nothing was accepted
#pragma unroll
            for (int d = 0; d < DMAX; d++) {
                tg0[d] = (tg0[d] + x0[d]) - x0[d];
                tg1[d] = (tg1[d] - x0[d]) + x0[d];
            }
            moved = 1;
        }
        t++;
        const uint32_t pos_next = pos_v + 1 - ((hv / HW_NODRAW) & 1u);
        ST_CNT(7, 1);
        ST_CNT(8, accept);
        ST_CNT(9, moved);
        ST_MARK(12);
        if (moved) evaluate();
        ST_MARK(13);
        const uint32_t off_next = pos_next - w_base;
        if (off_next >= 128u) {        // (only behind scalar draws that went on for more than a block)
            block_first(pos_next);
            p = 0;
        } else if (off_next >= 64u) {  // the entries are up to date (evaluate above): the new block's hop words are made from them
            p = off_next - 64u;
            block_advance();
        } else {
            p = off_next;
            if (moved) hop_words();
        }
        ST_MARK(14);
        ST_CNT(4, __builtin_readcyclecounter() - g0c);
    }
    ST_CNT(5, total);
    ST_CNT(6, n_blocks);
    ST_ADD(0);
    if (lane == 0) m.k2_stats[16] += n_events;
    rng.pos = w_base + p;
    rng_release(rng, lane);
#pragma unroll
    for (int r = 0; r < NR; r++)
        if (lane + 64 * r < n) m.assign[lane + 64 * r] = (uint8_t)((argmax[r] >> lane) & 1ull);
    wsync();
    *rng_io = rng;
    return max;
}

}  // namespace
