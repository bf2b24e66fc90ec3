// chain_generic.h -- included by mcmc_kernels.hip alone: mcmc_chain, one proposal per iteration for any K.
#pragma once

namespace {

// mcmc_with_filter (:704-762), generic in K, one proposal per iteration.  m.assign holds the k-means labels on entry, the
// best-seen labels on exit.  This is the chain of mcmc_kernel_huge: pile-ups of more than JTK_MAX_PILEUP reads, or whose work
// area exceeds a CU's LDS -- there the per-read arrays of `m` point into a GLOBAL-memory workspace (every access below goes
// through generic pointers), the 10-bit read indices of the table-driven chains do not apply, and speed is not the point:
// clustering_on_pileup (local_clustering/mod.rs:86-123) takes any depth, so this library does too.
template <int K, bool SMALL>
__device__ __forceinline__ double mcmc_chain(const Lds &m, uint32_t n, uint32_t D, double cov, Rng &rng, uint32_t lane) {
    // size_to_lk[x] = max_{c=1..K} poisson_lk(x, cov*c)
    LaneTab size_to_lk;
#pragma unroll
    for (int r = 0; r < (SMALL ? 1 : 4); r++) {
        const uint32_t x = lane + 64 * r;
        double mx = -__builtin_inf();
        if (x <= n)
            for (int c = 1; c <= K; c++) {
                const double lam = cov * (double)c;
                mx = jtk_fmax(mx, (double)x * jtk_log(lam) - lam - m.lfact[x]);
            }
        size_to_lk.v[r] = mx;
    }
    // Pile-ups of more than 255 reads (high copy numbers: 8 copies x 40 reads) do not fit the four-register tables:
    // sizes and labels then live in LDS (m.size_to_lk, m.assign in place, m.argmax), one extra round trip per look-up.
    const bool big = !SMALL && n > 255u;
    if (big) {
        for (uint32_t x = lane; x <= n; x += 64) {
            double mx = -__builtin_inf();
            for (int c = 1; c <= K; c++) {
                const double lam = cov * (double)c;
                mx = jtk_fmax(mx, (double)x * jtk_log(lam) - lam - m.lfact[x]);
            }
            m.size_to_lk[x] = mx;
        }
        wsync();
    }
    auto size_lk = [&](uint32_t x) -> double { return big ? unif64(m.size_to_lk[x]) : tab_get<SMALL>(size_to_lk, x); };
    // ---- initial LKCounts in the reference's order (reads outer)
    double tg[K];
    int np[K], w[K], cl[K];
#pragma unroll
    for (int c = 0; c < K; c++) {
        tg[c] = 0.0;
        np[c] = 0;
        w[c] = 0;
        cl[c] = 0;
    }
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t c = uni(m.assign[i]);
        Elem el = {0.0, 0, 0};
        if (lane < D) el = elem_of(m.data[i * D + lane]);
#pragma unroll
        for (int cc = 0; cc < K; cc++)
            if ((uint32_t)cc == c) {
                tg[cc] += el.x;
                np[cc] += el.dp;
                w[cc] += el.pw;
                cl[cc]++;
            }
    }
    int totp = 0;  // reads with a positive value in this column: sum_c num_pos[c], constant along the chain
    unsigned long long posm[K], infm[K];
    const unsigned long long colm = D >= 64 ? ~0ull : ((1ull << D) - 1ull);
#pragma unroll
    for (int c = 0; c < K; c++) {
        totp += np[c];
        posm[c] = __ballot(0.0 < tg[c]) & colm;
        infm[c] = __ballot(w[c] > 0);
    }
    LaneLabels assign, argmax;
#pragma unroll
    for (int r = 0; r < (SMALL ? 1 : 4); r++) {
        const uint32_t i = lane + 64 * r;
        assign.v[r] = i < n ? (int)m.assign[i] : 0;
        argmax.v[r] = assign.v[r];
    }
    if (big) {
        for (uint32_t i = lane; i < n; i += 64) m.argmax[i] = m.assign[i];
        wsync();
    }
    // get_lk (:785-795) on a tentative state: size terms first, then clusters outer / columns inner, left to
    // right; exactly-zero terms (unused column or total_gain <= 0) leave the f64 sum unchanged and are skipped.
    auto get_lk = [&](const double *T, const int *P, const int *cls, const unsigned long long *pm,
                      const unsigned long long *im) -> double {
        double S = 0.0;
#pragma unroll
        for (int c = 0; c < K; c++) S += size_lk((uint32_t)cls[c]);
        int in_use = 0;
        unsigned long long anym = 0;
#pragma unroll
        for (int c = 0; c < K; c++) {
            in_use += (0.0 < T[c]) ? P[c] : 0;
            anym |= pm[c] & im[c];  // some cluster is_informative (:818-822) on this column
        }
        // get_used_columns (:847-869): informative somewhere, and 2 * pos_in_neg < pos_in_use
        const unsigned long long usedm = __ballot(3 * in_use > 2 * totp) & anym;
#pragma unroll
        for (int c = 0; c < K; c++) {
            unsigned long long mm = usedm & pm[c];
            while (mm) {
                const uint32_t d = (uint32_t)__builtin_ctzll(mm);
                mm &= mm - 1;
                S += readlane_f64(T[c], d);
            }
        }
        return S;
    };
    // The same quantity without the ordering (any order of the same terms: off by ~1e-12 at most).  The ordered sum
    // costs a v_readlane + a dependent add per term; this costs one cross-lane reduction, and it is enough to see
    // that a proposal is certainly rejected -- which > 96% of them are.
    // (its size terms come from three small per-cluster tables -- the entry of the current size, of one read less and
    // of one read more -- kept up to date on the rare accepts: no table look-up per proposal)
    double sz0[K], szm[K], szp[K];
    auto size_terms = [&](int c) {
        const uint32_t x = (uint32_t)cl[c];
        sz0[c] = size_lk(x);
        szm[c] = x > 0 ? size_lk(x - 1) : 0.0;
        szp[c] = x < n ? size_lk(x + 1) : 0.0;
    };
#pragma unroll
    for (int c = 0; c < K; c++) size_terms(c);
    auto approx_lk = [&](const double *T, const int *P, uint32_t from, uint32_t to, const unsigned long long *pm,
                         const unsigned long long *im) -> double {
        double S = 0.0;
#pragma unroll
        for (int c = 0; c < K; c++) S += (uint32_t)c == from ? szm[c] : ((uint32_t)c == to ? szp[c] : sz0[c]);
        int in_use = 0;
        unsigned long long anym = 0;
#pragma unroll
        for (int c = 0; c < K; c++) {
            in_use += (0.0 < T[c]) ? P[c] : 0;
            anym |= pm[c] & im[c];
        }
        const unsigned long long usedm = __ballot(3 * in_use > 2 * totp) & anym;
        const bool used = (usedm >> lane) & 1ull;
        double loc = 0.0;
#pragma unroll
        for (int c = 0; c < K; c++) loc += (used && 0.0 < T[c]) ? T[c] : 0.0;
        return S + wave_sum_f64(loc);
    };
    double lk = get_lk(tg, np, cl, posm, infm);
    double max = lk;
    const uint32_t total = 2000u * n;
    JTK_STAT(unsigned long long gs[6] = {0, 0, 0, 0, 0, 0};)
    // Proposals are parsed from the 64-draw register window, not draw by draw.  A proposal is gen_range(0..n) -- the
    // first draw at or after its start whose widening product passes the zone test -- and then, for i = 1..K-1,
    // gen_index(i) on the upper halves of the following draws, each with its own zone test; the pick is the last i
    // whose index came out 0 (choose_pos).  Which draws pass which test, and which give index 0, depends on the draws
    // only: one ballot each per window, after which a proposal is a few scalar shift / find-first-set steps instead of
    // ~6 rejection loops on values that have to cross from the vector to the scalar side one at a time.
    uint32_t wp_base = 0xfffffff0u, wp_hi = 0;
    unsigned long long wp_ok0 = 0, wp_ok[K], wp_z[K];
#pragma unroll
    for (int i = 0; i < K; i++) wp_ok[i] = wp_z[i] = 0;
    const uint64_t zone_n = ((uint64_t)n << __clzll((long long)n)) - 1;
    for (uint32_t t = 0; t < total; t++) {
        JTK_STAT(unsigned long long gs_t = __builtin_readcyclecounter();)
        uint32_t idx = 0, pos = 0;
        {
            uint32_t off = rng.pos - rng.win_base;
            if (off >= 40u) {  // keep 24 draws of look-ahead: reload the window at the current position
                rng_refill(rng);
                off = 0;
            }
            if (wp_base != rng.win_base) {
                const uint64_t v = rng.win;
                const uint32_t v32 = (uint32_t)(v >> 32);
                wp_hi = (uint32_t)__umul64hi(v, (uint64_t)n);
                wp_ok0 = __ballot(v * (uint64_t)n <= zone_n);
#pragma unroll
                for (int i = 1; i < K; i++) {
                    const uint32_t zone = ((uint32_t)i << __builtin_clz((uint32_t)i)) - 1u;
                    const uint64_t mi = (uint64_t)v32 * (uint32_t)i;
                    wp_ok[i] = __ballot((uint32_t)mi <= zone);
                    wp_z[i] = __ballot((uint32_t)(mi >> 32) == 0u);
                }
                wp_base = rng.win_base;
            }
            const unsigned long long m0 = wp_ok0 >> off;
            bool good = m0 != 0ull;
            const uint32_t p0 = off + (uint32_t)__builtin_ctzll(m0 | (1ull << 63));
            uint32_t q = p0;
#pragma unroll
            for (int i = 1; i < K; i++) {
                const unsigned long long mm = (good && q < 63u) ? wp_ok[i] >> (q + 1u) : 0ull;
                good = good && mm != 0ull;
                q = (q + 1u + (uint32_t)__builtin_ctzll(mm | (1ull << 63))) & 63u;
                if ((wp_z[i] >> q) & 1ull) pos = (uint32_t)i - 1u;
            }
            if (good) {
                idx = (uint32_t)__builtin_amdgcn_readlane((int)wp_hi, (int)p0);
                rng.pos = rng.win_base + q + 1u;
            } else {  // the proposal runs past the window: draw by draw
                idx = (uint32_t)gen_range_usize(rng, n);
                pos = choose_pos(rng, K);
            }
        }
        const uint32_t old = big ? uni((uint32_t)m.assign[idx]) : lab_get<SMALL>(assign, idx);
        const uint32_t nw = pos < old ? pos : pos + 1;
        GS_MARK(0);
        Elem el = {0.0, 0, 0};
        if (lane < D) el = elem_of(m.data[idx * D + lane]);
        // ---- tentative flip (:764-783): only the two touched clusters change
        double T[K];
        int P[K], W[K], ncl[K];
        unsigned long long npm[K], nim[K];
#pragma unroll
        for (int c = 0; c < K; c++) {
            const bool o = (uint32_t)c == old, a = (uint32_t)c == nw;
            T[c] = tg[c];
            P[c] = np[c];
            W[c] = w[c];
            ncl[c] = cl[c];
            npm[c] = posm[c];
            nim[c] = infm[c];
            if (o) {
                T[c] = tg[c] - el.x;
                P[c] = np[c] - el.dp;
                W[c] = w[c] - el.pw;
                ncl[c] = cl[c] - 1;
            }
            if (a) {
                T[c] = tg[c] + el.x;
                P[c] = np[c] + el.dp;
                W[c] = w[c] + el.pw;
                ncl[c] = cl[c] + 1;
            }
            if (o || a) {
                npm[c] = __ballot(0.0 < T[c]) & colm;
                nim[c] = __ballot(W[c] > 0);
            }
        }
        // estimate first: if proposed - lk is below -1e-3 the step certainly draws, and the draw usually settles it
        double proposed = 0.0;
        bool accept = false, decided = false, have_v = false;
        uint64_t v = 0;
        GS_MARK(1);
        const double dA = unif64(approx_lk(T, P, old, nw, npm, nim) - lk);
        GS_MARK(2);
        if (ubool(dA < -1e-3)) {
            v = next_u64(rng);
            have_v = true;
            const float u = (float)(uint32_t)(v >> 40) * 0x1p-24f;  // v / 2^64 within 2^-24
            decided = ubool(dA <= -44.5 || u > __expf((float)dA) * 1.001f + 3e-7f);  // certainly rejected
        }
        GS_MARK(3);
        if (!decided) {
            JTK_STAT(gs[5]++;)
            proposed = get_lk(T, P, ncl, npm, nim);
            const double diff = unif64(proposed - lk);
            // `0f64 < diff || rng.gen_bool(diff.exp())` (:736): gen_bool(1.0) draws nothing, and exp(diff) == 1.0
            // exactly when diff >= -2^-54 (never the case when the estimate was below -1e-3)
            accept = true;
            if (!ubool(diff >= -0x1p-54)) accept = bernoulli_exact(have_v ? v : next_u64(rng), diff);
        }
        if (accept) {
#pragma unroll
            for (int c = 0; c < K; c++) {
                tg[c] = T[c];
                np[c] = P[c];
                w[c] = W[c];
                cl[c] = ncl[c];
                posm[c] = npm[c];
                infm[c] = nim[c];
                if ((uint32_t)c == old || (uint32_t)c == nw) size_terms(c);
            }
            if (big) {
                if (lane == 0) m.assign[idx] = (uint8_t)nw;
                wsync();
            } else {
                lab_set<SMALL>(assign, idx, nw, lane);
            }
            lk = proposed;
            if (ubool(max < lk)) {
                max = proposed;
                argmax = assign;
                if (big) {
                    for (uint32_t i = lane; i < n; i += 64) m.argmax[i] = m.assign[i];
                    wsync();
                }
            }
        } else {
            // flip back (:746): the reference re-adds / re-subtracts, which leaves rounding residue
#pragma unroll
            for (int c = 0; c < K; c++) {
                if ((uint32_t)c == old) tg[c] = T[c] + el.x;
                if ((uint32_t)c == nw) tg[c] = T[c] - el.x;
            }
        }
        GS_MARK(4);
    }
    JTK_STAT(if (lane == 0) printf("GENSTAT K %d n %u D %u steps %u draws %llu flip %llu approx %llu decide %llu tail %llu exact %llu\n",
                    K, n, D, total, gs[0], gs[1], gs[2], gs[3], gs[4], gs[5]);)
    wsync();
    if (big) {
        for (uint32_t i = lane; i < n; i += 64) m.assign[i] = m.argmax[i];
    } else {
#pragma unroll
        for (int r = 0; r < (SMALL ? 1 : 4); r++) {
            const uint32_t i = lane + 64 * r;
            if (i < n) m.assign[i] = (uint8_t)argmax.v[r];
        }
    }
    wsync();
    return max;
}

}  // namespace
