// chain_tab.h -- included by mcmc_kernels.hip alone: mcmc_chain_tab, the table-driven chain for any K, and its window.
#pragma once

namespace {

// The table-driven chain for any K (mcmc_chain_tab): K > 2, and the diploid pile-ups the fast path below does not take.
//
// As in the diploid chain, more than 96 % of the proposals are rejected, and the fate of "move read i from cluster a to
// cluster b" is a function of the state.  The producer wave has parsed the proposal that WOULD start at every stream
// position into a record (producer_parse_gen); for a window of 64 records the consumer evaluates, one proposal per lane,
// a REJECTION THRESHOLD and then steps from proposal to proposal with one v_readlane each:
//  * certainly rejected (the uniform behind its Bernoulli draw exceeds the threshold): the step is the reference's
//    flip + flip-back on the two touched clusters' sums -- (tg - x) + x and (tg + x) - x, rounding residue included --
//    and nothing else;
//  * anything else is an EVENT: one exact step with the reference's arithmetic (ordered left-to-right get_lk, exact exp
//    only if the guarded f32 test cannot decide), exactly as mcmc_chain does it.
// The threshold comes from an estimate of proposed - lk that is SEPARABLE: as long as the move flips no `0 < total_gain`
// and no column's used / unused status, get_lk changes by  s[b][i] - s[a][i]  (s[c][i] = sum of x[i][d] over the columns d
// that are used and where cluster c has a positive sum: LDS, rebuilt only when that column set changes) plus two size
// terms.  Whether a move can flip anything is certified per column with margins that hold for EVERY read: |total_gain|
// above the column's largest |x|, 3 pos_in_use - 2 total_pos away from 0 by more than one read, an informative cluster that
// stays informative under any +-7 change of its counter.  Columns that fail are collected in per-cluster / global bit
// masks; a proposal whose read has a non-zero value in such a column is never classified (it becomes an event), and
// neither is any proposal while a sum with counts behind it is within 1e-6 of zero (rounding residues, which move sums by
// ulps, could flip its sign).  Thresholds carry a 1e-3 guard band; the masks and s are republished at every accept and at
// least every 65,536 steps.
// Bit-identical to the one-step-at-a-time chain by construction; checked against the oracle.
struct GenWindow {
    uint32_t base;
    uint32_t nxt;   // per lane: window offset of the following proposal (Bernoulli draw taken), 255 = not in this window
    uint32_t ip;    // per lane: read index | pick << 10
    float u;        // per lane: the draw its Bernoulli test compares, / 2^64, truncated to 13 bits
};
__device__ __forceinline__ void gwindow_load(GenWindow &wd, Rng &rng, uint32_t base, uint32_t lane) {
    rng.pos = base;
    rng_release(rng, lane);
    rng_wait_rec(rng, base + 64);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    wd.base = base;
    const uint32_t r = lds_ld32(&rng.rec[(base + lane) & (RN_OF(rng.seg_log) - 1)]);
    const uint32_t len = (r >> 13) & 63u;
    wd.ip = r & 0x1fffu;
    wd.nxt = (len != 0 && lane + len < 64) ? lane + len : 255u;
    wd.u = (float)(r >> 19) * 0x1p-13f;
}
typedef __attribute__((address_space(3))) const volatile uint8_t lds_cvu8;
__device__ __forceinline__ double lds_ld_f64(const double *p) { return jtk_bits_f64(lds_ld64(reinterpret_cast<const uint64_t *>(p))); }
// A pointer into LDS that reached this function through memory (a struct passed by reference, an argument register of an
// out-of-line call) looks divergent to the compiler: every use becomes a flat access with a null check and every branch
// on a value loaded through it an exec-mask region.  Rebuilt from its wave-uniform 32-bit LDS offset it is a scalar.
template <typename T>
__device__ __forceinline__ T *lds_uni(T *p) {
    typedef __attribute__((address_space(3))) char lds_char;
    const uint32_t off = uni((uint32_t)(uintptr_t)(lds_char *)const_cast<typename std::remove_const<T>::type *>(p));
    return (T *)(lds_char *)(uintptr_t)off;
}

template <int K>
__device__ __attribute__((noinline)) double mcmc_chain_tab(LdsShape shape, uint32_t n_in, uint32_t D_in, double cov_in,
                                                           Rng *rng_io, uint32_t lane) {
    // everything that steers control flow or addresses LDS is made provably wave-uniform first (see lds_uni)
    const uint32_t n = uni(n_in), D = uni(D_in);
    const double cov = unif64(cov_in);
    const Lds m = lds_carve(shape);
    Rng rng;
    rng.pos = uni(rng_io->pos);
    rng.wr_seen = uni(rng_io->wr_seen);
    rng.wp_seen = uni(rng_io->wp_seen);
    rng.win_base = uni(rng_io->win_base);
    rng.seg_log = uni(rng_io->seg_log);
    rng.pmode = uni(rng_io->pmode);
    rng.win = rng_io->win;
    JTK_STAT(rng.waits = rng_io->waits;)
    rng.ctl = m.ctl;
    rng.ring = m.ring;
    rng.rec = m.rec;
    const bool small = n <= 63u, big = n > 255u;
    // size_to_lk[x] = max_{c=1..K} poisson_lk(x, cov*c), in LDS whatever n is (round 4: see size_lk below)
    {
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
    // One LDS load, no branch.  Up to round 4 this read the table from its 4 registers for n <= 255 (`tab_get`: a switch on
    // x >> 6 around a pair of v_readlane): nine look-ups per accepted move and K per get_lk, ~8 branches each -- and a taken
    // branch costs a lone wave ~20 cycles: 2,200 -> 730 cycles for the state + size terms of an accept, 1,040 -> 480 for
    // get_lk (K = 2, 160 reads; profiles/r04_tab_event_breakdown.txt).
    auto size_lk = [&](uint32_t x) -> double { return unif64(m.size_to_lk[x]); };
    (void)small;
    (void)big;
    // ---- initial LKCounts in the reference's order (reads outer); lane = column
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
    int totp = 0;
    const unsigned long long colm = D >= 64 ? ~0ull : ((1ull << D) - 1ull);
#pragma unroll
    for (int c = 0; c < K; c++) totp += np[c];
    // labels live in LDS (m.assign, with the best-seen copy in m.argmax): the walk reads a proposal's cluster from its
    // hop word, so only events and the threshold build look labels up
    for (uint32_t i = lane; i < n; i += 64) m.argmax[i] = m.assign[i];
    wsync();
    auto label_of = [&](uint32_t i) -> uint32_t { return uni((uint32_t) * (lds_cvu8 *)(m.assign + i)); };
    // get_lk (:785-795) on a (tentative) state: size terms first, then clusters outer / columns inner, left to right;
    // exactly-zero terms leave the f64 sum unchanged and are skipped
    auto get_lk = [&](const double *T, const int *P, const int *Wt, const int *cls) -> double {
        double S = 0.0;
#pragma unroll
        for (int c = 0; c < K; c++) S += size_lk((uint32_t)cls[c]);
        int in_use = 0;
        unsigned long long anym = 0, pm[K];
#pragma unroll
        for (int c = 0; c < K; c++) {
            pm[c] = __ballot(0.0 < T[c]) & colm;
            in_use += (0.0 < T[c]) ? P[c] : 0;
            anym |= pm[c] & __ballot(Wt[c] > 0);  // some cluster is_informative (:818-822) on this column
        }
        const unsigned long long usedm = __ballot(3 * in_use > 2 * totp) & anym;  // get_used_columns (:847-869)
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
    // (the size terms of the K clusters -- size_to_lk of the size and of its two neighbours -- are looked up where they are
    // used, in publish(): kept in registers across the chain they were 3 K wave-uniform doubles, i.e. 6 K of the ~100 scalar
    // registers, and the chain's loop spilled scalars around every event)
    double lk = get_lk(tg, np, w, cl);
    double max = lk;
    // ---- thresholds (see the header comment).  Per-column constants first: the largest |x| and, per read, the columns
    //      with a non-zero value.
    const uint32_t npad = m.npad;
    typedef __attribute__((address_space(3))) const double lds_cd;
    typedef __attribute__((address_space(3))) double lds_d;
    typedef __attribute__((address_space(3))) uint32_t lds_u32;
    typedef __attribute__((address_space(3))) const uint32_t lds_cu32;
    lds_cd *const data_l = (lds_cd *)m.data;  // 32-bit LDS addressing for the hot gathers
    lds_d *const stab_l = (lds_d *)m.stab;
    lds_u32 *const nz_l = (lds_u32 *)m.nz;
    double xmax = 0.0;  // lane = column
    for (uint32_t i = 0; i < n; i++) {
        const double x = lane < D ? data_l[i * D + lane] : 0.0;
        xmax = fabs(x) > xmax ? fabs(x) : xmax;
    }
    for (uint32_t i = lane; i < n; i += 64) {
        uint32_t z = 0;
        for (uint32_t d = 0; d < D; d++) z |= data_l[i * D + d] != 0.0 ? 1u << d : 0u;
        nz_l[i] = z;
    }
    uint32_t umask[K];  // columns cluster c is paid for: used and total_gain > 0 (what s[c][.] is summed over)
#pragma unroll
    for (int c = 0; c < K; c++) umask[c] = 0xffffffffu;  // "never built"
    uint32_t nrcol = 0;   // columns whose used / unused status a single move could flip
    uint32_t nrun = 0;    // nrcol | every cluster's uncertified columns
    bool fragile = false; // some sum with counts behind it is within 1e-6 of zero
    double C0 = 0.0;      // (order-free get_lk of the current state) - lk: what every estimate starts from
    auto publish = [&]() {
        int IU = 0, AN = 0, RB = 0;
        bool alloff = true, frag = false;
        double G = 0.0;
        uint32_t nr[K], pm[K];
        double sz0[K], szm[K], szp[K];  // (the same value in every lane: LDS broadcast reads)
#pragma unroll
        for (int c = 0; c < K; c++) {
            const uint32_t x = (uint32_t)cl[c];
            sz0[c] = m.size_to_lk[x];
            szm[c] = x > 0 ? m.size_to_lk[x - 1] : 0.0;
            szp[c] = x < n ? m.size_to_lk[x + 1] : 0.0;
        }
#pragma unroll
        for (int c = 0; c < K; c++) {
            const bool pos = 0.0 < tg[c];
            IU += pos ? np[c] : 0;
            AN += (pos && w[c] > 0) ? 1 : 0;
            RB += (pos && w[c] > 7) ? 1 : 0;
            alloff = alloff && (!pos || w[c] <= -7);
            frag = frag || (fabs(tg[c]) < 1e-6 && (np[c] != 0 || w[c] > 0));
            pm[c] = (uint32_t)(__ballot(pos) & colm);
            // `0 < total_gain` of this cluster cannot flip under any single move iff the sum clears the column's largest |x|
            nr[c] = (uint32_t)(__ballot(!(fabs(tg[c]) > xmax + 1e-6)) & colm);
        }
        if (lane < D) {  // the exact state, for the columns a proposal is not certified on (see hop_words)
#pragma unroll
            for (int c = 0; c < K; c++) {
                const uint64_t tb = jtk_f64_bits(tg[c]);
                u32x4 e;
                e.x = (uint32_t)tb;
                e.y = (uint32_t)(tb >> 32);
                e.z = (uint32_t)np[c];
                e.w = (uint32_t)w[c];
                ((lds_u32x4 *)m.st)[lane * K + c] = e;
            }
            u32x4 e;
            e.x = (uint32_t)IU;
            e.y = (uint32_t)AN;
            e.z = (uint32_t)totp;
            e.w = 0;
            ((lds_u32x4 *)m.col)[lane] = e;
        }
        const int v = 3 * IU - 2 * totp;  // used needs v >= 1; one move changes 3 IU by at most 3
        const bool iu_rob = v >= 4 || v <= -3;
        const bool an_rob = RB >= 1 || alloff;  // an informative cluster that stays one, or none that could become one
        const bool used = AN > 0 && v >= 1;
        nrcol = (uint32_t)(__ballot(!(iu_rob && an_rob)) & colm);
        nrun = nrcol;
#pragma unroll
        for (int c = 0; c < K; c++) nrun |= nr[c];
        fragile = __ballot(lane < D && frag) != 0ull;
        const uint32_t usedm = (uint32_t)(__ballot(used) & colm);
#pragma unroll
        for (int c = 0; c < K; c++) G += (used && 0.0 < tg[c]) ? tg[c] : 0.0;
        double S0 = 0.0;
#pragma unroll
        for (int c = 0; c < K; c++) S0 += sz0[c];
        C0 = unif64((S0 + wave_sum_f64(lane < D ? G : 0.0)) - lk);
#pragma unroll
        for (int c = 0; c < K; c++) {
            const uint32_t um = usedm & pm[c];
            if (um != umask[c]) {  // rare once the clusters have formed: rebuild s[c][.]
                umask[c] = um;
                for (uint32_t i = lane; i < n; i += 64) {
                    double sc = 0.0;
                    uint32_t mm = um;
                    while (mm) {
                        const uint32_t d = (uint32_t)__builtin_ctz(mm);
                        mm &= mm - 1;
                        sc += data_l[i * D + d];
                    }
                    stab_l[(uint32_t)c * npad + i] = sc;
                }
            }
            if (lane == 0) {
                SzEnt e;
                e.rem = szm[c] - sz0[c];
                e.add = szp[c] - sz0[c];
                e.nr = nr[c];
                e.um = um;
                e.pad[0] = e.pad[1] = 0;
                lds_put_sz(&m.sz[c], e);
            }
        }
        wsync();
    };
    // per window position: nxt (6 bits) | certainly rejected << 6 | in-window << 7 | read index << 8 | pick << 18 |
    // the read's current cluster << 21 | the cluster the proposal moves it to << 24
    const uint32_t n1 = n - 1;
    auto hop_words = [&](const GenWindow &wd) -> uint32_t {
        uint32_t idx = wd.ip & 1023u;
        uint32_t pick = wd.ip >> 10;
        const bool in = wd.nxt != 255u;
        idx = idx < n1 ? idx : n1;  // a position that is not a parsed proposal may hold anything
        pick = pick < (uint32_t)(K - 1) ? pick : 0u;
        const uint32_t old = *(lds_cvu8 *)(m.assign + idx);
        const uint32_t nw = pick < old ? pick : pick + 1u;
        const SzEnt ea = lds_load_sz(&m.sz[old]), eb = lds_load_sz(&m.sz[nw]);
        const uint32_t z = ((lds_cu32 *)nz_l)[idx];
        // columns this proposal is not certified on: there the change of get_lk is evaluated from the exact state
        const uint32_t F = z & (ea.nr | eb.nr | nrcol);
        bool cant = fragile;
        double corr = 0.0;
        uint32_t any = nrun;  // the columns some proposal could be uncertified on (wave-uniform)
        while (any) {
            const uint32_t d = (uint32_t)__builtin_ctz(any);
            any &= any - 1;
            if (!((F >> d) & 1u)) continue;
            const Elem el = elem_of(data_l[idx * D + d]);
            const u32x4 ce = ((lds_c_u32x4 *)m.col)[d];
            const u32x4 qa = ((lds_c_u32x4 *)m.st)[d * K + old], qb = ((lds_c_u32x4 *)m.st)[d * K + nw];
            const double Ta0 = lo_f64(qa), Tb0 = lo_f64(qb);
            const int Pa = (int)qa.z, Wa = (int)qa.w, Pb = (int)qb.z, Wb = (int)qb.w;
            const bool pa = 0.0 < Ta0, pb = 0.0 < Tb0;
            const double Ta = Ta0 - el.x, Tb = Tb0 + el.x;
            const int Pa2 = Pa - el.dp, Wa2 = Wa - el.pw, Pb2 = Pb + el.dp, Wb2 = Wb + el.pw;
            const bool pa2 = 0.0 < Ta, pb2 = 0.0 < Tb;
            const int IU = (int)ce.x, AN = (int)ce.y, TP = (int)ce.z;
            const bool used0 = AN > 0 && 3 * IU > 2 * TP;
            const int IU2 = IU - (pa ? Pa : 0) - (pb ? Pb : 0) + (pa2 ? Pa2 : 0) + (pb2 ? Pb2 : 0);
            const int AN2 = AN - ((pa && Wa > 0) ? 1 : 0) - ((pb && Wb > 0) ? 1 : 0) + ((pa2 && Wa2 > 0) ? 1 : 0) +
                            ((pb2 && Wb2 > 0) ? 1 : 0);
            const bool used2 = AN2 > 0 && 3 * IU2 > 2 * TP;
            // the two clusters' terms before and after; the other clusters' terms only matter if `used` flips
            const double t0 = used0 ? ((pa ? Ta0 : 0.0) + (pb ? Tb0 : 0.0)) : 0.0;
            const double t2 = used2 ? ((pa2 ? Ta : 0.0) + (pb2 ? Tb : 0.0)) : 0.0;
            if (used0 != used2) cant = true;  // (every other cluster's term switches too: rare, left to the exact step)
            // sums near zero with counts behind them: rounding residues could flip their sign
            cant = cant || (fabs(Ta) < 1e-6 && (Pa2 != 0 || Wa2 > 0)) || (fabs(Tb) < 1e-6 && (Pb2 != 0 || Wb2 > 0));
            // replace the separable contribution of this column by the exact one
            const double sep = (((eb.um >> d) & 1u) ? el.x : 0.0) - (((ea.um >> d) & 1u) ? el.x : 0.0);
            corr += (t2 - t0) - sep;
        }
        const double dA = (((stab_l[nw * npad + idx] - stab_l[old * npad + idx]) + corr) + (ea.rem + eb.add)) + C0;
        const float t = cant ? 2.0f : reject_threshold(dA, false);
        return (wd.nxt & 63u) | ((in && wd.u > t) ? 64u : 0u) | (in ? 128u : 0u) | (idx << 8) | (pick << 18) | (old << 21) | (nw << 24);
    };
    JTK_STAT(unsigned long long ts[13] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};)  // fast, events, accepts, reloads, scalars, cyc rebuild, cyc event, residues, cyc window load, cyc hop words, uncertified columns
    JTK_STAT(const unsigned long long ts_t0 = __builtin_readcyclecounter();)
    publish();
    const uint32_t total = 2000u * n;
    uint32_t t = 0, p = 0, since_rebuild = 0;
    uint32_t n_events = 0;  // (reported per chunk: jtk_lc_debug_chain_profile)
    GenWindow wd;
    gwindow_load(wd, rng, rng.pos, lane);
    uint32_t hopw = hop_words(wd);
    const uint32_t row_lane_addr = (uint32_t)(uintptr_t)data_l + (lane < D ? lane : 0u) * 8u;  // (the rejected steps' hand-issued loads)
    // K <= 4 clusters of <= 16 columns (every BASELINE shape): during the quiet part of the chain the K sums of a column travel in
    // ONE register, lane 16 c + d = cluster c / column d, so that a rejected step is one multiplication and two additions for all
    // clusters, its factor picked per lane (two compares) instead of per cluster (four scalar instructions each).  The exact step
    // and publish() keep their register per cluster: packed on the way into the first block after an event, unpacked before the
    // next event (2 K ds_bpermute each way, against ~4,000 cycles of event).
    const bool packable = K <= 4 && D <= 16u;
    const uint32_t grp = lane >> 4, col16 = lane & 15u;
    const uint32_t row_lane_addr_pk = (uint32_t)(uintptr_t)data_l + (col16 < D ? col16 : 0u) * 8u;
    double tgp = 0.0;
    bool is_packed = false;
    auto pack_sums = [&]() {
        tgp = 0.0;
#pragma unroll
        for (int c = 0; c < K; c++) {
            const double v = __shfl(tg[c], (int)col16, 64);  // (lanes >= D of tg[c] hold +0)
            tgp = grp == (uint32_t)c ? v : tgp;
        }
        is_packed = true;
    };
    auto unpack_sums = [&]() {
#pragma unroll
        for (int c = 0; c < K; c++) {
            const double v = __shfl(tgp, (int)(16u * (uint32_t)c + col16), 64);
            tg[c] = lane < D ? v : 0.0;
        }
        is_packed = false;
    };
    auto row_of = [&](uint32_t hvv) -> double {  // the column values of the read a hop word names (lanes >= D: 0.0)
        uint32_t i = (hvv >> 8) & 1023u;
        i = i < n1 ? i : n1;  // a word that is not a proposal may hold anything
        return lane < D ? data_l[i * D + lane] : 0.0;
    };
    for (;;) {
        // ---- the quiet part, a loop of its own: blocks of certainly rejected proposals and window moves follow one another
        //      without passing the event's code (whose many live values the compiler would otherwise merge at every back edge:
        //      a chain spends ~8 steps per window and ~70 steps per event at K = 3)
        uint32_t hv = 0;
        bool finished = false;
        for (;;) {
        if (t >= total) {
            finished = true;
            break;
        }
        hv = uni((uint32_t)__builtin_amdgcn_readlane((int)hopw, (int)p));
        if ((hv & 192u) == 192u && since_rebuild < 65536u) {
            JTK_STAT(const unsigned long long f_t0 = __builtin_readcyclecounter();)
            // ---- certainly rejected proposals, one after the other: flip + flip back (:739,:746) on the two touched
            //      clusters and nothing else.  The next proposal's hop word and row are fetched before this one's
            //      arithmetic (an LDS round trip costs a lone wave ~100 cycles).  Round 5, from the ISA of the round-4 loop:
            //      (a) `x = xn` at the back edge made every step wait for the row it had just asked for -- the loop is unrolled
            //      twice over two row registers, a step waits for the OLDER load only; (b) 2 K scalar compare-and-branch pairs
            //      picked the two touched sums -- now every cluster's sum takes (s + m) - m with m = x * {-1, +1, 0} (a scalar
            //      factor): x * -1 and x * 1 are exact, (s + -x) - -x is (s - x) + x bit for bit, and m = +-0 leaves s as it is
            //      (no sum is ever -0: they grow from +0 by additions), so the bits are the reference's and nothing branches.
            uint32_t budget = total - t;
            if (budget > 65536u - since_rebuild) budget = 65536u - since_rebuild;
            uint32_t done = 0;
            auto rejected_step = [&](uint32_t hvv, double x, auto use_packed) {
                const uint32_t old = (hvv >> 21) & 7u, nw = (hvv >> 24) & 7u;
                JTK_STAT(bool st_res = false;)
                if (decltype(use_packed)::value) {
                    const uint32_t hi = grp == old ? 0xBFF00000u : (grp == nw ? 0x3FF00000u : 0u);
                    const double mc = x * __hiloint2double((int)hi, 0);
                    TS_ADD(7, __ballot((tgp + mc) - mc != tgp) != 0ull ? 1 : 0);
                    tgp = (tgp + mc) - mc;
                    return;
                }
#pragma unroll
                for (int c = 0; c < K; c++) {
                    const uint32_t hi = (uint32_t)c == old ? 0xBFF00000u : ((uint32_t)c == nw ? 0x3FF00000u : 0u);
                    const double mc = x * __hiloint2double((int)hi, 0);
                    JTK_STAT(st_res = st_res || (tg[c] + mc) - mc != tg[c];)
                    tg[c] = (tg[c] + mc) - mc;
                }
                TS_ADD(7, __ballot(st_res) != 0ull ? 1 : 0);  // rejected steps that leave a rounding residue in some sum
            };
            // The rows travel through hand-issued ds_read_b64 with hand-placed waits: the compiler's own scoreboard waits with
            // lgkmcnt(0) in this loop -- i.e. for the row it has just asked for as well -- where "all but the youngest load"
            // (lgkmcnt(1): LDS loads return in order) is what hides the round trip.  No other LDS access happens between the
            // first load and the drain behind the loop; lanes >= D read column 0 and keep their zero sums ((0 + m) - m == +0).
            auto row_issue = [&](uint32_t hvv, auto use_packed) -> double {
                const uint32_t i = (hvv >> 8) & 1023u;  // (hop_words clamps the index of a position that is not a proposal)
                double v;
                asm volatile("ds_read_b64 %0, %1" : "=v"(v)
                             : "v"((decltype(use_packed)::value ? row_lane_addr_pk : row_lane_addr) + i * (D * 8u)));
                return v;
            };
            // A window holds at most 21 proposals (three draws each at least): with 24 steps of budget left -- always, but at
            // the very end of a chain and once per 65,536 steps -- the block ends with the window and nothing counts steps
            // against the budget (three scalar instructions per step less).
            auto run_block = [&](auto watch_budget, auto use_packed) {
                double xa = row_issue(hv, use_packed), xb;
                for (;;) {
                    uint32_t pn = hv & 63u;
                    uint32_t hn = uni((uint32_t)__builtin_amdgcn_readlane((int)hopw, (int)pn));
                    xb = row_issue(hn, use_packed);
                    asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(xa));  // the older of the two rows in flight
                    rejected_step(hv, xa, use_packed);
                    p = pn;
                    hv = hn;
                    done++;
                    if ((hv & 192u) != 192u) break;
                    if (decltype(watch_budget)::value && done >= budget) break;
                    pn = hv & 63u;
                    hn = uni((uint32_t)__builtin_amdgcn_readlane((int)hopw, (int)pn));
                    xa = row_issue(hn, use_packed);
                    asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(xb));
                    rejected_step(hv, xb, use_packed);
                    p = pn;
                    hv = hn;
                    done++;
                    if ((hv & 192u) != 192u) break;
                    if (decltype(watch_budget)::value && done >= budget) break;
                }
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(xa), "+v"(xb));  // the row fetched for a step that did not run
            };
            if (packable) {
                if (!is_packed) pack_sums();
                if (budget >= 24u)
                    run_block(std::false_type(), std::true_type());
                else
                    run_block(std::true_type(), std::true_type());
            } else if (budget >= 24u) {
                run_block(std::false_type(), std::false_type());
            } else {
                run_block(std::true_type(), std::false_type());
            }
            t += done;
            since_rebuild += done;
            TS_ADD(0, done);
            JTK_STAT(ts[11] += __builtin_readcyclecounter() - f_t0;)   // cycles inside the rejected-steps block
            JTK_STAT(ts[12] += 1;)                                      // its entries
            continue;
        }
        if (!(hv & 128u) && p != 0) {  // the proposal does not end inside this window: move the window there
            JTK_STAT(const unsigned long long w_t0 = __builtin_readcyclecounter();)
            gwindow_load(wd, rng, wd.base + p, lane);
            JTK_STAT(const unsigned long long w_t1 = __builtin_readcyclecounter();)
            p = 0;
            hopw = hop_words(wd);
            TS_ADD(3, 1);
            JTK_STAT(ts[8] += w_t1 - w_t0;)
            JTK_STAT(ts[9] += __builtin_readcyclecounter() - w_t1;)
            JTK_STAT(ts[10] += (unsigned long long)__popc(nrun);)
            continue;
        }
        break;
        }
        if (is_packed) unpack_sums();
        if (finished) break;
        uint32_t idx, pick, pos_v;
        bool reload = false;
        if (hv & 128u) {
            idx = (hv >> 8) & 1023u;
            pick = (hv >> 18) & 7u;
            pos_v = wd.base + (hv & 63u) - 1;
        } else {  // not even at the window start: the producer could not parse this one -- scalar draws
            TS_ADD(4, 1);
            rng.pos = wd.base;
            idx = (uint32_t)gen_range_usize(rng, n);
            pick = choose_pos(rng, K);
            pos_v = rng.pos;
            reload = true;
        }
        // ---- the event: one exact step (as mcmc_chain)
        JTK_STAT(const unsigned long long ev_t0 = __builtin_readcyclecounter();)
        TS_ADD(1, 1);
        n_events++;
        const uint32_t old = label_of(idx);
        const uint32_t nw = pick < old ? pick : pick + 1;
        Elem el = {0.0, 0, 0};
        if (lane < D) el = elem_of(lds_ld_f64(&m.data[idx * D + lane]));
        double T[K];
        int P[K], W[K], ncl[K];
#pragma unroll
        for (int c = 0; c < K; c++) {
            const bool o = (uint32_t)c == old, a = (uint32_t)c == nw;
            T[c] = o ? tg[c] - el.x : (a ? tg[c] + el.x : tg[c]);
            P[c] = o ? np[c] - el.dp : (a ? np[c] + el.dp : np[c]);
            W[c] = o ? w[c] - el.pw : (a ? w[c] + el.pw : w[c]);
            ncl[c] = o ? cl[c] - 1 : (a ? cl[c] + 1 : cl[c]);
        }
        const double proposed = get_lk(T, P, W, ncl);
        const double diff = unif64(proposed - lk);
        // `0f64 < diff || rng.gen_bool(diff.exp())` (:736): gen_bool(1.0) draws nothing, and exp(diff) == 1.0 exactly
        // when diff >= -2^-54
        const bool no_draw = ubool(diff >= -0x1p-54);
        bool accept = true;
        if (!no_draw) {
            const float u = reload ? -1.0f : __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wd.u), (int)p));
            const float pe = __expf((float)diff);
            const bool in_range = u >= 0.0f && diff < -1e-3 && diff > -44.4;
            if (ubool(diff <= -44.4 || (in_range && u > pe * 1.001f + 1.3e-6f))) {
                accept = false;
            } else if (!ubool(in_range && u + 0x1p-13f < pe * 0.999f - 3e-7f)) {
                rng_wait(rng, pos_v + 1);
                accept = ubool(bernoulli_exact(uni64(lds_ld64(&rng.ring[ring_slot(pos_v, rng.seg_log)])), diff));
            }
        }
        if (accept) {
#pragma unroll
            for (int c = 0; c < K; c++) {
                tg[c] = T[c];
                np[c] = P[c];
                w[c] = W[c];
                cl[c] = ncl[c];
            }
            if (lane == 0) m.assign[idx] = (uint8_t)nw;
            wsync();
            lk = proposed;
            if (ubool(max < lk)) {
                max = proposed;
                for (uint32_t i = lane; i < n; i += 64) m.argmax[i] = m.assign[i];
                wsync();
            }
        } else {
            // flip back (:746): the reference re-adds / re-subtracts, which leaves rounding residue
#pragma unroll
            for (int c = 0; c < K; c++) {
                if ((uint32_t)c == old) tg[c] = T[c] + el.x;
                if ((uint32_t)c == nw) tg[c] = T[c] - el.x;
            }
        }
        t++;
        since_rebuild++;
        const bool rebuilt = accept || since_rebuild >= 65536u;
        TS_ADD(2, accept ? 1 : 0);
        if (rebuilt) {
            JTK_STAT(const unsigned long long rb_t0 = __builtin_readcyclecounter();)
            publish();
            since_rebuild = 0;
            TS_ADD(5, __builtin_readcyclecounter() - rb_t0);
        }
        TS_ADD(6, __builtin_readcyclecounter() - ev_t0);
        const uint32_t pos_next = no_draw ? pos_v : pos_v + 1;
        if (reload || pos_next - wd.base >= 64) {
            gwindow_load(wd, rng, pos_next, lane);
            p = 0;
            hopw = hop_words(wd);
        } else {
            p = pos_next - wd.base;
            if (rebuilt) hopw = hop_words(wd);
        }
    }
    JTK_STAT(if (lane == 0) printf("TABSTAT chunk %u K %d n %u D %u steps %u fast %llu events %llu accepts %llu reloads %llu scalars %llu cyc_rebuild %llu cyc_event %llu cyc_total %llu residues %llu cyc_wload %llu cyc_hopw %llu uncert %llu cyc_fast %llu fast_entries %llu\n",
                    blockIdx.x, K, n, D, total, ts[0], ts[1], ts[2], ts[3], ts[4], ts[5], ts[6],
                    __builtin_readcyclecounter() - ts_t0, ts[7], ts[8], ts[9], ts[10], ts[11], ts[12]);)
    if (lane == 0) m.k2_stats[16] += n_events;
    rng.pos = wd.base + p;
    rng_release(rng, lane);
    wsync();
    for (uint32_t i = lane; i < n; i += 64) m.assign[i] = m.argmax[i];
    wsync();
    *rng_io = rng;
    return max;
}

}  // namespace
