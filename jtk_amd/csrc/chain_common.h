// chain_common.h -- included by mcmc_kernels.hip alone: k-means, the LKCount helpers and what the three chains share.
#pragma once

namespace {

// slice.choose_weighted over weights w[0..n) in LDS; cum is scratch. Returns -1 on WeightedError.
__device__ __forceinline__ int choose_weighted(Rng &r, const double *w, uint32_t n, double *cum, uint32_t lane) {
    double total = w[0];
    if (!(total >= 0.0)) return -1;
    bool bad = false;
    for (uint32_t i = 1; i < n; i++) {
        const double wi = w[i];
        if (!(wi >= 0.0)) bad = true;
        if (lane == 0) cum[i - 1] = total;
        total += wi;
    }
    if (bad || total == 0.0) return -1;
    double scale = total;
    const double max_rand = 1.0 - 0x1p-52;
    while (scale * max_rand + 0.0 >= total) scale = jtk_bits_f64(jtk_f64_bits(scale) - 1);
    const double v12 = jtk_bits_f64((next_u64(r) >> 12) | 0x3ff0000000000000ULL);
    const double chosen = (v12 - 1.0) * scale + 0.0;
    wsync();
    // partition point of `cum[i] <= chosen` (cum is non-decreasing): count the entries <= chosen
    uint32_t cnt = 0;
    for (uint32_t i = lane; i + 1 < n; i += 64) cnt += cum[i] <= chosen ? 1u : 0u;
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    wsync();
    return (int)cnt;
}

__device__ __forceinline__ double dist_row(const double *a, const double *b, uint32_t D) {
    double s = 0.0;
    for (uint32_t d = 0; d < D; d++) {
        const double t = a[d] - b[d];
        s += t * t;
    }
    return s;
}

// misc.rs:261-276 with centres given as K rows of D doubles in LDS (first minimum wins)
__device__ __forceinline__ void update_assignments(const Lds &m, uint32_t n, uint32_t D, uint32_t k, const double *centers,
                                   uint8_t *assign, uint32_t lane) {
    for (uint32_t i = lane; i < n; i += 64) {
        uint32_t best = 0;
        double bd = dist_row(m.data + i * D, centers, D);
        for (uint32_t c = 1; c < k; c++) {
            const double d = dist_row(m.data + i * D, centers + c * D, D);
            if (d < bd) {
                bd = d;
                best = c;
            }
        }
        assign[i] = (uint8_t)best;
    }
    wsync();
}

// misc.rs:298-307: sum over reads, in read order, of dist(read, its centre)
__device__ __forceinline__ double get_dist(const Lds &m, uint32_t n, uint32_t D, const uint8_t *assign, uint32_t lane) {
    for (uint32_t i = lane; i < n; i += 64) m.fbuf[i] = dist_row(m.data + i * D, m.centers + assign[i] * D, D);
    wsync();
    double s = 0.0;
    for (uint32_t i = 0; i < n; i++) s += m.fbuf[i];
    wsync();
    return s;
}

// misc.rs:229-259; returns false where the reference would panic
__device__ __forceinline__ bool kmeans(const Lds &m, uint32_t n, uint32_t D, uint32_t k, Rng &rng, uint32_t lane) {
    const double UPDATE_THR = 0.00000001;
    if (gen_bool(rng, 0.5)) {
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t c = (uint32_t)gen_range_usize(rng, k);
            if (lane == 0) m.assign[i] = (uint8_t)c;
        }
        wsync();
    } else {
        // suggest_first (misc.rs:315-341): centre rows are borrowed data rows; keep their indices in cum's tail
        uint32_t centre_idx[JTK_MAX_COPY];
        centre_idx[0] = (uint32_t)gen_index(rng, n);
        uint32_t nc = 1;
        for (uint32_t it = 0; it + 1 < k; it++) {
            for (uint32_t i = lane; i < n; i += 64) {
                double mn = dist_row(m.data + i * D, m.data + centre_idx[0] * D, D);
                for (uint32_t c = 1; c < nc; c++) {
                    const double d = dist_row(m.data + i * D, m.data + centre_idx[c] * D, D);
                    if (d < mn) mn = d;
                }
                m.fbuf[i] = mn;
            }
            wsync();
            const int idx = choose_weighted(rng, m.fbuf, n, m.cum, lane);
            if (idx < 0) return false;
            centre_idx[nc++] = (uint32_t)idx;
        }
        for (uint32_t c = 0; c < k; c++)
            for (uint32_t d = lane; d < D; d += 64) m.centers[c * D + d] = m.data[centre_idx[c] * D + d];
        wsync();
        update_assignments(m, n, D, k, m.centers, m.assign, lane);
    }
    // Lloyd iterations; `dist` is first evaluated against all-zero centres
    for (uint32_t e = lane; e < k * D; e += 64) m.centers[e] = 0.0;
    wsync();
    double dist = get_dist(m, n, D, m.assign, lane);
    for (;;) {
        // update_centers (misc.rs:277-297): per (cluster, column) slot, sum in read order
        for (uint32_t e = lane; e < k * D; e += 64) {
            const uint32_t c = e / D, d = e % D;
            double s = 0.0;
            uint32_t cnt = 0;
            for (uint32_t i = 0; i < n; i++)
                if (m.assign[i] == c) {
                    s += m.data[i * D + d];
                    cnt++;
                }
            m.centers[e] = cnt > 0 ? s / (double)cnt : s;
        }
        wsync();
        update_assignments(m, n, D, k, m.centers, m.assign, lane);
        const double nd = get_dist(m, n, D, m.assign, lane);
        if (!(nd < dist + UPDATE_THR)) return false;  // assert!(new_dist < dist + UPDATE_THR)
        if (dist - nd < UPDATE_THR) break;
        dist = nd;
    }
    return true;
}

// Per-lane LKCount of one column for K clusters.
template <int K>
struct Counts {
    double tg[K];
    int np[K], nn[K];
};

template <int K>
__device__ __forceinline__ void lk_add(Counts<K> &q, uint32_t c, double x) {
#pragma unroll
    for (int cc = 0; cc < K; cc++)
        if ((uint32_t)cc == c) {  // c is wave-uniform: a scalar branch, static register index
            q.tg[cc] += x;
            if (JTK_POS_THR < x)
                q.np[cc]++;
            else if (x < -JTK_POS_THR)
                q.nn[cc]++;
        }
}
template <int K>
__device__ __forceinline__ void lk_sub(Counts<K> &q, uint32_t c, double x) {
#pragma unroll
    for (int cc = 0; cc < K; cc++)
        if ((uint32_t)cc == c) {
            q.tg[cc] -= x;
            if (JTK_POS_THR < x)
                q.np[cc]--;
            else if (x < -JTK_POS_THR)
                q.nn[cc]--;
        }
}

// get_used_columns (:847-869) for this lane's column.
// LKCount::is_informative (:818-822) is `0 < total_gain && 0.70 < num_pos / (num_pos + num_neg + 1e-7)`; for
// integer counts the f64 quotient test is exactly `3*num_pos > 7*num_neg` (no count pair comes within 1e-10 of
// the threshold; tests/test_host_and_abi.py checks every pair up to 2000 against the f64 expression).
template <int K>
__device__ __forceinline__ bool column_used(const Counts<K> &q) {
    bool any = false;
    int in_use = 0, in_neg = 0;
#pragma unroll
    for (int c = 0; c < K; c++) {
        const bool pos = 0.0 < q.tg[c];
        any |= pos && 3 * q.np[c] > 7 * q.nn[c];
        in_use += pos ? q.np[c] : 0;
        in_neg += pos ? 0 : q.np[c];
    }
    return any && 2 * in_neg < in_use;
}

template <int K>
__device__ __forceinline__ void fill_counts(const Lds &m, uint32_t n, uint32_t D, const uint8_t *assign,
                                            Counts<K> &q, int *clusters, uint32_t lane) {
#pragma unroll
    for (int c = 0; c < K; c++) {
        q.tg[c] = 0.0;
        q.np[c] = 0;
        q.nn[c] = 0;
        clusters[c] = 0;
    }
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t c = uni(assign[i]);
        const double x = lane < D ? m.data[i * D + lane] : 0.0;
        lk_add<K>(q, c, x);
#pragma unroll
        for (int cc = 0; cc < K; cc++)
            if ((uint32_t)cc == c) clusters[cc]++;
    }
}

__device__ __forceinline__ double readlane_f64(double v, uint32_t l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), (int)l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), (int)l);
    return __hiloint2double(hi, lo);
}

// Per-read values spread over lanes: element i lives in lane i & 63 of register i >> 6 (n <= 255).
// SMALL (n <= 63): everything sits in register 0 and the lookups are branch-free.
struct LaneTab {
    double v[4];
};
template <bool SMALL>
__device__ __forceinline__ double tab_get(const LaneTab &t, uint32_t i) {
    if (SMALL) return readlane_f64(t.v[0], i);
    const uint32_t l = i & 63;
    switch (i >> 6) {
        case 0: return readlane_f64(t.v[0], l);
        case 1: return readlane_f64(t.v[1], l);
        case 2: return readlane_f64(t.v[2], l);
        default: return readlane_f64(t.v[3], l);
    }
}
struct LaneLabels {
    int v[4];
};
template <bool SMALL>
__device__ __forceinline__ uint32_t lab_get(const LaneLabels &a, uint32_t i) {
    if (SMALL) return (uint32_t)__builtin_amdgcn_readlane(a.v[0], (int)i);
    const int l = (int)(i & 63);
    switch (i >> 6) {
        case 0: return (uint32_t)__builtin_amdgcn_readlane(a.v[0], l);
        case 1: return (uint32_t)__builtin_amdgcn_readlane(a.v[1], l);
        case 2: return (uint32_t)__builtin_amdgcn_readlane(a.v[2], l);
        default: return (uint32_t)__builtin_amdgcn_readlane(a.v[3], l);
    }
}
template <bool SMALL>
__device__ __forceinline__ void lab_set(LaneLabels &a, uint32_t i, uint32_t val, uint32_t lane) {
    const bool mine = lane == (i & 63);
    if (SMALL) {
        a.v[0] = mine ? (int)val : a.v[0];
        return;
    }
    switch (i >> 6) {
        case 0: a.v[0] = mine ? (int)val : a.v[0]; break;
        case 1: a.v[1] = mine ? (int)val : a.v[1]; break;
        case 2: a.v[2] = mine ? (int)val : a.v[2]; break;
        default: a.v[3] = mine ? (int)val : a.v[3]; break;
    }
}

// Position (0-based among the K-1 candidates) that `(0..K).filter(|c| c != old).choose(rng)` selects
// (pseudo_mcmc.rs:732): the i-th yielded candidate replaces the pick iff gen_index(i) == 0, whatever `old` is.
__device__ __forceinline__ uint32_t choose_pos(Rng &r, uint32_t k) {
    uint32_t pos = 0;
    for (uint32_t i = 1; i < k; i++)
        if (gen_index(r, i) == 0) pos = i - 1;
    return pos;
}

// The Bernoulli test of `0f64 < diff || rng.gen_bool(diff.exp())` (:736) for a step that does draw:
// gen_bool compares the u64 draw v with p_int = floor(exp(diff) * 2^64).  The exact exp is only evaluated
// when an f32 estimate with a guard band cannot decide, so the decision is always the exact one.
// (out of line: the exact exp is the rare path and the chain is sensitive to its code size)
__device__ __attribute__((noinline)) bool bernoulli_exact(uint64_t v, double diff) {
    // f32 estimate first: u = v / 2^64 within 2^-24, pe = exp(diff) within ~1e-5 relative
    const float u = (float)(uint32_t)(v >> 40) * 0x1p-24f;
    const float pe = __expf((float)diff);
    const bool in_range = diff < -1e-3 && diff > -44.4;
    if (ubool(diff <= -44.4 || (in_range && u > pe * 1.001f + 3e-7f))) return false;  // exp(diff) * 2^64 < 1 => p_int == 0
    if (ubool(in_range && u < pe * 0.999f - 3e-7f)) return true;
    const double scaled = unif64(jtk_exp(diff)) * 18446744073709551616.0;
    return v < uni64(__double2ull_rz(scaled));
}

// Neighbour-lane reads that stay off the LDS crossbar (a ds_bpermute round trip costs a lone wave ~100 cycles).
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double from_next_lane(double v) { return dpp_f64<0x134>(v); }  // lane l <- lane l+1 (wave_rol:1)
__device__ __forceinline__ double from_prev_lane(double v) { return dpp_f64<0x13C>(v); }  // lane l <- lane l-1 (wave_ror:1)
__device__ __forceinline__ double wave_sum_f64(double v) {  // order-free: for estimates only
    v += dpp_f64<0xB1>(v);   // quad_perm [1,0,3,2]
    v += dpp_f64<0x4E>(v);   // quad_perm [2,3,0,1]
    v += dpp_f64<0x141>(v);  // row_half_mirror
    v += dpp_f64<0x140>(v);  // row_mirror: every lane of a 16-lane row holds the row sum
    return (readlane_f64(v, 0) + readlane_f64(v, 16)) + (readlane_f64(v, 32) + readlane_f64(v, 48));
}

// The rejection threshold from the order-free estimate dA of proposed - lk.  u is the Bernoulli draw truncated to
// 19 bits (so the true uniform is < u + 2^-19); exp in f32 is good to ~1e-5 relative: 1.001 and 1.3e-6 cover both.
__device__ __forceinline__ float reject_threshold(double dA, bool pert) {
    float thr = 2.0f;  // cannot tell: the proposal becomes an event
    if (!pert && dA < -1e-3) thr = dA <= -44.5 ? -1.0f : __expf((float)dA) * 1.001f + 1.3e-6f;
    return thr;
}
// LDS accessors for the tables of the table-driven chains (generic pointers would make these flat accesses; structs
// travel as 16-byte vectors: one ds_read_b128 / ds_write_b128 each)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const u32x4 lds_c_u32x4;
typedef __attribute__((address_space(3))) u32x4 lds_u32x4;
typedef __attribute__((address_space(3))) const double lds_c_f64;
typedef __attribute__((address_space(3))) float lds_f32;
__device__ __forceinline__ double lo_f64(u32x4 v) { return jtk_bits_f64(((uint64_t)v.y << 32) | v.x); }
__device__ __forceinline__ double hi_f64(u32x4 v) { return jtk_bits_f64(((uint64_t)v.w << 32) | v.z); }
__device__ __forceinline__ void lds_put_sz(SzEnt *p, const SzEnt &e) {
    lds_u32x4 *q = (lds_u32x4 *)p;
    const uint64_t a = jtk_f64_bits(e.rem), b = jtk_f64_bits(e.add);
    u32x4 v, w;
    v.x = (uint32_t)a;
    v.y = (uint32_t)(a >> 32);
    v.z = (uint32_t)b;
    v.w = (uint32_t)(b >> 32);
    w.x = e.nr;
    w.y = e.um;
    w.z = w.w = 0;
    q[0] = v;
    q[1] = w;
}
__device__ __forceinline__ SzEnt lds_load_sz(const SzEnt *p) {
    lds_c_u32x4 *q = (lds_c_u32x4 *)p;
    const u32x4 a = q[0];
    SzEnt e;
    e.rem = lo_f64(a);
    e.add = hi_f64(a);
    e.nr = ((__attribute__((address_space(3))) const uint32_t *)p)[4];  // byte 16
    e.um = ((__attribute__((address_space(3))) const uint32_t *)p)[5];
    e.pad[0] = e.pad[1] = 0;
    return e;
}

}  // namespace
