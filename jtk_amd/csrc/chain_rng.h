// chain_rng.h -- included by mcmc_kernels.hip alone: the LDS accessors, the consumer's view of the random stream and the
// rand 0.8.5 sampling on top of it.
#pragma once

namespace {

// ---- LDS accessors for the producer/consumer hand-off.  The pointers reach us as generic pointers; casting
// them back to the LDS address space makes these ds_read/ds_write instead of waited flat accesses.
// volatile: re-read every time, in program order (LDS operations of one wave execute in order).
typedef __attribute__((address_space(3))) volatile uint32_t lds_vu32;
typedef __attribute__((address_space(3))) volatile uint64_t lds_vu64;
__device__ __forceinline__ uint32_t lds_ld32(const uint32_t *p) { return *(lds_vu32 *)p; }
__device__ __forceinline__ void lds_st32(uint32_t *p, uint32_t v) { *(lds_vu32 *)p = v; }
__device__ __forceinline__ uint64_t lds_ld64(const uint64_t *p) { return *(lds_vu64 *)p; }
__device__ __forceinline__ void lds_st64(uint64_t *p, uint64_t v) { *(lds_vu64 *)p = v; }
__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t uni64(uint64_t v) {
    return ((uint64_t)uni((uint32_t)(v >> 32)) << 32) | uni((uint32_t)v);
}

// stream position -> ring slot.  Inside a superblock, draw j of segment g sits at j * 64 + ((g + j) & 63): the
// producer's 64 lanes (one segment each) and the consumer's 64-draw windows (consecutive j) both hit distinct banks.
__device__ __forceinline__ uint32_t ring_slot(uint32_t pos, uint32_t seg_log) {
    const uint32_t half = 64u << seg_log;  // draws per superblock
    const uint32_t o = pos & (half - 1), g = o >> seg_log, j = o & ((1u << seg_log) - 1);
    return (pos & half) | (j * 64 + ((g + j) & 63));
}
// The consumer's view of the generator: a position in the stream of Xoshiro256StarStar::seed_from_u64(id * 3490)
// (local_clustering/mod.rs:97).  next_u64 == rand_xoshiro's next_u64, one stream position later.
struct Rng {
    uint32_t pos;      // next draw to take (absolute stream position)
    uint32_t wr_seen;  // producer progress last observed
    uint32_t wp_seen;  // record progress last observed
    uint32_t pmode;    // the parse mode last announced (epoch << 16 | mode)
    uint32_t win_base; // stream position of the draw held by lane 0 of `win`
    uint32_t seg_log;  // the ring's geometry (RN_OF(seg_log) draws)
    uint64_t win;      // per lane: the raw draw at win_base + lane (one LDS read serves 64 sequential draws)
    JTK_STAT(uint32_t waits;)    // polls of the producer's counters that found nothing new
    RCtl *ctl;
    const uint64_t *ring;
    const uint32_t *rec;  // proposal records, one per stream position (see producer_parse)
};
__device__ __forceinline__ uint64_t rotl64(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
__device__ __forceinline__ uint64_t splitmix64(uint64_t &x) {
    x += 0x9e3779b97f4a7c15ULL;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}
__device__ __forceinline__ void rng_wait(Rng &r, uint32_t upto) {  // until draws [.., upto) exist
    while ((int32_t)(r.wr_seen - upto) < 0) {
        r.wr_seen = uni(lds_ld32(&r.ctl->wr));
        if ((int32_t)(r.wr_seen - upto) < 0) __builtin_amdgcn_s_sleep(1);
    }
}
__device__ __forceinline__ void rng_wait_rec(Rng &r, uint32_t upto) {  // until records [.., upto) exist
    while ((int32_t)(r.wp_seen - upto) < 0) {
        r.wp_seen = uni(lds_ld32(&r.ctl->wp));
        JTK_STAT(if ((int32_t)(r.wp_seen - upto) < 0) r.waits++;)
        if ((int32_t)(r.wp_seen - upto) < 0) __builtin_amdgcn_s_sleep(1);
    }
}
// The records from stream position r.pos on are wanted in `mode` (see RCtl); returns once the producer has switched.
__device__ __forceinline__ void rng_set_parse_mode(Rng &r, uint32_t mode, uint32_t lane) {
    if ((r.pmode & 0xffffu) == mode) return;  // the producer parses every position: nothing to re-synchronise
    const uint32_t word = (((r.pmode >> 16) + 1u) << 16) | mode;
    r.pmode = word;
    if (lane == 0) {
        lds_st32(&r.ctl->rd, r.pos);
        lds_st32(&r.ctl->parse_from, r.pos);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (lane == 0) lds_st32(&r.ctl->pmode, word);
    while (uni(lds_ld32(&r.ctl->wp_epoch)) != (word >> 16)) __builtin_amdgcn_s_sleep(1);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    r.wp_seen = r.pos;  // progress of the old mode says nothing about the new one
}
__device__ __forceinline__ void rng_release(Rng &r, uint32_t lane) {  // draws before r.pos may be overwritten
    if (lane == 0) lds_st32(&r.ctl->rd, r.pos);
}
__device__ __forceinline__ void rng_refill(Rng &r) {  // the register window: 64 draws from r.pos on, one per lane
    r.win_base = r.pos;
    lds_st32(&r.ctl->rd, r.pos);  // every lane stores the same value: draws before r.pos may be overwritten
    rng_wait(r, r.pos + 64);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    r.win = lds_ld64(&r.ring[ring_slot(r.pos + (threadIdx.x & 63u), r.seg_log)]);
}
__device__ __forceinline__ uint64_t next_u64(Rng &r) {
    if ((uint32_t)(r.pos - r.win_base) >= 64u) rng_refill(r);
    const uint32_t off = r.pos - r.win_base;
    const uint64_t v = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(r.win >> 32), (int)off) << 32) |
                       (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)r.win, (int)off);
    r.pos++;
    return v;
}
__device__ __forceinline__ uint32_t next_u32(Rng &r) { return (uint32_t)(next_u64(r) >> 32); }
__device__ __forceinline__ uint64_t gen_range_usize(Rng &r, uint64_t n) {
    const uint64_t zone = (n << __clzll((long long)n)) - 1;
    for (;;) {
        const uint64_t v = next_u64(r);
        const uint64_t hi = __umul64hi(v, n), lo = v * n;
        if (lo <= zone) return hi;
    }
}
__device__ __forceinline__ uint32_t gen_range_u32(Rng &r, uint32_t n) {
    const uint32_t zone = (n << __clz((int)n)) - 1;
    for (;;) {
        const uint32_t v = next_u32(r);
        const uint64_t m = (uint64_t)v * n;
        if ((uint32_t)m <= zone) return (uint32_t)(m >> 32);
    }
}
__device__ __forceinline__ uint64_t gen_index(Rng &r, uint64_t ub) {
    return ub <= 0xffffffffULL ? gen_range_u32(r, (uint32_t)ub) : gen_range_usize(r, ub);
}
__device__ __forceinline__ bool gen_bool(Rng &r, double p) {
    if (p == 1.0) return true;
    const double scaled = p * 18446744073709551616.0;
    const uint64_t p_int = !(scaled > 0.0) ? 0ull : __double2ull_rz(scaled);
    return next_u64(r) < p_int;
}
__device__ __forceinline__ uint32_t choose_other(Rng &r, uint32_t k, uint32_t old) {
    uint32_t result = 0xffffffffu, consumed = 0;
    for (uint32_t c = 0; c < k; c++) {
        if (c == old) continue;
        consumed++;
        if (gen_index(r, consumed) == 0) result = c;
    }
    return result;
}

// Only wave 0 runs the non-chain phases, so LDS hand-offs between its lanes need a wave-level fence, not a
// workgroup barrier (the producer wave is parked at a real barrier meanwhile).
__device__ __forceinline__ void wsync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ double unif64(double v) { return jtk_bits_f64(uni64(jtk_f64_bits(v))); }
// a wave-uniform condition as a scalar: branches on it are s_cbranch, not exec-mask regions
__device__ __forceinline__ bool ubool(bool c) { return __ballot(c) != 0ull; }  // c is the same in every lane

}  // namespace
