// chain_producer.h -- included by mcmc_kernels.hip alone: the producer wave (xoshiro256** into the ring, proposal records).
#pragma once

namespace {

// The producer wave: Xoshiro256StarStar::seed_from_u64(seed), free running into the ring.
//
// xoshiro's state update is linear over GF(2), so the stream can be cut into segments that are generated side by
// side: lane l of the producer owns segment l of the current superblock (SEG consecutive draws) and runs the plain
// generator on its own copy of the state with ordinary 64-bit vector arithmetic -- 64 draws per ~20 instructions
// instead of one draw per ~11 scalar instructions.  After a superblock every lane stands at the start of the NEXT
// lane's segment and has to skip the other 63 segments: multiplication of the 256-bit state by the constant matrix
// M^(63*SEG), done as 128 two-bit look-ups in a 16 KiB table (g_jump_tab, computed once on the host from the step
// function itself, staged in LDS) XOR-ed together.  The sequence of draws is exactly that of the sequential generator.
// [byte of the state][value of that byte] -> 256-bit image under M^(63*SEG): 256 KiB in device memory, read by every producer
// wave of the machine (L2 resident).  One jump is 32 look-ups of 32 bytes XOR-ed together; up to round 4 the digits had two bits
// (128 look-ups in a 16 KiB table): 12 cycles per draw, as much as parsing the proposals -- now 4.
__device__ ulonglong2 g_jump_tab[2][32 * 256 * 2];  // [seg_log - 3]: M^(63 * 8), M^(63 * 16)

struct Xo {
    uint64_t s0, s1, s2, s3;
};
__device__ __forceinline__ void xo_step(Xo &x) {
    const uint64_t t = x.s1 << 17;
    x.s2 ^= x.s0;
    x.s3 ^= x.s1;
    x.s1 ^= x.s2;
    x.s0 ^= x.s3;
    x.s2 ^= t;
    x.s3 = rotl64(x.s3, 45);
}
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
// The loop is compact on purpose: fully unrolled it is kilobytes of straight-line code executed once per superblock, and
// this kernel is large.  Eight look-ups (16 loads) are in flight at a time.
__device__ __forceinline__ void xo_jump(Xo &x, uint32_t seg_log) {
    const u64x2 *tab = reinterpret_cast<const u64x2 *>(g_jump_tab[seg_log - 3u]);
    uint64_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
#pragma unroll 1
    for (int q = 0; q < 4; q++) {
        const uint64_t wq = q == 0 ? x.s0 : (q == 1 ? x.s1 : (q == 2 ? x.s2 : x.s3));
        const u64x2 *row = tab + (size_t)(q * 8) * 256 * 2;
        u64x2 lo[8], hi[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const uint32_t v = (uint32_t)(wq >> (8 * u)) & 255u;
            const u64x2 *e = row + ((size_t)u * 256 + v) * 2;
            lo[u] = e[0];
            hi[u] = e[1];
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            a0 ^= lo[u].x;
            a1 ^= lo[u].y;
            a2 ^= hi[u].x;
            a3 ^= hi[u].y;
        }
    }
    x.s0 = a0;
    x.s1 = a1;
    x.s2 = a2;
    x.s3 = a3;
}
// Proposal records.  For the diploid chain a proposal is: gen_range(0..n) takes the first draw at or after its start
// whose widening multiply is accepted, gen_index(1) (the single candidate of K == 2, pseudo_mcmc.rs:732) then takes
// draws until one has a clear top bit, and the next draw is the one a Bernoulli test would compare.  None of this
// depends on the chain, so the producer parses the proposal that WOULD start at every stream position q:
//   rec[q] = idx | len << 7 | (top 19 bits of the Bernoulli draw) << 13      (idx < 128; len = draws used incl. that draw)
// rec == 0: not parsed (needs more than the 16..63 draws of look-ahead; the consumer then steps with scalar draws).
// 64 positions are parsed at once -- acceptance masks by ballot, "next accepted draw at or after p" by s_ff1 -- and
// the first PKEEP are kept, so every kept start had at least 64 - PKEEP draws of look-ahead (a proposal needs more
// with probability 2^-14).  R rounds are written stage by stage so that their instruction streams interleave:
// a lone wave pays ~8 cycles for a dependent instruction and ~4 for an independent one.
#define PKEEP 48
template <int R>
__device__ __forceinline__ void producer_parse(const uint64_t *ring, uint32_t *rec, uint32_t base, uint32_t n, uint32_t lane,
                                               uint32_t seg_log) {
    const uint64_t zone = ((uint64_t)n << __clzll((long long)n)) - 1;
    uint64_t draw[R];
    uint32_t hi[R], pi[R], pv[R], idx[R], vhi[R];
    bool ok[R];
#pragma unroll
    for (int r = 0; r < R; r++) draw[r] = lds_ld64(&ring[ring_slot(base + r * PKEEP + lane, seg_log)]);
#pragma unroll
    for (int r = 0; r < R; r++) {
        hi[r] = (uint32_t)__umul64hi(draw[r], (uint64_t)n);
        const unsigned long long okm = __ballot(draw[r] * (uint64_t)n <= zone);  // gen_range(0..n) accepts this draw
        const unsigned long long topm = __ballot((int64_t)draw[r] >= 0);          // gen_index(1) accepts this draw
        const unsigned long long m1 = okm >> lane;
        pi[r] = lane + (uint32_t)__builtin_ctzll(m1 | (1ull << 63));
        const unsigned long long m2 = pi[r] < 63 ? topm >> (pi[r] + 1) : 0ull;
        pv[r] = pi[r] + 1 + (uint32_t)__builtin_ctzll(m2 | (1ull << 63)) + 1;  // the Bernoulli draw
        ok[r] = m1 != 0 && m2 != 0 && pv[r] < 64;
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
        idx[r] = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((pi[r] & 63) << 2), (int)hi[r]);
        vhi[r] = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((pv[r] & 63) << 2), (int)(uint32_t)(draw[r] >> 32));
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
        const uint32_t v = ok[r] ? (idx[r] | ((pv[r] + 1 - lane) << 7) | (vhi[r] & 0xffffe000u)) : 0u;
        if (lane < PKEEP) lds_st32(&rec[(base + r * PKEEP + lane) & (RN_OF(seg_log) - 1)], v);
    }
}
// Records of the general chain (any K).  A proposal is gen_range(0..n) -- the first draw at or after its start whose
// widening product passes the zone test -- then gen_index(i) for i = 1..K-1 on the upper halves of the following draws,
// each with its own zone test (IteratorRandom::choose over the K-1 other clusters, pseudo_mcmc.rs:732: the pick is the
// last i whose index came out 0), and the next draw is the one a Bernoulli test would compare:
//   rec[q] = idx (10 bits) | pick << 10 (3) | len << 13 (6: draws used incl. the Bernoulli draw) | top 13 bits of that draw << 19
// rec == 0: not parsed (needs more look-ahead than the window gives).  `keep` positions are kept per round, so every kept
// start had 64 - keep draws of look-ahead.
__device__ __forceinline__ void producer_parse_gen(const uint64_t *ring, uint32_t *rec, uint32_t base, uint32_t n, uint32_t K,
                                                   uint32_t keep, uint32_t lane, uint32_t seg_log) {
    const uint64_t zone = ((uint64_t)n << __clzll((long long)n)) - 1;
    const uint64_t draw = lds_ld64(&ring[ring_slot(base + lane, seg_log)]);
    const uint32_t v32 = (uint32_t)(draw >> 32);
    const uint32_t hi = (uint32_t)__umul64hi(draw, (uint64_t)n);
    const unsigned long long ok0 = __ballot(draw * (uint64_t)n <= zone);
    const unsigned long long m0 = ok0 >> lane;
    bool good = m0 != 0ull;
    uint32_t p = lane + (uint32_t)__builtin_ctzll(m0 | (1ull << 63));  // window offset of the gen_range draw
    const uint32_t idx = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((p & 63u) << 2), (int)hi);
    uint32_t pick = 0;
    for (uint32_t i = 1; i < K; i++) {
        const uint32_t zi = (i << __builtin_clz(i)) - 1u;
        const uint64_t mi = (uint64_t)v32 * i;
        const unsigned long long okm = __ballot((uint32_t)mi <= zi);
        const unsigned long long zm = __ballot((uint32_t)(mi >> 32) == 0u);
        const unsigned long long mm = (good && p < 63u) ? okm >> (p + 1u) : 0ull;
        good = good && mm != 0ull;
        p = (p + 1u + (uint32_t)__builtin_ctzll(mm | (1ull << 63))) & 127u;
        if (good && ((zm >> (p & 63u)) & 1ull)) pick = i - 1u;
    }
    const uint32_t pv = p + 1u;  // the Bernoulli draw
    good = good && pv < 64u;
    const uint32_t vhi = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((pv & 63u) << 2), (int)v32);
    const uint32_t v = good ? (idx | (pick << 10) | ((pv + 1u - lane) << 13) | (vhi & 0xfff80000u)) : 0u;
    if (lane < keep) lds_st32(&rec[(base + lane) & (RN_OF(seg_log) - 1)], v);
}
__device__ __forceinline__ void producer_main(RCtl *ctl, uint64_t *ring, uint32_t *rec, uint32_t seg_log, uint64_t seed,
                                              const uint64_t *resume, uint32_t lane) {
    const uint32_t SEG = 1u << seg_log, SBLK = 64u << seg_log, RN = RN_OF(seg_log);
    uint64_t z = seed;
    Xo x;
    if (resume) {  // a later clustering() call of the same chunk continues the stream (clustering_recursive, mod.rs:158)
        x.s0 = resume[0];
        x.s1 = resume[1];
        x.s2 = resume[2];
        x.s3 = resume[3];
    } else {
        x.s0 = splitmix64(z);
        x.s1 = splitmix64(z);
        x.s2 = splitmix64(z);
        x.s3 = splitmix64(z);
    }
    for (uint32_t j = 0; j < lane * SEG; j++) xo_step(x);  // lane l starts at stream position l * SEG
    uint32_t parse_n = 0, pmode = 0;
    uint32_t wr = 0, wp = 0;
    JTK_STAT(uint32_t st_sleeps = 0;)
    JTK_STAT(unsigned long long st_gen = 0, st_parse = 0, st_jump = 0;)
    for (;;) {
        const uint64_t c = uni64(lds_ld64((const uint64_t *)&ctl->rd));  // rd, quit
        if ((uint32_t)(c >> 32)) {
            JTK_STAT(if (lane == 0) printf("K2PROD wr %u sleeps %u cyc_gen %llu cyc_parse %llu cyc_jump %llu\n", wr, st_sleeps, st_gen, st_parse, st_jump);)
            return;
        }
        {   // a new parse mode: records are re-parsed from the position the consumer names
            const uint32_t pm = uni(lds_ld32(&ctl->pmode));
            if (pm != pmode) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                pmode = pm;
                parse_n = uni(lds_ld32(&ctl->parse_n));
                wp = uni(lds_ld32(&ctl->parse_from));
                if (lane == 0) lds_st32(&ctl->wp, wp);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                if (lane == 0) lds_st32(&ctl->wp_epoch, pm >> 16);
            }
        }
        const uint32_t mode = pmode & 0xffffu;
        if (mode) {
            JTK_STAT(const unsigned long long tq0 = __builtin_readcyclecounter();)
            // a start at q needs draws up to q + 63: the last positions wait for the next superblock
            bool parsed = false;
            while ((int32_t)(wr - (wp + 64)) >= 0) {
                if (mode == PM_K2) {
                    if ((int32_t)(wr - (wp + 3 * PKEEP + 64)) >= 0) {
                        producer_parse<4>(ring, rec, wp, parse_n, lane, seg_log);
                        wp += 4 * PKEEP;
                    } else {
                        producer_parse<1>(ring, rec, wp, parse_n, lane, seg_log);
                        wp += PKEEP;
                    }
                } else {
                    const uint32_t keep = mode <= 4u ? 44u : 32u;  // K - 1 more rejection loops need more look-ahead
                    producer_parse_gen(ring, rec, wp, parse_n, mode, keep, lane, seg_log);
                    wp += keep;
                }
                parsed = true;
            }
            if (parsed) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                if (lane == 0) lds_st32(&ctl->wp, wp);
            }
            JTK_STAT(st_parse += __builtin_readcyclecounter() - tq0;)
        }
        if ((int32_t)(wr + SBLK - (uint32_t)c) > (int32_t)RN) {
            JTK_STAT(st_sleeps++;)
            __builtin_amdgcn_s_sleep(2);
            continue;
        }
        JTK_STAT(const unsigned long long tp0 = __builtin_readcyclecounter();)
        uint64_t *blk = ring + (wr & (RN - 1));
#pragma unroll 8
        for (uint32_t j = 0; j < SEG; j++) {
            const uint64_t m5 = (x.s1 << 2) + x.s1, rr = rotl64(m5, 7);
            lds_st64(&blk[j * 64 + ((lane + j) & 63)], (rr << 3) + rr);  // rotl(s1 * 5, 7) * 9, skewed: no bank conflicts
            xo_step(x);
        }
        wr += SBLK;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if (lane == 0) lds_st32(&ctl->wr, wr);
        JTK_STAT(const unsigned long long tp1 = __builtin_readcyclecounter();)
        JTK_STAT(st_gen += tp1 - tp0;)
        JTK_STAT(const unsigned long long tp2 = __builtin_readcyclecounter();)
        xo_jump(x, seg_log);
        JTK_STAT(st_jump += __builtin_readcyclecounter() - tp2;)
    }
}

}  // namespace
