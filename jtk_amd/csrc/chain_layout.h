// chain_layout.h -- the ring's geometry, the control block and ONE list of the arrays of a chunk's work area, from which the
// device's carve (lds_carve, chain_lds.h; mcmc_kernels.hip alone) and the host's sizes below both follow (mcmc_kernels.hip for
// its launches, session_plan.h for the launch classes).  Plain C++ (tests/test_chain_layout.py compiles it without HIP); wants
// JTK_MAX_COPY (batch_types.h).
#pragma once
#include <stddef.h>
#include <stdint.h>

// The ring of raw xoshiro256** outputs.  `wr` draws have been produced, the consumer has released `rd`.
#ifndef JTK_LIGHT_MAX_READS
#define JTK_LIGHT_MAX_READS 127u  // what mcmc_kernel_light takes: diploid pile-ups of <= 127 reads ...
#endif
#define JTK_LIGHT_MAX_DIM 2u      // ... with <= 2 variant columns (mcmc_chain_k2<1,..> / <2,..>: 168 registers)
// The producer's lanes generate SEG = 2^seg_log consecutive draws each per superblock (64 SEG draws); the ring holds two
// superblocks (RN draws + RN records).  seg_log is a launch parameter (round 5): 4 in the light kernel and the global-memory one
// (a 24 KiB ring: the jump is paid once per 1,024 draws), 3 in the general kernel -- a 12 KiB ring is what lets FOUR chain
// workgroups of a 4-copy pile-up share a CU's LDS (40.7 KB each), and the K-way chains' producer has slack for the extra jumps.
#ifndef JTK_SEG_LOG_LIGHT
#define JTK_SEG_LOG_LIGHT 4u
#endif
#define JTK_SEG_LOG_GENERAL 3u
#define RN_OF(seg_log) (128u << (seg_log))
#define K2_STAT_SLOTS 24             // counters in LDS per chunk: 16 of the statistics build, [16] events (every build)
#define JTK_HUGE_LDS (128u * 1024u)  // dynamic LDS of mcmc_kernel_huge behind the ring and its control block

namespace {

struct RCtl {
    uint32_t rd, quit;  // written by the consumer (read together, 8-byte aligned)
    uint32_t wr, wp;    // written by the producer: draws produced / stream positions whose proposal record exists
    // Proposal records are parsed for ONE (format, K) at a time.  The consumer announces a new mode by writing parse_from
    // (the stream position from which it will read records), parse_n and then pmode = epoch << 16 | mode; the producer
    // re-parses from parse_from and acknowledges with wp_epoch = epoch (after resetting wp).
    uint32_t parse_n;     // reads in the pile-up
    uint32_t parse_from;
    uint32_t pmode;       // mode: 0 = no records, PM_K2 = the diploid chain's format, otherwise K of the general format
    uint32_t wp_epoch;
};
#define PM_K2 0x100u
// The work area is carved out of the workgroup's dynamic LDS from four numbers.  Out-of-line functions get THOSE (by value)
// and carve again: two dozen 64-bit pointers that live across a call -- or travel through memory as a struct -- cost the
// caller its registers and the callee flat loads (and hipcc 7.2 fails with "Subtarget requires even aligned vector
// registers" when a kernel body has to spill a 64-bit value across a call).
struct LdsShape {
    uint32_t n, d, k, seg_log;  // capacity in reads / columns / clusters; the ring's geometry
    uint64_t gws;            // 0, or the address of a global-memory workspace (mcmc_kernel_huge): whatever of the arrays sized
                             // by n / d / k does not fit the JTK_HUGE_LDS bytes of LDS behind the ring goes there, in carve order
};
struct SzEnt {     // 32 bytes, read as two 16-byte vectors
    double rem;    // size_to_lk[size - 1] - size_to_lk[size]: what the size terms gain when a read leaves the cluster
    double add;    // size_to_lk[size + 1] - size_to_lk[size]
    uint32_t nr;   // columns where this cluster's `total_gain > 0` could flip under a single move
    uint32_t um;   // columns this cluster is paid for (used and total_gain > 0): what s[c][.] sums over
    uint32_t pad[2];
};

}  // namespace

// The arrays of the work area, in carve order: X(member of Lds, element type, bytes), the bytes an expression in n, d, k (the
// capacity in reads / columns / clusters), npad (n rounded up to 64: the row stride of stab) and seg_log; every array starts
// on a 16-byte boundary.  The fixed head sits in LDS in every kernel; of the sized arrays mcmc_kernel_huge keeps what fits
// JTK_HUGE_LDS and puts the rest into the chunk's global workspace.  The sized arrays are listed in two pieces because the
// carve computes npad between them, where it always did: computed earlier, the same statements compile to other machine code.
// (fbuf / cum are no arrays of their own: they live inside stab, see lds_carve.)
#define JTK_CHAIN_FIXED_ARRAYS(X)                                  \
    X(ctl, RCtl, sizeof(RCtl))                                     \
    X(ring, uint64_t, sizeof(uint64_t) * RN_OF(seg_log))           \
    X(rec, uint32_t, sizeof(uint32_t) * RN_OF(seg_log))            \
    X(k2_stats, unsigned long long, K2_STAT_SLOTS * 8)
#define JTK_CHAIN_SIZED_ARRAYS(X) JTK_CHAIN_SIZED_HEAD(X) JTK_CHAIN_SIZED_TABLES(X)
#define JTK_CHAIN_SIZED_HEAD(X)                                    \
    X(data, double, (size_t)n * d * 8)                             \
    X(size_to_lk, double, (size_t)(n + 1) * 8)                     \
    X(lfact, double, (size_t)(n + 1) * 8)                          \
    X(val, double, (size_t)JTK_MAX_COPY * d * 8)                   \
    X(centers, double, (size_t)JTK_MAX_COPY * d * 8)               \
    X(assign, uint8_t, n)                                          \
    X(argmax, uint8_t, n)                                          \
    X(best, uint8_t, n)                                            \
    X(accepted, uint8_t, n)                                        \
    X(tmp_asn, uint8_t, n)                                         \
    X(used, uint8_t, d)                                            \
    X(prev_used, uint8_t, d)                                       \
    X(tmp_used, uint8_t, d)
#define JTK_CHAIN_SIZED_TABLES(X) /* the tables of mcmc_chain_tab */ \
    X(stab, double, (size_t)k * npad * 8)                          \
    X(nz, uint32_t, (size_t)npad * 4)                              \
    X(sz, SzEnt, (size_t)k * sizeof(SzEnt))                        \
    X(st, u32x4_t, (size_t)d * k * 16)                             \
    X(col, u32x4_t, (size_t)d * 16)
#define JTK_CHAIN_NPAD(n) (((n) + 63u) & ~63u)

// LDS work area of one chunk for a ring of 2 x (64 << seg_log) positions (the producer's jump table lives in global memory / L2).
#define JTK_CHAIN_ADD_BYTES(member, type, bytes) +(((size_t)(bytes) + 15) & ~(size_t)15)
static size_t mcmc_lds_core(uint32_t n, uint32_t d, uint32_t k, uint32_t seg_log = JTK_SEG_LOG_LIGHT) {
    const uint32_t npad = JTK_CHAIN_NPAD(n);
    return 0 JTK_CHAIN_FIXED_ARRAYS(JTK_CHAIN_ADD_BYTES) JTK_CHAIN_SIZED_ARRAYS(JTK_CHAIN_ADD_BYTES);
}
static uint32_t clamp_k(uint32_t lds_k) { return lds_k < 2 ? 2 : (lds_k > JTK_MAX_COPY ? JTK_MAX_COPY : lds_k); }
// mcmc_kernel_huge: the LDS in front of the sized arrays (ring + control block) and the global workspace of one chunk (an upper
// bound: everything sized by n, d, k -- lds_carve keeps what fits JTK_HUGE_LDS in LDS)
static size_t mcmc_lds_fixed() {
    const uint32_t seg_log = JTK_SEG_LOG_LIGHT;
    return 0 JTK_CHAIN_FIXED_ARRAYS(JTK_CHAIN_ADD_BYTES);
}
inline size_t mcmc_ws_bytes(uint32_t n, uint32_t d, uint32_t k) {
    k = clamp_k(k);
    return ((mcmc_lds_core(n, d, k) - mcmc_lds_fixed()) + 255) & ~(size_t)255;
}
// (the session sorts chunks into launch classes by this number, which assumes the light kernel's 24 KiB ring; the general kernel
// is launched with 12 KiB less (launch_mcmc), so the classing is conservative by that much and jtk_lc_timing_t.chain_lds_bytes
// reports an upper bound -- ADVICE round 5; left as it is: tests pin the class boundaries at these sizes)
inline size_t mcmc_lds_bytes(uint32_t lds_n, uint32_t lds_d, uint32_t lds_k) { return mcmc_lds_core(lds_n, lds_d, clamp_k(lds_k)); }
