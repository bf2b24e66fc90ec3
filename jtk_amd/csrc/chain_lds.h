// chain_lds.h -- included by mcmc_kernels.hip alone: one chunk's work area as the device sees it (Lds) and its carve.
#pragma once

extern __shared__ __align__(16) unsigned char jtk_mcmc_smem[];  // the chain kernels' dynamic LDS (see lds_carve)

namespace {

// LDS work area of one chunk
struct Elem {  // one (read, column) cell as the chain needs it (derived from the value on the fly: LDS holds only x)
    double x;  // the likelihood gain
    int dp;    // 1 if x >  POS_THR (counts towards num_pos)
    int pw;    // 3*[x > POS_THR] - 7*[x < -POS_THR]: increment of 3*num_pos - 7*num_neg
};
__device__ __forceinline__ Elem elem_of(double x) {
    Elem el;
    el.x = x;
    el.dp = JTK_POS_THR < x ? 1 : 0;
    el.pw = 3 * el.dp - 7 * (x < -JTK_POS_THR ? 1 : 0);
    return el;
}
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
struct Lds {
    RCtl *ctl;
    uint64_t *ring;      // RN raw draws
    uint32_t *rec;       // RN proposal records of the diploid chain
    unsigned long long *k2_stats;  // 16 debug counters (JTK_MCMC_STATS builds only) + [16]: events of the table-driven chains
    double *data;        // n x D
    double *size_to_lk;  // n + 1
    double *lfact;       // n + 1
    double *val;         // K x D staging of the per-(cluster, column) terms
    double *centers;     // K x D
    double *fbuf;        // n (dists / weights / per-read gains)   -- fbuf and cum alias the head of stab (lds_carve)
    double *cum;         // n
    uint8_t *assign;     // n   current labels
    uint8_t *argmax;     // n   best labels seen in this chain
    uint8_t *best;       // n   best over restarts for this k
    uint8_t *accepted;   // n   labels of the accepted k
    uint8_t *used;       // D
    uint8_t *prev_used;  // D
    uint8_t *tmp_asn;    // n
    uint8_t *tmp_used;   // D
    // tables of the table-driven chain (mcmc_chain_tab)
    double *stab;               // lds_k x npad: s[c][i] = sum over the columns cluster c is paid for of x[i][d]
    uint32_t *nz;               // npad: bit d set iff x[i][d] != 0.0
    struct SzEnt *sz;           // K per-cluster terms: size deltas and the columns where a move involving c is not certified
    u32x4_t *st;                // D x K: (total_gain, num_pos, 3 num_pos - 7 num_neg) of (column, cluster), 16 bytes each
    u32x4_t *col;               // D: (pos_in_use, informative clusters, total pos, -) of the column
    uint32_t npad;              // row stride of stab
    struct LdsShape shape;      // what the carve was made from
};

// The carve: the array list of chain_layout.h turned into take() calls (mcmc_lds_core sums the same list).  `base` passes through an empty asm so that two carves are not merged across a call.
template <bool HUGE = false>
__device__ __forceinline__ Lds lds_carve(LdsShape sh_in) {
    LdsShape sh;
    sh.n = uni(sh_in.n);
    sh.d = uni(sh_in.d);
    sh.k = uni(sh_in.k);
    sh.seg_log = uni(sh_in.seg_log);
    sh.gws = uni64(sh_in.gws);
    uint32_t base = 0;
    asm volatile("" : "+s"(base));
    unsigned char *p = jtk_mcmc_smem + base;
    // mcmc_kernel_huge only: an array that does not fit what is left of JTK_HUGE_LDS lives in the chunk's global workspace.
    // There every pointer is made from an integer that went through an empty asm: the optimizer must not try to prove an address
    // space for a pointer that is LDS on one path and global on the other (hipcc 7.2 crashes in simplifycfg when it does).
    uint64_t pl = 0, gl = sh.gws;
    size_t lds_left = ~(size_t)0;
    if (HUGE) {
        pl = (uint64_t)(uintptr_t)p;
        asm volatile("" : "+s"(pl));
    }
    auto take = [&](size_t bytes) -> unsigned char * {
        bytes = (bytes + 15) & ~(size_t)15;
        if (HUGE) {
            const bool in_lds = bytes <= lds_left;
            uint64_t q = in_lds ? pl : gl;
            pl += in_lds ? bytes : 0;
            gl += in_lds ? 0 : bytes;
            lds_left -= in_lds ? bytes : 0;
            asm volatile("" : "+s"(q));
            return reinterpret_cast<unsigned char *>((uintptr_t)q);
        }
        unsigned char *q = p;
        p += bytes;
        return q;
    };
    const uint32_t n = sh.n, d = sh.d, k = sh.k, seg_log = sh.seg_log;
    Lds m;
#define JTK_CHAIN_TAKE(member, type, bytes) m.member = (type *)take(bytes);
    JTK_CHAIN_FIXED_ARRAYS(JTK_CHAIN_TAKE)
    if (HUGE) lds_left = JTK_HUGE_LDS;  // from here on an array that does not fit goes to the workspace (host twin: mcmc_ws_bytes)
    JTK_CHAIN_SIZED_HEAD(JTK_CHAIN_TAKE)
    const uint32_t npad = m.npad = JTK_CHAIN_NPAD(n);  // row stride of stab (here, not above: see chain_layout.h)
    JTK_CHAIN_SIZED_TABLES(JTK_CHAIN_TAKE)
#undef JTK_CHAIN_TAKE
    // The k-means scratch (and, in its place, the diploid chain's 16-byte entries) shares the first 16 n bytes of stab: stab is
    // rebuilt by the first publish() of every K-way chain (umask starts as "never built") and nothing reads it between chains,
    // k-means and get_read_lk_gains run only between them.  2.5 KB per chunk at 160 reads -- what a 4-copy pile-up's work area
    // (55.7 KB) was above a third of a CU's LDS: three chain workgroups per CU instead of two (cfg 4).
    m.fbuf = m.stab;
    m.cum = m.stab + n;
    m.shape = sh;
    return m;
}

}  // namespace
