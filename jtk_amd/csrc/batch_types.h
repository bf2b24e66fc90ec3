// batch_types.h -- the plain constants and records of a resident batch: what the kernels read (device_common.h), what the
// session keeps (session_internal.h) and what the host-only batch plan fills in (session_plan.h).  No HIP include: the
// plan and its test compile this with a plain C++ compiler.
#pragma once
#include <stdint.h>

#define JTK_WAVE 64
#define JTK_MAX_RADIUS 30        // 2r+1 <= 61 lanes: 3 spare lanes make the lane ring unambiguous (phmm_kernel)
#define JTK_WIDE_MAX_RADIUS 255  // wider bands (CLR / None reads, long ONT chunks) take phmm_wide_kernel (LDS frames of 256 / 512 cells)
#define JTK_PAIR_MAX_RADIUS 14   // 2r+1 <= 29 cells + 3 spare lanes fit a 32-lane half: phmm_pair_kernel runs two reads per wave
#define JTK_SCALE_BLOCK 64       // one power-of-two exponent per 64 anti-diagonals (oracle/phmm.c)
#define JTK_SCRATCH_GUARD 16     // zero rows in front of a wave's forward stripe (phmm_kernel reads pairs of diagonals >= -13)
#define JTK_ACC_N 16             // accumulators per template row (see phmm_kernels.hip)
#define JTK_LOG_ZERO (-1.0e300)
#define JTK_LN2 0.6931471805599453094
#define JTK_POS_THR 0.00001      // pseudo_mcmc.rs:5
#define JTK_MASK_LENGTH 7        // pseudo_mcmc.rs:3
#define JTK_MAX_HOMOP_LENGTH 2   // pseudo_mcmc.rs:4
#define JTK_MAX_COPY 7           // one clustering() call sees copy_num < 8 (UPPER_COPY_NUM, mod.rs:85); larger chunks
                                 // go through clustering_recursive's split, which session_split.hip drives
#define JTK_TRACE_MAX_PICKS 64    // jtk_lc_session_trace: picks recorded per chunk (ROUND * max(copy_num, 2) <= 21 of them happen)
#define JTK_MAX_DIM (3 * JTK_MAX_COPY)  // ROUND * max(copy_num, 2) picked columns (pseudo_mcmc.rs:421,527,532)
#define JTK_MAX_PILEUP 1023      // reads per pile-up in the chain kernel: 10-bit read indices in its proposal records and hop
                                 // words (register tables to 255 reads, LDS tables beyond); the LDS work area (n x D
                                 // doubles + tables) has to fit 160 KiB as well: session_plan.h sizes it per launch
#define JTK_POLISH_MIN_GAIN 0.1
#define JTK_POLISH_MAX_ROUNDS 20

// One read of the resident batch.
struct ReadMeta {
    uint32_t chunk;      // index into ChunkMeta
    uint32_t read_len;   // n
    uint64_t ey_off;     // into d_ey: ey[j] = y[j-1] | ctx(j)<<2 for j = 1..n (ey[0] unused)
    uint64_t ops_off;    // into d_ops[cur] (capacity slot)
    uint32_t ops_cap;
    uint32_t strand;     // 1 = forward model
    uint64_t delta_off;  // into d_delta (u64 words)
    uint64_t table_off;  // the read's table, JTK_NUM_ROW doubles per position: == raw_off (finalize_kernel works in place)
    uint64_t raw_off;    // into d_raw (doubles): JTK_ACC_N * (tmpl_cap + 1) per read; row sums, then the table
    uint64_t row_off;    // into d_rawG (ints): tmpl_cap + 1 per read
};

// One chunk (pile-up) of the resident batch.
struct ChunkMeta {
    uint64_t chunk_id;
    uint32_t copy_num;
    uint32_t n_reads;
    uint32_t read_first;
    uint32_t tmpl_cap;   // capacity of each template buffer
    uint64_t tmpl_off;   // into d_tmpl[cur]
    uint64_t total_off;  // into d_total (doubles): JTK_NUM_ROW * (tmpl_cap + 1)
    uint32_t radius;     // band radius for this chunk: ceil(len0 * band_frac) / 2 (mod.rs:96,105)
    uint32_t edit_cap;   // capacity of this chunk's edit list
    uint64_t edit_off;   // into d_edits
    uint64_t feat_off;   // into d_feat (doubles): n_reads * JTK_MAX_DIM
    uint64_t cand_off;   // into d_cand (doubles): JTK_NUM_ROW * (tmpl_cap + 1) candidate scores
    double local_coverage;  // ClusteringConfig.local_coverage (mod.rs:108-112)
    uint32_t take_num;   // HMMPolishConfig take_num: only the first take_num reads vote in a polish round (0 = all)
    uint32_t pad0;
};

// Mutable per-chunk state (device resident).
struct ChunkState {
    uint32_t tmpl_len;   // current template length
    uint32_t buf;        // which of the two template / ops buffers is current
    uint32_t active;     // 1 while polishing has not converged
    uint32_t rounds;     // polish rounds executed
    int32_t status;      // jtk_status of this chunk
    uint32_t n_edits;    // edits selected in the current round
    uint32_t dim;        // D selected variant columns
    uint32_t k;          // cluster_num
    double score;
    uint64_t draws;      // RNG stream positions the clustering consumed
    uint64_t chain_cycles;  // shader-clock cycles the chunk's consumer wave spent in the chain kernel (jtk_lc_debug_chain_profile)
    uint32_t chain_events;  // proposals of its table-driven chains that could not be stepped over
    uint32_t chain_pad;
};

struct HmmDev {
    double a[9];      // mat_mat, mat_ins, mat_del, ins_mat, ins_ins, ins_del, del_mat, del_ins, del_del
    double eM[16];
    double eI[20];
};

struct Edit {
    uint32_t pos;
    uint32_t row;
};

// The three buffer sets (template codes, per-base ops and their lengths); ChunkState.buf selects the current one.  Set 0
// holds the batch as uploaded and is never written: a pass starts from it without a device-to-device reset copy; the first
// polish round that edits a chunk writes set 1, later rounds ping-pong between 1 and 2.  Passed to kernels by value.
struct DevBufs {
    uint8_t *tmpl[3];
    uint8_t *ops[3];
    uint32_t *ops_len[3];
};
#define JTK_NEXT_BUF(b) ((b) == 0u ? 1u : 3u - (b))

// what a sub-problem inherits from its chunk instead of deriving it from its own template / read count
struct ChunkExtra {
    uint32_t radius;        // config.band_width (mod.rs:112,142,153)
    double local_coverage;  // config.local_coverage (mod.rs:108-112)
    uint64_t rng[4];        // the chunk's generator, as the previous call left it (mod.rs:158)
    uint32_t take_num;      // HMMPolishConfig take_num (0 = every read votes)
};

// One launch of the chain kernel: a range of the launch order and the (reads, columns, clusters) its work area is sized for.
struct ChainClass {
    uint32_t first = 0, count = 0, lds_n = 0, lds_d = 0, lds_k = 0, lds_bytes = 0;
};
