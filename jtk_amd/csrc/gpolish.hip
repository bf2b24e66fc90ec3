// gpolish.hip -- jtk_lc_polish_guided: consensus polishing that votes with banded edit distances; what the reference gets from
// kiley::bialignment::guided::polish_until_converge(_with) (encode/deletion_fill.rs:260-285, polish_chunks.rs:64-65,
// consensus/mod.rs:442,470-472, determine_chunks.rs:439, dense_encoding.rs:575-577).  Specification: DESIGN.md section 4,
// "Guided polishing"; it is this build's own, parity with kiley's polish is not pinned.
//
// A round is five launches on one stream, and only the count of pile-ups still active crosses to the host:
//   1. gp_begin_kernel: a pile-up whose template has nothing to scan stops; the others get their gain table zeroed.
//   2. gp_fill_kernel, one wave per (pile-up, read), slice behind slice of the work area:
//        the band from the read's current ops (jtk_band_rows, wave_util.h);
//        the forward fill, rows in order, lanes over the columns, 64 at a time: the left neighbour is a prefix minimum with slope
//        +1, F(i, j) = j + min_{k <= j} (g(k) - k), g the better of the two moves from the row above (six __shfl_up steps and a
//        carry between the pieces).  F is kept whole as 16-bit cells (n + m <= 64,000; 65,535 is +infinity), the two rows the
//        recurrence needs also in a ring of four rows (LDS where the widest row has at most GP_LDS_WIDTH cells, global otherwise);
//        the walk back over the stored F (lanes 0..2 fetch the three predecessors at once), 64 ops per store;
//        for a voting read the backward fill from row n down, mirrored (the right neighbour is the prefix minimum of the columns
//        counted from the right), B only in the ring; at row p the 14 table entries are minima over the columns of row p of sums
//        of F rows p..p+3 and B rows p..p+3: per-lane minima over the pieces, then 14 wave reductions, and lanes 0..13 add
//        dist - T to the pile-up's int32 gains (atomics; integers, so the order is free) or mark the entry dead.
//   3. gp_select_kernel: the left-to-right scan (first best row, applied when >= 1) and the edited template.
//   4. gp_rethread_kernel: the local surgery of every read's ops (rules of rethread_kernel, polish_kernels.hip).
//   5. gp_commit_kernel: flips the template buffers and stores the number of pile-ups still active in mapped host memory.
// After the last round one more gp_fill_kernel pass (no table) runs for the pile-ups whose ops do not belong to their consensus.
#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#include "guided_internal.h"
#include "jtk_lc_debug.h"
#include "wave_util.h"

namespace {

constexpr int32_t GP_BIG = 1 << 20;                // +infinity in registers: finite sums stay below 2 x 64,000
constexpr uint32_t GP_INF16 = 65535;               // +infinity in a stored cell
constexpr uint32_t GP_MAX_LEN = 32000;             // as the guided aligner
constexpr uint32_t GP_MAX_WIDTH = JTK_GUIDED_MAX_WIDTH;
constexpr uint32_t GP_WAVES = 4;                   // waves per block
constexpr uint32_t GP_LDS_WIDTH = 512;             // 4 rows x 2 bytes x 512 cells = 4 KiB per wave, 16 KiB per block
constexpr uint32_t GP_ROWS = 14;
constexpr uint32_t GP_DEFAULT_ROUNDS = 20;
constexpr uint32_t GP_DEAD = 0xffffffffu;

struct GpPile {  // constant over the call
    uint64_t tmpl_off;  // into each of the two template buffers; tmpl_cap bytes
    uint64_t gain_off;  // into gain / dead: (tmpl_cap + 1) x 14 entries
    uint64_t edit_off;
    uint32_t tmpl_cap, edit_cap, n_reads, read_first, radius, pad;
};
struct GpState {
    int32_t status;
    uint32_t active;   // still polishing
    uint32_t dirty;    // the reads' ops and distances do not belong to the current template
    uint32_t rounds, n, buf, n_edits, new_n;
};
struct GpRead {  // constant over the call
    uint64_t y_off;     // into the read bases
    uint64_t ops_off;   // into the ops area: two halves of ops_cap bytes
    uint64_t tab_off;   // share of the slice: 2 (tmpl_cap + 2) uint32
    uint64_t f_off, f_cap;  // share of the slice: F cells
    uint64_t ring_off;  // 4 x GP_MAX_WIDTH cells where a row may pass GP_LDS_WIDTH
    uint32_t pile, m, ops_cap, rank;  // rank: index inside the pile-up
};
struct GpReadState {
    uint32_t at, len;  // the current ops inside the read's ops area
    uint32_t dist, pad;
};
struct GpEdit {
    uint32_t pos, row;
};

struct GpArgs {
    uint32_t first, count;  // the slice (reads)
    const GpPile *piles;
    GpState *state;
    const GpRead *reads;
    GpReadState *rstate;
    uint8_t *tmpl[2];
    const uint8_t *y;
    uint8_t *ops;
    uint32_t *tab;
    uint16_t *f, *ring;
    int32_t *gain;
    uint32_t *dead;
    GpEdit *edits;
    uint32_t *dbg_table;  // jtk_lc_debug_guided_table: per read (tmpl_cap + 1) x 14
    unsigned long long *cells;  // [0] band cells filled forward, [1] of them by voting reads (whose table reads F four times over)
    uint32_t take_num, ignore_edge;
    int final_pass;
};

__device__ __forceinline__ int32_t gp_min(int32_t a, int32_t b) { return a < b ? a : b; }
__device__ __forceinline__ int32_t gp_ld(const uint16_t *p) {
    const uint32_t v = *p;
    return v == GP_INF16 ? GP_BIG : (int32_t)v;
}
__device__ __forceinline__ uint16_t gp_sat(int32_t v) { return (uint16_t)(v >= (int32_t)GP_INF16 ? GP_INF16 : (uint32_t)v); }
__device__ __forceinline__ int32_t gp_scan_min(int32_t t, uint32_t lane) {
#pragma unroll
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const int32_t u = __shfl_up(t, o, 64);
        if (lane >= o) t = gp_min(t, u);
    }
    return t;
}
__device__ __forceinline__ uint8_t gp_base(uint32_t b) { return b == 0 ? 'A' : (b == 1 ? 'C' : (b == 2 ? 'G' : 'T')); }

// One read of one round.  ring: 4 rows of `stride` cells.
__device__ void gp_read(const GpArgs &a, uint32_t r, const GpPile &pl, GpState *st, uint32_t n, const uint32_t *lo, const uint32_t *off,
                        uint16_t *ring, uint32_t stride, bool vote, uint32_t lane) {
    const GpRead rd = a.reads[r];
    const uint32_t m = rd.m;
    const uint8_t *x = a.tmpl[st->buf] + pl.tmpl_off, *y = a.y + rd.y_off;
    uint16_t *f = a.f + rd.f_off;
    // ---- forward: row i into f and into ring row i & 1
    {
        uint32_t prev_first = 1, prev_width = 0;
        for (uint32_t i = 0; i <= n; i++) {
            const uint32_t cb = lo[i], at = off[i], width = off[i + 1] - at;
            const uint8_t xi = i ? x[i - 1] : 0;
            uint16_t *cur = ring + (i & 1u) * stride;
            const uint16_t *prev = ring + ((i & 1u) ^ 1u) * stride;
            int32_t run = GP_BIG;
            for (uint32_t base = 0; base < width; base += 64) {
                const uint32_t c = base + lane, j = cb + c;
                int32_t g = GP_BIG;
                if (c < width) {
                    if (i == 0 && j == 0) g = 0;
                    if (i > 0) {
                        const uint32_t dc = j - 1 - prev_first;
                        if (j >= 1 && j - 1 >= prev_first && dc < prev_width) g = gp_ld(prev + dc) + (xi != y[j - 1] ? 1 : 0);
                        const uint32_t uc = j - prev_first;
                        if (j >= prev_first && uc < prev_width) g = gp_min(g, gp_ld(prev + uc) + 1);
                    }
                }
                int32_t t = gp_min(gp_scan_min(g - (int32_t)c, lane), run);
                run = __shfl(t, 63, 64);
                if (c < width) {
                    const uint16_t v = gp_sat(t + (int32_t)c);
                    cur[c] = v;
                    f[(uint64_t)at + c] = v;
                }
            }
            jtk_wave_sync();
            prev_first = cb;
            prev_width = width;
        }
    }
    const uint32_t last_w = off[n + 1] - off[n];
    const int32_t dist = gp_ld(ring + (n & 1u) * stride + (last_w - 1));  // row n ends at column m
    // ---- the walk back over F: diagonal, then Del, then Ins; op k from the end goes to slot_last - k
    const GpReadState rs = a.rstate[r];
    const uint32_t half = rs.at >= rd.ops_cap ? 0u : 1u;  // the half the guide is not in
    uint8_t *slot_last = a.ops + rd.ops_off + (uint64_t)half * rd.ops_cap + rd.ops_cap - 1;
    uint32_t k = 0;
    bool lost = dist >= GP_BIG;
    {
        uint32_t i = n, j = m, held = 0;
        int32_t val = dist;
        uint32_t c_lo = lo[n], c_off = off[n];
        uint32_t p_lo = n ? lo[n - 1] : 0, p_off = n ? off[n - 1] : 0;
        const uint32_t max_steps = n + m;
        while (!lost && (i > 0 || j > 0)) {
            if (k >= max_steps) {
                lost = true;
                break;
            }
            const uint32_t p_w = c_off - p_off;  // width of row i - 1 (i > 0)
            int32_t cand = GP_BIG;
            if (lane == 0) {
                if (i > 0 && j > 0 && j - 1 >= p_lo && j - 1 - p_lo < p_w)
                    cand = gp_ld(f + (uint64_t)p_off + (j - 1 - p_lo)) + (x[i - 1] != y[j - 1] ? 1 : 0);
            } else if (lane == 1) {
                if (i > 0 && j >= p_lo && j - p_lo < p_w) cand = gp_ld(f + (uint64_t)p_off + (j - p_lo)) + 1;
            } else if (lane == 2) {
                if (j > 0 && j - 1 >= c_lo) cand = gp_ld(f + (uint64_t)c_off + (j - 1 - c_lo)) + 1;
            }
            const unsigned long long hit = __ballot(lane < 3 && cand == val && cand < GP_BIG);
            if (!hit) {
                lost = true;
                break;
            }
            const uint32_t move = (uint32_t)__ffsll((long long)hit) - 1;
            const int32_t got = __shfl(cand, (int)move, 64);
            uint32_t op;
            if (move == 0) {
                const bool mis = x[i - 1] != y[j - 1];
                op = mis ? JTK_OP_MISMATCH : JTK_OP_MATCH;
                val = got - (mis ? 1 : 0);
                i--;
                j--;
            } else if (move == 1) {
                op = JTK_OP_DEL;
                val = got - 1;
                i--;
            } else {
                op = JTK_OP_INS;
                val = got - 1;
                j--;
            }
            if (move != 2) {
                c_lo = p_lo;
                c_off = p_off;
                if (i > 0) {
                    p_lo = lo[i - 1];
                    p_off = off[i - 1];
                }
            }
            if (lane == (k & 63u)) held = op;
            k++;
            if ((k & 63u) == 0) *(slot_last - (k - 64 + lane)) = (uint8_t)held;
        }
        if (k & 63u) {
            if (lane < (k & 63u)) *(slot_last - ((k & ~63u) + lane)) = (uint8_t)held;
        }
    }
    if (lost) {
        if (lane == 0) atomicCAS(&st->status, 0, (int)JTK_ERR_INTERNAL);
        return;
    }
    if (lane == 0) {
        GpReadState out;
        out.at = half * rd.ops_cap + rd.ops_cap - k;
        out.len = k;
        out.dist = (uint32_t)dist;
        out.pad = 0;
        a.rstate[r] = out;
    }
    if (!vote) return;
    // ---- backward, row i into ring row i & 3, columns counted from the right; then the table entries of position i
    jtk_wave_sync();
    int32_t *gain = a.gain + pl.gain_off;
    uint32_t *dead = a.dead + pl.gain_off;
    uint32_t *dbg = a.dbg_table ? a.dbg_table + ((uint64_t)rd.rank * (pl.tmpl_cap + 1)) * GP_ROWS : nullptr;
    uint32_t lo_[4] = {0, 0, 0, 0}, w_[4] = {0, 0, 0, 0}, of_[4] = {0, 0, 0, 0};  // rows i .. i + 3; w = 0: no such row
    for (uint32_t i = n;; i--) {
#pragma unroll
        for (int q = 3; q > 0; q--) {
            lo_[q] = lo_[q - 1];
            w_[q] = w_[q - 1];
            of_[q] = of_[q - 1];
        }
        lo_[0] = lo[i];
        of_[0] = off[i];
        w_[0] = off[i + 1] - of_[0];
        const uint32_t width = w_[0], cb = lo_[0];
        uint16_t *cur = ring + (i & 3u) * stride;
        const uint16_t *nxt = ring + ((i + 1) & 3u) * stride;
        const uint8_t xi = i < n ? x[i] : 0;
        {
            int32_t run = GP_BIG;
            for (uint32_t base = 0; base < width; base += 64) {
                const uint32_t q = base + lane;
                int32_t g = GP_BIG;
                uint32_t c = 0;
                if (q < width) {
                    c = width - 1 - q;
                    const uint32_t j = cb + c;
                    if (i == n && j == m) g = 0;
                    if (i < n) {
                        const uint32_t dc = j + 1 - lo_[1];
                        if (j < m && j + 1 >= lo_[1] && dc < w_[1]) g = gp_ld(nxt + dc) + (xi != y[j] ? 1 : 0);
                        const uint32_t uc = j - lo_[1];
                        if (j >= lo_[1] && uc < w_[1]) g = gp_min(g, gp_ld(nxt + uc) + 1);
                    }
                }
                int32_t t = gp_min(gp_scan_min(g - (int32_t)q, lane), run);
                run = __shfl(t, 63, 64);
                if (q < width) cur[c] = gp_sat(t + (int32_t)q);
            }
        }
        jtk_wave_sync();
        {
            const uint32_t p = i;
            int32_t acc[GP_ROWS];
#pragma unroll
            for (uint32_t e = 0; e < GP_ROWS; e++) acc[e] = GP_BIG;
            for (uint32_t base = 0; base < width; base += 64) {
                const uint32_t c = base + lane;
                if (c >= width) continue;
                const uint32_t j = cb + c;
                const int32_t fp = gp_ld(f + (uint64_t)of_[0] + c);
                const int32_t bp = gp_ld(cur + c);
                const uint8_t yj = j < m ? y[j] : 0;
                // insert b before p: (p, j) -> (p, j + 1) with b on y_j, or b against nothing
                const int32_t ins_d = (j < m && c + 1 < width) ? fp + gp_ld(cur + c + 1) : GP_BIG;
                const int32_t ins_g = fp + 1 + bp;
                // substitute b at p: (p, j) -> (p + 1, j + 1) with b on y_j, or b against nothing -> (p + 1, j)
                int32_t sub_d = GP_BIG, sub_g = GP_BIG;
                if (p < n) {
                    const uint32_t dc = j + 1 - lo_[1];
                    if (j < m && j + 1 >= lo_[1] && dc < w_[1]) sub_d = fp + gp_ld(nxt + dc);
                    const uint32_t uc = j - lo_[1];
                    if (j >= lo_[1] && uc < w_[1]) sub_g = fp + 1 + gp_ld(nxt + uc);
                }
#pragma unroll
                for (uint32_t b = 0; b < 4; b++) {
                    const int32_t ne = gp_base(b) != yj ? 1 : 0;
                    acc[b] = gp_min(acc[b], gp_min(sub_d + ne, sub_g));
                    acc[4 + b] = gp_min(acc[4 + b], gp_min(ins_d + ne, ins_g));
                }
#pragma unroll
                for (uint32_t d = 1; d <= 3; d++) {
                    const uint32_t kc = j - lo_[d];
                    if (j >= lo_[d] && kc < w_[d]) {
                        // copy d: F(p + d, j) + B(p, j); delete d: F(p, j) + B(p + d, j)
                        if (p + d <= n) acc[7 + d] = gp_min(acc[7 + d], gp_ld(f + (uint64_t)of_[d] + kc) + bp);
                        if (p + d < n) acc[10 + d] = gp_min(acc[10 + d], fp + gp_ld(ring + ((p + d) & 3u) * stride + kc));
                    }
                }
            }
            int32_t mine = GP_BIG;
#pragma unroll
            for (uint32_t e = 0; e < GP_ROWS; e++) {
                int32_t v = acc[e];
#pragma unroll
                for (uint32_t o = 32; o; o >>= 1) v = gp_min(v, __shfl_xor(v, o, 64));
                if (lane == e) mine = v;
            }
            if (lane < GP_ROWS) {
                const uint64_t at = (uint64_t)p * GP_ROWS + lane;
                if (mine >= GP_BIG)
                    atomicOr(dead + at, 1u);
                else
                    atomicAdd(gain + at, dist - mine);
                if (dbg) dbg[at] = mine >= GP_BIG ? GP_DEAD : (uint32_t)mine;
            }
        }
        jtk_wave_sync();  // ring row (i + 3) & 3 is the next row's
        if (i == 0) break;
    }
}

__global__ void __launch_bounds__(GP_WAVES * 64) gp_fill_kernel(GpArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint16_t gp_lds[];
    const uint32_t lane = threadIdx.x & 63u, wave_in_block = threadIdx.x >> 6;
    const uint32_t w = blockIdx.x * GP_WAVES + wave_in_block;
    if (w >= a.count) return;
    const uint32_t r = a.first + w;
    const GpRead rd = a.reads[r];
    const GpPile pl = a.piles[rd.pile];
    GpState *st = a.state + rd.pile;
    const int32_t status = __builtin_amdgcn_readfirstlane(st->status);
    const uint32_t go = (uint32_t)__builtin_amdgcn_readfirstlane((int)(a.final_pass ? st->dirty : st->active));
    if (status != 0 || !go) return;
    const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)st->n);
    uint32_t *lo = a.tab + rd.tab_off, *off = lo + (n + 2);
    const GpReadState rs = a.rstate[r];
    uint32_t total = 0;
    const uint32_t widest = jtk_band_rows(n, rd.m, pl.radius, a.ops + rd.ops_off + rs.at, rs.len, lo, off, lane, &total);
    jtk_wave_sync();
    const uint32_t cells = off[n + 1];  // (== total) read back behind the barrier, like the rows
    if (widest > GP_MAX_WIDTH || cells > rd.f_cap) {
        // the host's bound holds for every guide: the second case has never been seen
        if (lane == 0) atomicCAS(&st->status, 0, widest > GP_MAX_WIDTH ? (int)JTK_ERR_UNSUPPORTED : (int)JTK_ERR_INTERNAL);
        return;
    }
    const bool vote = !a.final_pass && (a.take_num == 0 || rd.rank < a.take_num);
    if (lane == 0) {
        atomicAdd(a.cells, (unsigned long long)cells);
        if (vote) atomicAdd(a.cells + 1, (unsigned long long)cells);
    }
    if (widest <= GP_LDS_WIDTH)
        gp_read(a, r, pl, st, n, lo, off, gp_lds + wave_in_block * 4 * GP_LDS_WIDTH, GP_LDS_WIDTH, vote, lane);
    else
        gp_read(a, r, pl, st, n, lo, off, a.ring + rd.ring_off, GP_MAX_WIDTH, vote, lane);
}

// A round begins: nothing to scan ends the pile-up (the round counts), otherwise the gains start from zero.
__global__ void __launch_bounds__(256) gp_begin_kernel(const GpPile *piles, GpState *state, int32_t *gain, uint32_t *dead, uint32_t ignore_edge,
                                                      int scan) {
    const GpPile pl = piles[blockIdx.x];
    GpState *st = state + blockIdx.x;
    if (st->status != 0 || !st->active) return;
    const uint32_t n = st->n;
    __syncthreads();
    if (scan && 2ull * ignore_edge >= n) {
        if (threadIdx.x == 0) {
            st->active = 0;
            st->rounds++;
        }
        return;
    }
    const uint32_t cnt = (n + 1) * GP_ROWS;
    for (uint32_t q = threadIdx.x; q < cnt; q += 256) {
        gain[pl.gain_off + q] = 0;
        dead[pl.gain_off + q] = 0;
    }
}

// One wave per pile-up: lanes find the first best row of every position, lane 0 does the scan and writes the edited template.
__global__ void __launch_bounds__(64) gp_select_kernel(const GpPile *piles, GpState *state, uint8_t *tmpl0, uint8_t *tmpl1, const int32_t *gain_all,
                                                       const uint32_t *dead_all, GpEdit *edits_all, uint32_t ignore_edge) {
    extern __shared__ unsigned char gp_best[];  // per position: best row | 0x80 where it is applied
    const GpPile pl = piles[blockIdx.x];
    GpState *st = state + blockIdx.x;
    if (st->status != 0 || !st->active) return;
    const uint32_t n = st->n;
    const int32_t *gain = gain_all + pl.gain_off;
    const uint32_t *dead = dead_all + pl.gain_off;
    for (uint32_t p = threadIdx.x; p < n; p += 64) {
        uint32_t best = 0;
        int32_t g = INT_MIN;
        for (uint32_t row = 0; row < GP_ROWS; row++) {
            const int32_t v = dead[p * GP_ROWS + row] ? INT_MIN : gain[p * GP_ROWS + row];
            if (v > g) {
                g = v;
                best = row;
            }
        }
        gp_best[p] = (unsigned char)(best | (g >= 1 ? 0x80u : 0u));
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const uint32_t round = st->rounds;
    const uint32_t inactive = 5 + (5 * round) % 21;
    GpEdit *edits = edits_all + pl.edit_off;
    uint32_t ne = 0, pos = ignore_edge, grow = 0;
    while (pos + ignore_edge < n) {
        const unsigned char b = gp_best[pos];
        if ((b & 0x80u) && ne < pl.edit_cap) {
            const uint32_t row = b & 0x7fu;
            edits[ne].pos = pos;
            edits[ne].row = row;
            ne++;
            grow += row >= 4 && row < 8 ? 1u : (row >= 8 && row < 11 ? row - 7 : 0u);
            pos += (row >= 11 ? row - 10 : 1) + inactive;
        } else {
            pos++;
        }
    }
    st->rounds = round + 1;
    st->n_edits = ne;
    st->dirty = 0;  // this round's fill belongs to this template
    if (ne == 0) {
        st->active = 0;
        return;
    }
    if (n + grow > pl.tmpl_cap) {
        st->status = JTK_ERR_CHUNK_FAILED;
        return;
    }
    const uint8_t *src = (st->buf ? tmpl1 : tmpl0) + pl.tmpl_off;
    uint8_t *dst = (st->buf ? tmpl0 : tmpl1) + pl.tmpl_off;
    uint32_t w = 0, e = 0, p = 0;
    while (p < n) {
        if (e < ne && edits[e].pos == p) {
            const uint32_t row = edits[e].row;
            e++;
            if (row < 4) {
                dst[w++] = gp_base(row);
                p++;
            } else if (row < 8) {
                dst[w++] = gp_base(row - 4);
                dst[w++] = src[p++];
            } else if (row < 11) {
                const uint32_t c = row - 7;  // exists: p + c <= n
                for (uint32_t q = 0; q < c; q++) dst[w++] = src[p + q];
                dst[w++] = src[p++];
            } else {
                p += row - 10;
            }
        } else {
            dst[w++] = src[p++];
        }
    }
    st->new_n = w;
}

// The rules of rethread_kernel (polish_kernels.hip) on this file's buffers: one wave per read, 64 ops per step.
__global__ void __launch_bounds__(GP_WAVES * 64) gp_rethread_kernel(uint32_t n_reads, const GpPile *piles, const GpState *state, const GpRead *reads,
                                                                    GpReadState *rstate, const uint8_t *tmpl0, const uint8_t *tmpl1, const uint8_t *y_all,
                                                                    uint8_t *ops_all, const GpEdit *edits_all) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t r = blockIdx.x * GP_WAVES + (threadIdx.x >> 6);
    if (r >= n_reads) return;
    const GpRead rd = reads[r];
    const GpState *st = state + rd.pile;
    if (st->status != 0 || !st->active || st->n_edits == 0) return;
    const GpPile pl = piles[rd.pile];
    const uint32_t ne = st->n_edits;
    const GpEdit *edits = edits_all + pl.edit_off;
    const GpReadState rs = rstate[r];
    const uint32_t to = rs.at >= rd.ops_cap ? 0u : rd.ops_cap;
    const uint8_t *ops = ops_all + rd.ops_off + rs.at;
    uint8_t *out = ops_all + rd.ops_off + to;
    const uint32_t n_ops = rs.len;
    const uint8_t *tmpl = (st->buf ? tmpl0 : tmpl1) + pl.tmpl_off;  // the edited template
    const uint8_t *y = y_all + rd.y_off;
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t w0 = 0, ti0 = 0, ni0 = 0, nj0 = 0;  // uniform: ops written, old template bases consumed, new template / read position
    uint32_t e_cur = 0;
    bool overflow = false;
    auto inserted = [](uint32_t row) { return row >= 4 && row < 8 ? 1u : (row >= 8 && row < 11 ? row - 7 : 0u); };
    if (edits[0].pos == 0 && edits[0].row >= 4 && edits[0].row < 11) {  // an insertion edit at position 0 fires before the first op
        const uint32_t k = inserted(edits[0].row);
        if (lane < k && lane < rd.ops_cap) out[lane] = JTK_OP_DEL;
        overflow = overflow || k > rd.ops_cap;
        w0 = k;
        ni0 = k;
    }
    for (uint32_t base = 0; base < n_ops; base += 64) {
        const uint32_t kk = base + lane;
        const bool has = kk < n_ops;
        const uint32_t op = has ? ops[kk] : (uint32_t)JTK_OP_INS;
        const bool cons = has && op != JTK_OP_INS;
        const unsigned long long mc = __ballot(cons);
        const uint32_t ti = ti0 + (uint32_t)__popcll(mc & below);
        while (e_cur < ne) {
            const GpEdit ed = edits[e_cur];
            const uint32_t last = ed.row >= 11 ? ed.pos + (ed.row - 10) - 1 : (ed.row >= 4 ? ed.pos - 1 : ed.pos);
            if ((ed.row >= 4 && ed.row < 11 && ed.pos == 0) || last < ti0)
                e_cur++;
            else
                break;
        }
        uint32_t first = has ? op : 4u;  // what the op becomes: an op code, or 4 = nothing
        uint32_t k_del = 0;              // Del ops that follow it
        if (cons) {
            for (uint32_t e = e_cur; e < ne; e++) {
                const GpEdit ed = edits[e];
                if (ed.pos > ti + 1) break;
                if (ed.row >= 11) {
                    if (ed.pos <= ti && ti < ed.pos + (ed.row - 10)) first = op != JTK_OP_DEL ? (uint32_t)JTK_OP_INS : 4u;
                } else if (ed.row >= 4 && ed.pos == ti + 1) {
                    k_del = inserted(ed.row);
                }
            }
        }
        const uint32_t c_out = (first != 4u ? 1u : 0u) + k_del;
        const uint32_t c_t = ((first <= JTK_OP_MISMATCH || first == JTK_OP_DEL) ? 1u : 0u) + k_del;
        const uint32_t c_r = (first <= JTK_OP_MISMATCH || first == JTK_OP_INS) ? 1u : 0u;
        const uint32_t packed = c_out | c_t << 10 | c_r << 20;
        uint32_t incl = packed;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u = __shfl_up(incl, o, 64);
            if ((int)lane >= o) incl += u;
        }
        const uint32_t excl = incl - packed, total = __shfl(incl, 63, 64);
        uint32_t w = w0 + (excl & 1023u);
        const uint32_t ni = ni0 + ((excl >> 10) & 1023u), nj = nj0 + (excl >> 20);
        if (first != 4u) {
            uint32_t o1 = first;
            if (first <= JTK_OP_MISMATCH) o1 = tmpl[ni] == y[nj] ? JTK_OP_MATCH : JTK_OP_MISMATCH;
            if (w < rd.ops_cap) out[w] = (uint8_t)o1;
            w++;
        }
        for (uint32_t q = 0; q < k_del; q++)
            if (w + q < rd.ops_cap) out[w + q] = JTK_OP_DEL;
        w0 += total & 1023u;
        ni0 += (total >> 10) & 1023u;
        nj0 += total >> 20;
        ti0 += (uint32_t)__popcll(mc);
        overflow = overflow || w0 > rd.ops_cap;
    }
    if (lane == 0) {
        GpReadState o = rs;
        o.at = to;
        o.len = overflow ? rd.ops_cap : w0;
        rstate[r] = o;
        if (overflow) atomicCAS(const_cast<int32_t *>(&st->status), 0, (int)JTK_ERR_CHUNK_FAILED);
    }
}

__global__ void __launch_bounds__(256) gp_commit_kernel(uint32_t n_piles, GpState *state, uint32_t *n_active_host) {
    uint32_t mine = 0;
    for (uint32_t ci = threadIdx.x; ci < n_piles; ci += 256) {
        GpState *st = &state[ci];
        if (st->status != 0 || !st->active) continue;
        if (st->n_edits > 0) {
            st->buf ^= 1u;
            st->n = st->new_n;
            st->n_edits = 0;
            st->dirty = 1;
        }
        mine++;
    }
    __shared__ uint32_t s_total;
    if (threadIdx.x == 0) s_total = 0;
    __syncthreads();
    if (mine) atomicAdd(&s_total, mine);
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(n_active_host, s_total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// blocks 0 .. n_reads - 1: a read's ops; then one block per pile-up: its consensus
__global__ void __launch_bounds__(256) gp_pack_kernel(uint32_t n_reads, uint32_t n_piles, const GpPile *piles, const GpState *state, const GpRead *reads,
                                                      const GpReadState *rstate, const uint8_t *tmpl0, const uint8_t *tmpl1, const uint8_t *ops,
                                                      const uint64_t *ops_dst, const uint64_t *cons_dst, uint8_t *ops_out, uint8_t *cons_out) {
    const uint32_t b = blockIdx.x;
    if (b < n_reads) {
        const uint32_t len = (uint32_t)(ops_dst[b + 1] - ops_dst[b]);
        const uint8_t *src = ops + reads[b].ops_off + rstate[b].at;
        for (uint32_t q = threadIdx.x; q < len; q += 256) ops_out[ops_dst[b] + q] = src[q];
    } else if (b - n_reads < n_piles) {
        const uint32_t c = b - n_reads;
        const uint32_t len = (uint32_t)(cons_dst[c + 1] - cons_dst[c]);
        const uint8_t *src = (state[c].buf ? tmpl1 : tmpl0) + piles[c].tmpl_off;
        for (uint32_t q = threadIdx.x; q < len; q += 256) cons_out[cons_dst[c] + q] = src[q];
    }
}

thread_local double g_gpolish_timing[8];  // jtk_lc_debug_gpolish_timing

uint64_t gp_cells_bound(uint32_t n, uint32_t m, uint32_t r) {
    const uint64_t rows = (uint64_t)n + 1, longest = std::max(n, m);
    const uint64_t rr = std::min<uint64_t>(r, longest + 1);
    const uint64_t by_path = (uint64_t)n + m + 1 + 2 * rr * rows;
    return std::min({rows * ((uint64_t)m + 1), by_path, rows * GP_MAX_WIDTH});
}

struct GpCount {  // the mapped host word gp_commit_kernel stores to
    uint32_t *h = nullptr;
    ~GpCount() {
        if (h) (void)hipHostFree(h);
    }
};

struct GpOut {
    std::vector<GpState> state;
    std::vector<GpReadState> rstate;
};

// The whole call after validation.  table_out != null: one round's fill of a single pile-up, nothing is applied.
int gp_run(size_t n_chunks, const jtk_lc_chunk_t *chunks, const uint8_t *tmpl_bases, const uint8_t *read_bases, const uint64_t *read_off,
           const uint8_t *ops, const uint64_t *ops_off, const uint32_t *radius, uint32_t take_num, uint32_t ignore_edge, uint32_t max_rounds,
           uint8_t *cons_out, uint64_t *cons_off, uint64_t cons_cap, uint8_t *ops_out, uint64_t *ops_out_off, uint64_t ops_cap, uint32_t *dist_out,
           jtk_lc_result_t *result, uint32_t *table_out) {
    const uint64_t n_reads = n_chunks ? chunks[n_chunks - 1].read_first + chunks[n_chunks - 1].n_reads : 0;
    if (n_chunks >= 0x7fffffffu || n_reads >= 0x7fffffffu) return jtk_fail(JTK_ERR_UNSUPPORTED, "2^31 - 1 pile-ups or reads, or more");
    std::vector<GpPile> piles(n_chunks);
    std::vector<GpState> state(n_chunks);
    std::vector<GpRead> reads(n_reads);
    std::vector<GpReadState> rstate(n_reads);
    uint64_t tmpl_bytes = 0, gain_n = 0, edit_n = 0, ops_bytes = 0, y_bytes = 0, max_cap = 0;
    for (size_t c = 0; c < n_chunks; c++) {
        const jtk_lc_chunk_t &ch = chunks[c];
        GpPile &pl = piles[c];
        GpState &st = state[c];
        std::memset(&pl, 0, sizeof pl);
        std::memset(&st, 0, sizeof st);
        bool ok = ch.tmpl_len <= GP_MAX_LEN;
        for (uint64_t r = ch.read_first; r < ch.read_first + ch.n_reads; r++) ok = ok && read_off[r + 1] - read_off[r] <= GP_MAX_LEN;
        const uint32_t n = ok ? (uint32_t)ch.tmpl_len : 0;
        pl.tmpl_off = tmpl_bytes;
        pl.gain_off = gain_n;
        pl.edit_off = edit_n;
        pl.tmpl_cap = ok ? std::min<uint32_t>(GP_MAX_LEN, n + 64 + n / 8) : 0;
        pl.edit_cap = pl.tmpl_cap / 6 + 2;
        pl.n_reads = ch.n_reads;
        pl.read_first = (uint32_t)ch.read_first;
        pl.radius = radius[c];
        tmpl_bytes += pl.tmpl_cap;
        gain_n += ((uint64_t)pl.tmpl_cap + 1) * GP_ROWS;
        edit_n += pl.edit_cap;
        max_cap = std::max<uint64_t>(max_cap, pl.tmpl_cap);
        st.status = ok ? 0 : JTK_ERR_UNSUPPORTED;
        st.active = ok;
        st.dirty = ok;
        st.n = n;
        for (uint32_t q = 0; q < ch.n_reads; q++) {
            const uint64_t r = ch.read_first + q;
            GpRead &rd = reads[r];
            std::memset(&rd, 0, sizeof rd);
            rd.pile = (uint32_t)c;
            rd.rank = q;
            rd.m = ok ? (uint32_t)(read_off[r + 1] - read_off[r]) : 0;
            rd.y_off = read_off[r];
            rd.ops_off = ops_bytes;
            const uint64_t in_len = ops_off[r + 1] - ops_off[r];
            rd.ops_cap = ok ? (uint32_t)std::max<uint64_t>(pl.tmpl_cap + rd.m, in_len) : 0;
            ops_bytes += 2ull * rd.ops_cap;
            rstate[r] = GpReadState{0, ok ? (uint32_t)in_len : 0, GP_DEAD, 0};
            y_bytes = std::max(y_bytes, read_off[r + 1]);
        }
    }
    // ---- shares of the work area (F cells, row tables, rings); a slice ends where the next read would pass the budget
    std::vector<uint32_t> slice_first;
    uint64_t tab_need = 0, f_need = 0, ring_need = 0, work_bytes = 0;  // work_bytes: every read's share, by the host's bound
    {
        const uint64_t cap = guided_scratch_cap();
        uint64_t tab_used = 0, f_used = 0, ring_used = 0;
        for (uint64_t r = 0; r < n_reads; r++) {
            GpRead &rd = reads[r];
            const GpPile &pl = piles[rd.pile];
            const bool skip = state[rd.pile].status != 0;
            const uint64_t cells = skip ? 0 : (gp_cells_bound(pl.tmpl_cap, rd.m, pl.radius) + 15) & ~15ull;
            const uint64_t tab = skip ? 0 : 2 * ((uint64_t)pl.tmpl_cap + 2);
            const uint64_t ring = (skip || rd.m + 1 <= GP_LDS_WIDTH) ? 0 : 4ull * GP_MAX_WIDTH;
            if (r == 0 || 2 * (f_used + cells) + 4 * (tab_used + tab) + 2 * (ring_used + ring) > cap) {
                slice_first.push_back((uint32_t)r);
                tab_used = f_used = ring_used = 0;
            }
            work_bytes += 2 * cells + 4 * tab + 2 * ring;
            rd.tab_off = tab_used;
            rd.f_off = f_used;
            rd.f_cap = cells;
            rd.ring_off = ring_used;
            tab_used += tab;
            f_used += cells;
            ring_used += ring;
            tab_need = std::max(tab_need, tab_used);
            f_need = std::max(f_need, f_used);
            ring_need = std::max(ring_need, ring_used);
        }
        slice_first.push_back((uint32_t)n_reads);
    }
    GpCount count;  // outlives the stream
    DevStream s;
    JTK_HIP_TRY(s.create(2));
    const uint32_t limit = table_out ? 1 : (max_rounds ? max_rounds : GP_DEFAULT_ROUNDS);
    JTK_HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&count.h), sizeof(uint32_t), hipHostMallocMapped));
    uint32_t *h_count_dev = nullptr;
    JTK_HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&h_count_dev), count.h, 0));
    count.h[0] = 0;  // every round waits for its count, so one slot serves them all
    const hipStream_t st = s.st;
    DevArr<GpPile> d_piles;
    DevArr<GpState> d_state;
    DevArr<GpRead> d_reads;
    DevArr<GpReadState> d_rstate;
    DevArr<uint8_t> d_t0, d_t1, d_y, d_ops;
    DevArr<uint32_t> d_tab, d_dead, d_dbg;
    DevArr<uint16_t> d_f, d_ring;
    DevArr<int32_t> d_gain;
    DevArr<GpEdit> d_edits;
    DevArr<unsigned long long> d_cells;
    {
        int rc;
        if ((rc = d_piles.upload(piles, st)) || (rc = d_state.upload(state, st)) || (rc = d_reads.upload(reads, st)) || (rc = d_rstate.upload(rstate, st)))
            return jtk_fail(rc, "device upload failed");
    }
    JTK_HIP_TRY(d_t0.alloc(tmpl_bytes));
    JTK_HIP_TRY(d_t1.alloc(tmpl_bytes));
    JTK_HIP_TRY(d_y.alloc(y_bytes));
    JTK_HIP_TRY(d_ops.alloc(ops_bytes));
    JTK_HIP_TRY(d_tab.alloc(tab_need));
    JTK_HIP_TRY(d_f.alloc(f_need));
    JTK_HIP_TRY(d_ring.alloc(ring_need));
    JTK_HIP_TRY(d_gain.alloc(gain_n));
    JTK_HIP_TRY(d_dead.alloc(gain_n));
    JTK_HIP_TRY(d_edits.alloc(edit_n));
    JTK_HIP_TRY(d_cells.alloc(2));
    JTK_HIP_TRY(d_cells.zero(2, st));
    uint64_t dbg_n = 0;
    if (table_out) {
        dbg_n = (uint64_t)n_reads * (piles[0].tmpl_cap + 1) * GP_ROWS;
        JTK_HIP_TRY(d_dbg.alloc(dbg_n));
        JTK_HIP_TRY(hipMemsetAsync(d_dbg.get(), 0xff, std::max<uint64_t>(dbg_n, 1) * sizeof(uint32_t), st));
    }
    for (size_t c = 0; c < n_chunks; c++)
        if (state[c].status == 0 && chunks[c].tmpl_len)
            JTK_HIP_TRY(hipMemcpyAsync(d_t0.get() + piles[c].tmpl_off, tmpl_bases + chunks[c].tmpl_off, chunks[c].tmpl_len, hipMemcpyHostToDevice, st));
    if (y_bytes) JTK_HIP_TRY(hipMemcpyAsync(d_y.get(), read_bases, y_bytes, hipMemcpyHostToDevice, st));
    {
        // the input ops of every read into the first half of its share: gathered on the host, one copy
        std::vector<uint8_t> init(ops_bytes, 0);
        for (uint64_t r = 0; r < n_reads; r++)
            if (rstate[r].len) std::memcpy(init.data() + reads[r].ops_off, ops + ops_off[r], rstate[r].len);
        if (ops_bytes) JTK_HIP_TRY(hipMemcpyAsync(d_ops.get(), init.data(), ops_bytes, hipMemcpyHostToDevice, st));
        JTK_HIP_TRY(hipStreamSynchronize(st));  // `init` goes with this scope
    }
    GpArgs a{};
    a.piles = d_piles.cget();
    a.state = d_state.get();
    a.reads = d_reads.cget();
    a.rstate = d_rstate.get();
    a.tmpl[0] = d_t0.get();
    a.tmpl[1] = d_t1.get();
    a.y = d_y.cget();
    a.ops = d_ops.get();
    a.tab = d_tab.get();
    a.f = d_f.get();
    a.ring = d_ring.get();
    a.gain = d_gain.get();
    a.dead = d_dead.get();
    a.edits = d_edits.get();
    a.dbg_table = d_dbg.get();
    a.cells = d_cells.get();
    a.take_num = take_num;
    a.ignore_edge = ignore_edge;
    const size_t fill_lds = GP_WAVES * 4 * GP_LDS_WIDTH * sizeof(uint16_t);
    auto fill = [&](int final_pass) -> int {
        a.final_pass = final_pass;
        for (size_t sl = 0; sl + 1 < slice_first.size(); sl++) {
            a.first = slice_first[sl];
            a.count = slice_first[sl + 1] - slice_first[sl];
            if (!a.count) continue;
            gp_fill_kernel<<<(a.count + GP_WAVES - 1) / GP_WAVES, GP_WAVES * 64, fill_lds, st>>>(a);
            JTK_HIP_TRY(hipGetLastError());
        }
        return 0;
    };
    double kernel_ms = 0;
    uint32_t rounds_run = 0;
    const uint32_t nc = (uint32_t)n_chunks, nr = (uint32_t)n_reads;
    for (uint32_t t = 0; t < limit && nc; t++) {
        JTK_HIP_TRY(hipEventRecord(s.ev[0], st));
        gp_begin_kernel<<<nc, 256, 0, st>>>(a.piles, a.state, a.gain, a.dead, ignore_edge, table_out ? 0 : 1);
        JTK_HIP_TRY(hipGetLastError());
        if (int rc = fill(0)) return rc;
        if (!table_out) {
            gp_select_kernel<<<nc, 64, max_cap + 64, st>>>(a.piles, a.state, a.tmpl[0], a.tmpl[1], a.gain, a.dead, a.edits, ignore_edge);
            JTK_HIP_TRY(hipGetLastError());
            if (nr) {
                gp_rethread_kernel<<<(nr + GP_WAVES - 1) / GP_WAVES, GP_WAVES * 64, 0, st>>>(nr, a.piles, a.state, a.reads, a.rstate, a.tmpl[0], a.tmpl[1],
                                                                                            a.y, a.ops, a.edits);
                JTK_HIP_TRY(hipGetLastError());
            }
            gp_commit_kernel<<<1, 256, 0, st>>>(nc, a.state, h_count_dev);
            JTK_HIP_TRY(hipGetLastError());
        }
        JTK_HIP_TRY(hipEventRecord(s.ev[1], st));
        JTK_HIP_TRY(hipStreamSynchronize(st));
        JTK_HIP_TRY(hipGetLastError());
        float ms = 0.f;
        JTK_HIP_TRY(s.elapsed(0, 1, &ms));
        kernel_ms += ms;
        rounds_run++;
        if (table_out || __atomic_load_n(&count.h[0], __ATOMIC_RELAXED) == 0) break;
    }
    if (!table_out && nc) {  // ops and distances of the pile-ups that stopped on a template no fill has seen
        JTK_HIP_TRY(hipEventRecord(s.ev[0], st));
        if (int rc = fill(1)) return rc;
        JTK_HIP_TRY(hipEventRecord(s.ev[1], st));
        JTK_HIP_TRY(hipStreamSynchronize(st));
        JTK_HIP_TRY(hipGetLastError());
        float ms = 0.f;
        JTK_HIP_TRY(s.elapsed(0, 1, &ms));
        kernel_ms += ms;
    }
    if (nc) JTK_HIP_TRY(d_state.download(state.data(), n_chunks, st));
    if (nr) JTK_HIP_TRY(d_rstate.download(rstate.data(), n_reads, st));
    unsigned long long cells[2] = {0, 0};
    JTK_HIP_TRY(d_cells.download(cells, 2, st));
    JTK_HIP_TRY(hipStreamSynchronize(st));
    g_gpolish_timing[0] = (double)n_chunks;
    g_gpolish_timing[1] = (double)n_reads;
    g_gpolish_timing[2] = rounds_run;
    g_gpolish_timing[3] = (double)cells[0];
    g_gpolish_timing[4] = kernel_ms;
    g_gpolish_timing[5] = (double)(slice_first.size() - 1);
    g_gpolish_timing[6] = (double)work_bytes;
    g_gpolish_timing[7] = (double)cells[1];
    int rc = 0;
    for (size_t c = 0; c < n_chunks; c++) {
        if (state[c].status == JTK_ERR_INTERNAL) return jtk_fail(JTK_ERR_INTERNAL, "guided polish: a walk left the band or a share of the work area was too small");
        if (state[c].status) rc = JTK_ERR_CHUNK_FAILED;
    }
    if (table_out) {
        if (rc) return jtk_fail(JTK_ERR_UNSUPPORTED, "the pile-up is beyond the limits of the guided polish");
        for (uint64_t r = 0; r < n_reads; r++) dist_out[r] = rstate[r].dist;
        if (dbg_n) JTK_HIP_TRY(hipMemcpy(table_out, d_dbg.cget(), dbg_n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        return 0;
    }
    std::vector<uint64_t> ops_dst(n_reads + 1, 0), cons_dst(n_chunks + 1, 0);
    for (size_t c = 0; c < n_chunks; c++) {
        const bool ok = state[c].status == 0;
        cons_dst[c + 1] = cons_dst[c] + (ok ? state[c].n : 0);
        for (uint64_t r = chunks[c].read_first; r < chunks[c].read_first + chunks[c].n_reads; r++) {
            ops_dst[r + 1] = ops_dst[r] + (ok ? rstate[r].len : 0);
            dist_out[r] = ok ? rstate[r].dist : GP_DEAD;
        }
        std::memset(&result[c], 0, sizeof result[c]);
        result[c].status = state[c].status;
        result[c].polish_rounds = state[c].rounds;
    }
    const uint64_t ops_total = ops_dst[n_reads], cons_total = cons_dst[n_chunks];
    if (cons_total > cons_cap) return jtk_fail(JTK_ERR_INVALID_ARG, "cons_cap is smaller than the consensus sequences of the batch");
    if (ops_total > ops_cap) return jtk_fail(JTK_ERR_INVALID_ARG, "ops_cap is smaller than the ops of the batch");
    if (ops_total + cons_total) {
        DevArr<uint64_t> d_od, d_cd;
        DevArr<uint8_t> d_oo, d_co;
        int rc2;
        if ((rc2 = d_od.upload(ops_dst, st)) || (rc2 = d_cd.upload(cons_dst, st))) return jtk_fail(rc2, "device upload failed");
        JTK_HIP_TRY(d_oo.alloc(ops_total));
        JTK_HIP_TRY(d_co.alloc(cons_total));
        gp_pack_kernel<<<nr + nc, 256, 0, st>>>(nr, nc, a.piles, a.state, a.reads, a.rstate, a.tmpl[0], a.tmpl[1], a.ops, d_od.cget(), d_cd.cget(),
                                                d_oo.get(), d_co.get());
        JTK_HIP_TRY(hipGetLastError());
        if (ops_total) JTK_HIP_TRY(d_oo.download(ops_out, ops_total, st));
        if (cons_total) JTK_HIP_TRY(d_co.download(cons_out, cons_total, st));
        JTK_HIP_TRY(hipStreamSynchronize(st));
        JTK_HIP_TRY(hipGetLastError());
    }
    std::copy(ops_dst.begin(), ops_dst.end(), ops_out_off);
    std::copy(cons_dst.begin(), cons_dst.end(), cons_off);
    if (rc) return jtk_fail(rc, "a pile-up is beyond 32,000 bases per sequence or JTK_GUIDED_MAX_WIDTH cells per band row, or outgrew its buffers");
    return 0;
}

// Everything the call reads of its inputs, before a device is looked for.
int gp_validate(size_t n_chunks, const jtk_lc_chunk_t *chunks, const uint8_t *tmpl_bases, const uint8_t *read_bases, const uint64_t *read_off,
                const uint8_t *ops, const uint64_t *ops_off, const uint32_t *radius, bool radius_zero_ok) {
    if (n_chunks && (!chunks || !radius)) return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    uint64_t n_reads = 0;
    if (int rc = check_contiguous(chunks, n_chunks, &n_reads)) return rc;
    if (n_reads && (!read_off || !ops_off)) return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    for (size_t c = 0; c < n_chunks; c++) {
        if (!radius_zero_ok && radius[c] == 0) return jtk_fail(JTK_ERR_INVALID_ARG, "a radius of 0");
        if (chunks[c].tmpl_len && !tmpl_bases) return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
        for (uint64_t q = 0; q < chunks[c].tmpl_len; q++) {
            const uint8_t v = tmpl_bases[chunks[c].tmpl_off + q];
            if (v != 'A' && v != 'C' && v != 'G' && v != 'T') return jtk_fail(JTK_ERR_INVALID_ARG, "non-ACGT base");
        }
    }
    for (uint64_t r = 0; r < n_reads; r++) {
        if (read_off[r + 1] < read_off[r] || ops_off[r + 1] < ops_off[r]) return jtk_fail(JTK_ERR_INVALID_ARG, "offsets must not decrease");
        if (ops_off[r + 1] - ops_off[r] > 2ull * GP_MAX_LEN + 128) return jtk_fail(JTK_ERR_INVALID_ARG, "more ops than two sequences of 32,000 bases take");
    }
    if (n_reads) {
        if ((read_off[n_reads] > read_off[0] && !read_bases) || (ops_off[n_reads] > ops_off[0] && !ops)) return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
        for (uint64_t q = read_off[0]; q < read_off[n_reads]; q++) {
            const uint8_t v = read_bases[q];
            if (v != 'A' && v != 'C' && v != 'G' && v != 'T') return jtk_fail(JTK_ERR_INVALID_ARG, "non-ACGT base");
        }
        for (uint64_t q = ops_off[0]; q < ops_off[n_reads]; q++)
            if (ops[q] > 3) return jtk_fail(JTK_ERR_INVALID_ARG, "op code above 3");
    }
    return 0;
}

}  // namespace

extern "C" void jtk_lc_debug_gpolish_timing(double *out) {
    if (out) std::memcpy(out, g_gpolish_timing, sizeof(g_gpolish_timing));
}

extern "C" int jtk_lc_polish_guided(size_t n_chunks, const jtk_lc_chunk_t *chunks, const uint8_t *tmpl_bases, const uint8_t *read_bases,
                                    const uint64_t *read_off, const uint8_t *ops, const uint64_t *ops_off, const uint32_t *radius, uint32_t take_num,
                                    uint32_t ignore_edge, uint32_t max_rounds, uint8_t *cons_out, uint64_t *cons_off, uint64_t cons_cap, uint8_t *ops_out,
                                    uint64_t *ops_out_off, uint64_t ops_cap, uint32_t *dist_out, jtk_lc_result_t *result, int device) {
    g_last_error.clear();
    if (!cons_off || !ops_out_off) return jtk_fail(JTK_ERR_INVALID_ARG, "null output");
    if (n_chunks && (!result || !cons_out || !ops_out)) return jtk_fail(JTK_ERR_INVALID_ARG, "null output");
    if (int rc = gp_validate(n_chunks, chunks, tmpl_bases, read_bases, read_off, ops, ops_off, radius, false)) return rc;
    if (n_chunks && chunks[n_chunks - 1].read_first + chunks[n_chunks - 1].n_reads && !dist_out) return jtk_fail(JTK_ERR_INVALID_ARG, "null output");
    if (int rc = jtk_require_device(device)) return rc;
    cons_off[0] = 0;
    ops_out_off[0] = 0;
    if (!n_chunks) return 0;
    return gp_run(n_chunks, chunks, tmpl_bases, read_bases, read_off, ops, ops_off, radius, take_num, ignore_edge, max_rounds, cons_out, cons_off, cons_cap,
                  ops_out, ops_out_off, ops_cap, dist_out, result, nullptr);
}

extern "C" int jtk_lc_debug_guided_table(const uint8_t *tmpl, uint32_t tmpl_len, uint32_t n_reads, const uint8_t *read_bases, const uint64_t *read_off,
                                         const uint8_t *ops, const uint64_t *ops_off, uint32_t radius, uint32_t *dist_out, uint32_t *table_out,
                                         uint64_t table_stride, int device) {
    g_last_error.clear();
    if (!n_reads || !dist_out || !table_out) return jtk_fail(JTK_ERR_INVALID_ARG, "null argument or no read");
    jtk_lc_chunk_t ch;
    std::memset(&ch, 0, sizeof ch);
    ch.n_reads = n_reads;
    ch.tmpl_len = tmpl_len;
    if (int rc = gp_validate(1, &ch, tmpl, read_bases, read_off, ops, ops_off, &radius, true)) return rc;
    if (int rc = jtk_require_device(device)) return rc;
    const uint32_t cap = std::min<uint32_t>(GP_MAX_LEN, tmpl_len + 64 + tmpl_len / 8);  // the stride of the device's table
    if (tmpl_len > GP_MAX_LEN) return jtk_fail(JTK_ERR_UNSUPPORTED, "the template is longer than 32,000 bases");
    if (table_stride < ((uint64_t)tmpl_len + 1) * GP_ROWS) return jtk_fail(JTK_ERR_INVALID_ARG, "table_stride is smaller than (tmpl_len + 1) x 14");
    std::vector<uint32_t> wide((uint64_t)n_reads * (cap + 1) * GP_ROWS);
    if (int rc = gp_run(1, &ch, tmpl, read_bases, read_off, ops, ops_off, &radius, 0, 0, 1, nullptr, nullptr, 0, nullptr, nullptr, 0, dist_out, nullptr,
                        wide.data()))
        return rc;
    for (uint32_t r = 0; r < n_reads; r++)
        std::memcpy(table_out + r * table_stride, wide.data() + (uint64_t)r * (cap + 1) * GP_ROWS, ((uint64_t)tmpl_len + 1) * GP_ROWS * sizeof(uint32_t));
    return 0;
}
