// guided.hip -- jtk_lc_align_guided: banded three-state affine-gap alignment along a guide path, global or infix; what the
// reference gets from kiley::bialignment::guided (encode/deletion_fill.rs:526,553-554, dense_encoding.rs:757,
// determine_chunks.rs:538, consensus/mod.rs:560,1231-1233,1259-1261).  Specification: DESIGN.md section 4, "Guided alignment";
// it is this build's own, parity with kiley's band and tie-breaking is not pinned.
//
// One wave per pair, in three launches per slice of the batch:
//   1. guided_rows_kernel: the walk over the guide (64 ops per coalesced load, then lane-uniform steps on registers) leaves the
//      path's first and last column of every row; a scan over the rows turns them into the band's first column and the row's
//      offset into the traceback area (the prefix sum of the widths), and gives the widest row.
//   2. guided_fill_kernel: rows in order, lanes over the columns of a row, 64 at a time.  M and D need the row above only; I
//      along the row is a prefix maximum with linear decay, I(i, j) = j ext + max_{k < j} (max(M, D)(i, k) + open - (k + 1) ext)
//      (six __shfl_up steps and a carry between the 64-column pieces).  Two rows of three int32 states per wave: in LDS where
//      the widest row has at most GD_LDS_WIDTH cells, in a global work area of the few waves of a second launch otherwise.
//      One traceback byte per cell -- two bits per state: the first predecessor that reproduces it; bit 6: a mismatch --
//      written one byte per lane.  Then the walk back, every lane the same, 64 ops per store.
// Minus infinity is GD_NEG: every state is clamped to it from below, scores are bounded by JTK_GUIDED_MAX_SCORE and lengths by
// 32,000, so a finite value (>= -6.6e7) is never confused with one derived from GD_NEG (<= GD_NEG + 3.8e7).
// The traceback area is budgeted: a pair takes at most min((n + 1)(m + 1), n + m + 1 + 2 r (n + 1), (n + 1) MAX_WIDTH) cells
// (the path has at most n + m + 1 cells, each row gains at most 2 r), the host cuts the batch into slices that fit
// GD_WORK_BYTES by that bound and enqueues them behind each other on one stream -- the offsets inside a pair's share come
// from the device pass, and nothing waits for a pair.
#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#include "device_common.h"
#include "guided_internal.h"
#include "jtk_lc_debug.h"
#include "wave_util.h"

namespace {

constexpr int32_t GD_NEG = -0x40000000;
constexpr uint32_t GD_MAX_LEN = 32000;             // ALIGN_MAX_LEN of align_kernels.hip
constexpr uint32_t GD_MAX_WIDTH = JTK_GUIDED_MAX_WIDTH;
constexpr uint32_t GD_WAVES = 4;                   // waves per block of the LDS launch
constexpr uint32_t GD_LDS_WIDTH = 512;             // 2 rows x 3 states x 4 bytes x 512 cells = 12 KiB per wave, 48 KiB per block
constexpr uint32_t GD_LARGE_WAVES = 512;           // waves of the second launch: 96 KiB of rows each
constexpr uint64_t GD_WORK_BYTES = 4ull << 30;     // traceback bytes + row tables per slice
constexpr uint32_t GD_MIS = 64;                    // traceback bit: the M step is a mismatch

using GdWork = GuidedWork;

struct GdArgs {
    uint32_t first, count;  // the slice
    const jtk_guided_pair_t *pairs;
    const GdWork *work;
    const uint8_t *x, *y, *guide;
    uint32_t *tab;
    uint8_t *tb;
    int32_t *rows;          // LARGE only: 6 GD_MAX_WIDTH ints per wave
    uint32_t *maxw;         // per pair: the widest row; 0 = nothing to fill
    int32_t *score, *status;
    uint32_t *start, *end, *nops;
    uint8_t *slots;
    const uint64_t *slot_end;
    unsigned long long *cells;
    int32_t match, mismatch, gap_open, gap_ext;
    int infix;
};

__device__ __forceinline__ int32_t gd_max(int32_t a, int32_t b) { return a > b ? a : b; }

// The guide's path and the band of one pair: tab[i] = first column of row i, tab[n + 2 + i] = cells in the rows above it.
__global__ void __launch_bounds__(GD_WAVES * 64) guided_rows_kernel(GdArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = blockIdx.x * GD_WAVES + (threadIdx.x >> 6);
    if (w >= a.count) return;
    const uint32_t p = a.first + w;
    if (a.status[p] != 0) {
        if (lane == 0) a.maxw[p] = 0;
        return;
    }
    const jtk_guided_pair_t pr = a.pairs[p];
    const GdWork wk = a.work[p];
    const uint32_t n = pr.x_len, m = pr.y_len;
    uint32_t *lo = a.tab + wk.tab_off, *hi = lo + (n + 2);
    uint32_t carry = 0;
    const uint32_t widest = jtk_band_rows(n, m, pr.radius, a.guide + pr.guide_off, pr.guide_len, lo, hi, lane, &carry);
    if (lane == 0) {
        int32_t st = 0;
        if (widest > GD_MAX_WIDTH)
            st = JTK_ERR_UNSUPPORTED;
        else if (carry > wk.tb_cap)
            st = JTK_ERR_INTERNAL;  // the host's bound holds for every guide; never seen
        a.maxw[p] = st ? 0u : widest;
        if (st) {
            a.status[p] = st;
            a.score[p] = 0;
            a.start[p] = a.end[p] = a.nops[p] = 0;
        } else {
            atomicAdd(a.cells, (unsigned long long)carry);
        }
    }
}

// The fill and the walk back of one pair by one wave; rows = 6 * stride ints (LDS or global).
__device__ void gd_pair(const GdArgs &a, uint32_t p, uint32_t stride, int32_t *rows, uint32_t lane) {
    const jtk_guided_pair_t pr = a.pairs[p];
    const GdWork wk = a.work[p];
    const uint32_t n = pr.x_len, m = pr.y_len;
    const uint32_t *first_col = a.tab + wk.tab_off, *row_off = first_col + (n + 2);
    uint8_t *tb = a.tb + wk.tb_off;
    const uint8_t *x = a.x + pr.x_off, *y = a.y + pr.y_off;
    const int32_t s_open = a.gap_open, s_ext = a.gap_ext;
    int32_t best = INT_MIN;
    uint32_t best_row = 0, best_state = 0;
    uint32_t prev_first = 1, prev_width = 0;  // no row above row 0
    uint32_t cb = first_col[0], off = row_off[0], off_next = row_off[1];
    uint8_t xi = 0;
    for (uint32_t i = 0; i <= n; i++) {
        // the next row's constants are on their way while this one is filled
        uint32_t n_cb = 0, n_off_next = 0;
        uint8_t n_xi = 0;
        if (i < n) {
            n_cb = first_col[i + 1];
            n_off_next = row_off[i + 2];
            n_xi = x[i];
        }
        const uint32_t width = off_next - off;
        int32_t *cur = rows + (i & 1u) * 3 * stride;
        const int32_t *prev = rows + ((i & 1u) ^ 1u) * 3 * stride;
        int32_t run = GD_NEG, left_m = GD_NEG, left_d = GD_NEG;
        for (uint32_t base = 0; base < width; base += 64) {
            const uint32_t c = base + lane;
            const bool active = c < width;
            const uint32_t j = cb + c;
            int32_t vm = GD_NEG, vd = GD_NEG;
            uint32_t bits = 0;
            if (active) {
                if (i > 0) {
                    const uint32_t dc = j - 1 - prev_first;  // wraps below the band of the row above
                    if (j >= 1 && j - 1 >= prev_first && dc < prev_width) {
                        const int32_t pm = prev[dc], pd = prev[stride + dc], pi = prev[2 * stride + dc];
                        const int32_t mx = gd_max(pm, gd_max(pd, pi));
                        bits = pm == mx ? 0u : (pd == mx ? 1u : 2u);
                        const bool same = xi == y[j - 1];
                        vm = mx + (same ? a.match : a.mismatch);
                        if (!same) bits |= GD_MIS;
                    }
                    const uint32_t uc = j - prev_first;
                    if (j >= prev_first && uc < prev_width) {
                        const int32_t c0 = prev[uc] + s_open, c1 = prev[stride + uc] + s_ext, c2 = prev[2 * stride + uc] + s_open;
                        vd = gd_max(c0, gd_max(c1, c2));
                        bits |= (c0 == vd ? 0u : (c1 == vd ? 1u : 2u)) << 2;
                    }
                }
                if (j == 0 && (i == 0 || a.infix)) vm = 0;
                vm = gd_max(vm, GD_NEG);
                vd = gd_max(vd, GD_NEG);
            }
            // I: the best gap that ends here, opened behind column k < j of this row
            int32_t incl = active ? gd_max(vm, vd) + s_open - (int32_t)(c + 1) * s_ext : GD_NEG;
            for (uint32_t o = 1; o < 64; o <<= 1) {
                const int32_t u = __shfl_up(incl, o, 64);
                if (lane >= o) incl = gd_max(incl, u);
            }
            int32_t excl = __shfl_up(incl, 1, 64);
            int32_t lm = __shfl_up(vm, 1, 64), ld = __shfl_up(vd, 1, 64);
            if (lane == 0) {
                excl = GD_NEG;
                lm = left_m;
                ld = left_d;
            }
            const int32_t vi = gd_max(GD_NEG, (int32_t)c * s_ext + gd_max(run, excl));
            bits |= (lm + s_open == vi ? 0u : (ld + s_open == vi ? 1u : 2u)) << 4;
            run = gd_max(run, __shfl(incl, 63, 64));
            left_m = __shfl(vm, 63, 64);
            left_d = __shfl(vd, 63, 64);
            if (active) {
                cur[c] = vm;
                cur[stride + c] = vd;
                cur[2 * stride + c] = vi;
                tb[(uint64_t)off + c] = (uint8_t)bits;
            }
        }
        jtk_wave_sync();
        if (cb + width - 1 == m && (a.infix || i == n)) {  // an end cell; the first row that holds the maximum keeps it
            const int32_t e0 = cur[width - 1], e1 = cur[stride + width - 1], e2 = cur[2 * stride + width - 1];
            const int32_t ev = gd_max(e0, gd_max(e1, e2));
            if (ev > best) {
                best = ev;
                best_row = i;
                best_state = e0 == ev ? 0u : (e1 == ev ? 1u : 2u);
            }
        }
        prev_first = cb;
        prev_width = width;
        cb = n_cb;
        off = off_next;
        off_next = n_off_next;
        xi = n_xi;
    }
    // ---- the walk back, every lane the same; op k from the end goes to slot_end - 1 - k, 64 of them per store
    uint8_t *slot_last = a.slots + a.slot_end[p] - 1;
    const uint32_t k0 = n - best_row;  // the free run behind the end
    for (uint32_t t = lane; t < k0; t += 64) *(slot_last - t) = JTK_OP_DEL;
    uint32_t k = k0, i = best_row, j = m, state = best_state;
    uint32_t held = 0;
    uint32_t row_first = first_col[i], row_at = row_off[i];
    bool lost = false;
    const uint32_t max_steps = n + m + 1;
    for (uint32_t steps = 0;; steps++) {
        if (state == 0 && j == 0 && (a.infix || i == 0)) break;
        if (steps > max_steps || (state != 2 && i == 0) || (state != 1 && j == 0) || j < row_first) {
            lost = true;
            break;
        }
        const uint32_t b = tb[(uint64_t)row_at + (j - row_first)];
        uint32_t op;
        if (state == 0) {
            op = b & GD_MIS ? JTK_OP_MISMATCH : JTK_OP_MATCH;
            state = b & 3u;
            i--;
            j--;
        } else if (state == 1) {
            op = JTK_OP_DEL;
            state = (b >> 2) & 3u;
            i--;
        } else {
            op = JTK_OP_INS;
            state = (b >> 4) & 3u;
            j--;
        }
        if (op != JTK_OP_INS) {
            row_first = first_col[i];
            row_at = row_off[i];
        }
        if (lane == (k & 63u)) held = op;
        k++;
        if ((k & 63u) == 0) {
            const uint32_t at = k - 64 + lane;
            if (at >= k0) *(slot_last - at) = (uint8_t)held;
        }
    }
    if (k & 63u) {
        const uint32_t at = (k & ~63u) + lane;
        if (lane < (k & 63u) && at >= k0) *(slot_last - at) = (uint8_t)held;
    }
    const uint32_t start = a.infix ? i : 0;
    for (uint32_t t = lane; t < start; t += 64) *(slot_last - (k + t)) = JTK_OP_DEL;
    k += start;
    if (lane == 0) {
        a.status[p] = lost ? JTK_ERR_INTERNAL : 0;
        a.score[p] = best;
        a.start[p] = start;
        a.end[p] = best_row;
        a.nops[p] = lost ? 0u : k;
    }
    jtk_wave_sync();  // the rows are the next pair's
}

// LARGE == false: the pairs whose widest row fits the wave's LDS; true: the others, rows in the global area of a few waves.
template <bool LARGE>
__global__ void __launch_bounds__(GD_WAVES * 64) guided_fill_kernel(GdArgs a) {
    extern __shared__ __attribute__((aligned(16))) int32_t gd_lds[];
    const uint32_t lane = threadIdx.x & 63u, wave_in_block = threadIdx.x >> 6;
    const uint32_t wave = blockIdx.x * (blockDim.x >> 6) + wave_in_block, n_waves = gridDim.x * (blockDim.x >> 6);
    int32_t *rows = LARGE ? a.rows + (uint64_t)wave * 6 * GD_MAX_WIDTH : gd_lds + wave_in_block * 6 * GD_LDS_WIDTH;
    for (uint32_t w = wave; w < a.count; w += n_waves) {
        const uint32_t p = a.first + w;
        const uint32_t widest = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.maxw[p]);
        if (widest == 0 || widest > GD_MAX_WIDTH || (widest > GD_LDS_WIDTH) != LARGE) continue;
        gd_pair(a, p, LARGE ? GD_MAX_WIDTH : GD_LDS_WIDTH, rows, lane);
    }
}

__global__ void __launch_bounds__(256) guided_pack_kernel(uint32_t n, const uint8_t *slots, const uint64_t *slot_end, const uint32_t *nops,
                                                          const uint64_t *dst_off, uint8_t *out) {
    const uint32_t p = blockIdx.x;
    if (p >= n) return;
    const uint32_t len = (uint32_t)(dst_off[p + 1] - dst_off[p]);
    if (len == 0 || len != nops[p]) return;  // a failed pair has an empty share
    const uint8_t *src = slots + slot_end[p] - len;
    uint8_t *dst = out + dst_off[p];
    for (uint32_t q = threadIdx.x; q < len; q += blockDim.x) dst[q] = src[q];
}

thread_local uint64_t g_guided_cap = 0;    // jtk_lc_debug_guided_scratch_cap
thread_local double g_guided_timing[4];    // pairs, cells, kernel ms, slices

uint64_t gd_cells_bound(uint32_t n, uint32_t m, uint32_t r) {
    const uint64_t rows = (uint64_t)n + 1, longest = std::max(n, m);
    const uint64_t rr = std::min<uint64_t>(r, longest + 1);
    const uint64_t by_path = (uint64_t)n + m + 1 + 2 * rr * rows;
    return std::min({rows * ((uint64_t)m + 1), by_path, rows * GD_MAX_WIDTH});
}

}  // namespace

uint64_t guided_scratch_cap() { return g_guided_cap ? g_guided_cap : GD_WORK_BYTES; }

int guided_plan(const GuidedBatch &b, GuidedRun &run) {
    run.work.assign(b.n, GuidedWork{});
    run.slice_first.clear();
    run.tab_need = run.tb_need = 0;
    run.any_large = false;
    run.slices = 0;
    if (!b.n) return 0;
    if (b.n >= 0x7fffffffu) return jtk_fail(JTK_ERR_UNSUPPORTED, "2^31 - 1 pairs or more");
    // shares of the work area; a slice ends where the next pair would pass the budget (a pair alone always runs)
    const uint64_t cap = guided_scratch_cap();
    uint64_t tab_used = 0, tb_used = 0;
    for (size_t p = 0; p < b.n; p++) {
        const uint32_t n = b.h_xlen[p], m = b.h_ylen[p];
        const bool skip = n > GD_MAX_LEN || m > GD_MAX_LEN;  // its status is set; the kernels leave it alone
        const uint64_t cells = skip ? 0 : (gd_cells_bound(n, m, b.h_radius[p]) + 15) & ~15ull;
        const uint64_t tab = skip ? 0 : 2 * ((uint64_t)n + 2);
        if (p == 0 || tb_used + cells + 4 * (tab_used + tab) > cap) {
            run.slice_first.push_back((uint32_t)p);
            tab_used = tb_used = 0;
        }
        run.work[p].tab_off = tab_used;
        run.work[p].tb_off = tb_used;
        run.work[p].tb_cap = cells;
        tab_used += tab;
        tb_used += cells;
        run.tab_need = std::max(run.tab_need, tab_used);
        run.tb_need = std::max(run.tb_need, tb_used);
        if (!skip && m + 1 > GD_LDS_WIDTH) run.any_large = true;  // a row may be as wide as the guide makes it
    }
    run.slice_first.push_back((uint32_t)b.n);
    return 0;
}

int guided_reserve(GuidedArea &area, const GuidedRun &run) {
    if (run.tab_need > area.tab_have || !area.tab.get()) {
        area.tab_have = 0;
        JTK_HIP_TRY(area.tab.alloc(run.tab_need));
        area.tab_have = run.tab_need;
    }
    if (run.tb_need > area.tb_have || !area.tb.get()) {
        area.tb_have = 0;
        JTK_HIP_TRY(area.tb.alloc(run.tb_need));
        area.tb_have = run.tb_need;
    }
    if (run.any_large && !area.rows_have) {
        JTK_HIP_TRY(area.rows.alloc((uint64_t)GD_LARGE_WAVES * 6 * GD_MAX_WIDTH));
        area.rows_have = true;
    }
    return 0;
}

int guided_enqueue(const GuidedBatch &b, GuidedRun &run, GuidedArea &area, hipStream_t st) {
    run.slices = 0;
    if (!b.n) return 0;
    if (run.work.size() != b.n || run.tab_need > area.tab_have || run.tb_need > area.tb_have || (run.any_large && !area.rows_have))
        return jtk_fail(JTK_ERR_INTERNAL, "guided: the batch was not planned or its work area not reserved");
    // run.work stays with the caller until the stream has been synchronised: the copy below reads it when the stream gets there
    if (int rc = run.d_work.upload(run.work, st)) return jtk_fail(rc, "device upload failed");
    JTK_HIP_TRY(run.maxw.alloc(b.n));
    JTK_HIP_TRY(run.cells.alloc(1));
    JTK_HIP_TRY(run.cells.zero(1, st));
    JTK_HIP_TRY(run.ev.create(2));
    GdArgs a{};
    a.pairs = b.d_pairs;
    a.work = run.d_work.cget();
    a.x = b.d_x;
    a.y = b.d_y;
    a.guide = b.d_guide;
    a.tab = area.tab.get();
    a.tb = area.tb.get();
    a.rows = area.rows.get();
    a.maxw = run.maxw.get();
    a.score = b.d_score;
    a.status = b.d_status;
    a.start = b.d_start;
    a.end = b.d_end;
    a.nops = b.d_nops;
    a.slots = b.d_slots;
    a.slot_end = b.d_slot_end;
    a.cells = run.cells.get();
    a.match = b.match;
    a.mismatch = b.mismatch;
    a.gap_open = b.gap_open;
    a.gap_ext = b.gap_ext;
    a.infix = b.infix;
    JTK_HIP_TRY(hipEventRecord(run.ev[0], st));
    for (size_t s = 0; s + 1 < run.slice_first.size(); s++) {
        a.first = run.slice_first[s];
        a.count = run.slice_first[s + 1] - run.slice_first[s];
        const uint32_t blocks = (a.count + GD_WAVES - 1) / GD_WAVES;
        guided_rows_kernel<<<blocks, GD_WAVES * 64, 0, st>>>(a);
        JTK_HIP_TRY(hipGetLastError());
        guided_fill_kernel<false><<<blocks, GD_WAVES * 64, GD_WAVES * 6 * GD_LDS_WIDTH * sizeof(int32_t), st>>>(a);
        JTK_HIP_TRY(hipGetLastError());
        if (run.any_large) {
            guided_fill_kernel<true><<<std::min<uint32_t>(a.count, GD_LARGE_WAVES), 64, 0, st>>>(a);
            JTK_HIP_TRY(hipGetLastError());
        }
        run.slices++;
    }
    JTK_HIP_TRY(hipEventRecord(run.ev[1], st));
    return 0;
}

int guided_elapsed(const GuidedRun &keep, double *ms, double *cells) {
    *ms = *cells = 0;
    if (!keep.slices) return 0;
    float f = 0.f;
    JTK_HIP_TRY(keep.ev.elapsed(0, 1, &f));
    unsigned long long c = 0;
    JTK_HIP_TRY(hipMemcpy(&c, keep.cells.cget(), sizeof(c), hipMemcpyDeviceToHost));
    *ms = f;
    *cells = (double)c;
    return 0;
}

int guided_pack(size_t n, const uint8_t *d_slots, const uint64_t *d_slot_end, const uint32_t *d_nops, const uint64_t *d_dst_off,
                uint8_t *d_out, hipStream_t st) {
    if (!n) return 0;
    guided_pack_kernel<<<(uint32_t)n, 256, 0, st>>>((uint32_t)n, d_slots, d_slot_end, d_nops, d_dst_off, d_out);
    JTK_HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" void jtk_lc_debug_guided_scratch_cap(uint64_t bytes) { g_guided_cap = bytes; }

extern "C" void jtk_lc_debug_guided_timing(double *out) {
    if (out) std::memcpy(out, g_guided_timing, sizeof(g_guided_timing));
}

extern "C" int jtk_lc_align_guided(size_t n_pairs, const jtk_guided_pair_t *pairs, const uint8_t *x_bases, const uint8_t *y_bases,
                                   const uint8_t *guide_ops, int mode, int match, int mismatch, int gap_open, int gap_ext,
                                   uint8_t *ops_out, uint64_t *ops_out_off, uint64_t ops_cap, int32_t *score_out, uint32_t *start_out,
                                   uint32_t *end_out, int32_t *status, int device) {
    g_last_error.clear();
    if (mode != JTK_ALIGN_GLOBAL && mode != JTK_ALIGN_INFIX) return jtk_fail(JTK_ERR_INVALID_ARG, "the mode is global or infix");
    if (!(gap_open <= gap_ext && gap_ext <= 0 && mismatch <= 0 && 0 <= match))
        return jtk_fail(JTK_ERR_INVALID_ARG, "scores need gap_open <= gap_ext <= 0 and mismatch <= 0 <= match");
    if (match > JTK_GUIDED_MAX_SCORE || mismatch < -JTK_GUIDED_MAX_SCORE || gap_open < -JTK_GUIDED_MAX_SCORE)
        return jtk_fail(JTK_ERR_INVALID_ARG, "a score above JTK_GUIDED_MAX_SCORE in magnitude");
    if (!ops_out_off || (n_pairs && (!pairs || !score_out || !start_out || !end_out || !status))) return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    if (n_pairs >= 0x7fffffffu) return jtk_fail(JTK_ERR_UNSUPPORTED, "2^31 - 1 pairs or more");
    // ---- validation; what the pairs reach of the three buffers
    uint64_t x_bytes = 0, y_bytes = 0, g_bytes = 0;
    for (size_t p = 0; p < n_pairs; p++) {
        const jtk_guided_pair_t &pr = pairs[p];
        if ((pr.x_len && !x_bases) || (pr.y_len && !y_bases) || (pr.guide_len && !guide_ops)) return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
        x_bytes = std::max(x_bytes, pr.x_off + pr.x_len);
        y_bytes = std::max(y_bytes, pr.y_off + pr.y_len);
        g_bytes = std::max(g_bytes, pr.guide_off + pr.guide_len);
    }
    {
        // every byte a pair reaches is looked at once, however many pairs share it
        auto scan = [&](const uint8_t *buf, uint64_t bytes, int which) {
            std::vector<uint8_t> want(bytes, 0);
            for (size_t p = 0; p < n_pairs; p++) {
                const jtk_guided_pair_t &pr = pairs[p];
                const uint64_t off = which == 0 ? pr.x_off : which == 1 ? pr.y_off : pr.guide_off;
                const uint32_t len = which == 0 ? pr.x_len : which == 1 ? pr.y_len : pr.guide_len;
                if (len) std::memset(want.data() + off, 1, len);
            }
            for (uint64_t q = 0; q < bytes; q++)
                if (want[q]) {
                    const uint8_t v = buf[q];
                    if (which == 2 ? v > 3 : (v != 'A' && v != 'C' && v != 'G' && v != 'T')) return false;
                }
            return true;
        };
        if (!scan(x_bases, x_bytes, 0) || !scan(y_bases, y_bytes, 1)) return jtk_fail(JTK_ERR_INVALID_ARG, "non-ACGT base");
        if (!scan(guide_ops, g_bytes, 2)) return jtk_fail(JTK_ERR_INVALID_ARG, "guide op code above 3");
    }
    if (int rc = jtk_require_device(device)) return rc;
    ops_out_off[0] = 0;
    if (!n_pairs) return 0;
    std::vector<uint32_t> xlen(n_pairs), ylen(n_pairs), radius(n_pairs);
    std::vector<int32_t> st_v(n_pairs, 0);
    std::vector<uint64_t> slot_end(n_pairs);
    uint64_t slot = 0;
    for (size_t p = 0; p < n_pairs; p++) {
        xlen[p] = pairs[p].x_len;
        ylen[p] = pairs[p].y_len;
        radius[p] = pairs[p].radius;
        if (xlen[p] > GD_MAX_LEN || ylen[p] > GD_MAX_LEN)
            st_v[p] = JTK_ERR_UNSUPPORTED;
        else
            slot += (uint64_t)xlen[p] + ylen[p];
        slot_end[p] = slot;
    }
    DevStream s;
    JTK_HIP_TRY(s.create());
    const hipStream_t st = s.st;
    DevArr<jtk_guided_pair_t> d_pairs;
    DevArr<uint8_t> d_x, d_y, d_g, d_slots;
    DevArr<int32_t> d_score, d_status;
    DevArr<uint32_t> d_start, d_end, d_nops;
    DevArr<uint64_t> d_slot_end;
    {
        const std::vector<jtk_guided_pair_t> pv(pairs, pairs + n_pairs);
        const std::vector<uint8_t> xv(x_bases, x_bases + x_bytes), yv(y_bases, y_bases + y_bytes), gv(guide_ops, guide_ops + g_bytes);
        int rc;
        if ((rc = d_pairs.upload(pv, st)) || (rc = d_x.upload(xv, st)) || (rc = d_y.upload(yv, st)) || (rc = d_g.upload(gv, st)) ||
            (rc = d_status.upload(st_v, st)) || (rc = d_slot_end.upload(slot_end, st)))
            return jtk_fail(rc, "device upload failed");
        JTK_HIP_TRY(hipStreamSynchronize(st));  // the vectors go with this scope
    }
    JTK_HIP_TRY(d_score.alloc(n_pairs));
    JTK_HIP_TRY(d_start.alloc(n_pairs));
    JTK_HIP_TRY(d_end.alloc(n_pairs));
    JTK_HIP_TRY(d_nops.alloc(n_pairs));
    JTK_HIP_TRY(d_slots.alloc(slot + 1));
    JTK_HIP_TRY(d_score.zero(n_pairs, st));
    JTK_HIP_TRY(d_start.zero(n_pairs, st));
    JTK_HIP_TRY(d_end.zero(n_pairs, st));
    JTK_HIP_TRY(d_nops.zero(n_pairs, st));
    GuidedBatch b;
    b.n = n_pairs;
    b.d_pairs = d_pairs.cget();
    b.d_x = d_x.cget();
    b.d_y = d_y.cget();
    b.d_guide = d_g.cget();
    b.infix = mode == JTK_ALIGN_INFIX;
    b.match = match;
    b.mismatch = mismatch;
    b.gap_open = gap_open;
    b.gap_ext = gap_ext;
    b.h_xlen = xlen.data();
    b.h_ylen = ylen.data();
    b.h_radius = radius.data();
    b.d_score = d_score.get();
    b.d_status = d_status.get();
    b.d_start = d_start.get();
    b.d_end = d_end.get();
    b.d_nops = d_nops.get();
    b.d_slots = d_slots.get();
    b.d_slot_end = d_slot_end.cget();
    GuidedRun run;
    GuidedArea area;
    if (int rc = guided_plan(b, run)) return rc;
    if (int rc = guided_reserve(area, run)) return rc;
    if (int rc = guided_enqueue(b, run, area, st)) return rc;
    std::vector<uint32_t> nops(n_pairs), start_v(n_pairs), end_v(n_pairs);
    std::vector<int32_t> score_v(n_pairs);
    JTK_HIP_TRY(d_nops.download(nops.data(), n_pairs, st));
    JTK_HIP_TRY(d_start.download(start_v.data(), n_pairs, st));
    JTK_HIP_TRY(d_end.download(end_v.data(), n_pairs, st));
    JTK_HIP_TRY(d_score.download(score_v.data(), n_pairs, st));
    JTK_HIP_TRY(d_status.download(st_v.data(), n_pairs, st));
    JTK_HIP_TRY(hipStreamSynchronize(st));
    JTK_HIP_TRY(hipGetLastError());
    {
        double ms = 0, cells = 0;
        if (int rc = guided_elapsed(run, &ms, &cells)) return rc;
        g_guided_timing[0] = (double)n_pairs;
        g_guided_timing[1] = cells;
        g_guided_timing[2] = ms;
        g_guided_timing[3] = run.slices;
    }
    int rc = 0;
    std::vector<uint64_t> dst_off(n_pairs + 1, 0);
    for (size_t p = 0; p < n_pairs; p++) {
        if (st_v[p] == JTK_ERR_INTERNAL) return jtk_fail(JTK_ERR_INTERNAL, "guided: the walk left the band");
        if (st_v[p]) {
            rc = JTK_ERR_CHUNK_FAILED;
            nops[p] = 0;
        }
        dst_off[p + 1] = dst_off[p] + nops[p];
    }
    const uint64_t total = dst_off[n_pairs];
    if (total > ops_cap || (total && !ops_out)) return jtk_fail(JTK_ERR_INVALID_ARG, "ops_cap is smaller than the ops of the batch");
    if (total) {
        DevArr<uint64_t> d_off;
        DevArr<uint8_t> d_out;
        if (int rc2 = d_off.upload(dst_off, st)) return jtk_fail(rc2, "device upload failed");
        JTK_HIP_TRY(d_out.alloc(total));
        if (int rc2 = guided_pack(n_pairs, d_slots.cget(), d_slot_end.cget(), d_nops.cget(), d_off.cget(), d_out.get(), st)) return rc2;
        JTK_HIP_TRY(d_out.download(ops_out, total, st));
        JTK_HIP_TRY(hipStreamSynchronize(st));
        JTK_HIP_TRY(hipGetLastError());
    }
    std::copy(dst_off.begin(), dst_off.end(), ops_out_off);
    std::copy(score_v.begin(), score_v.end(), score_out);
    std::copy(start_v.begin(), start_v.end(), start_out);
    std::copy(end_v.begin(), end_v.end(), end_out);
    std::copy(st_v.begin(), st_v.end(), status);
    if (rc) return jtk_fail(rc, "a pair is longer than 32,000 bases or its band has a row wider than JTK_GUIDED_MAX_WIDTH cells");
    return 0;
}
