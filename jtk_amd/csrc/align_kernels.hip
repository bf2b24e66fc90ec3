// align_kernels.hip -- jtk_lc_align_reads: batched global unit-cost alignment of reads to their templates (the reference's
// edlib Global / Alignment calls: consensus/mod.rs:424-435, polish_chunks.rs:114-120), and jtk_lc_align_reads_mode: the same
// with one sequence's ends free (edlib Infix / Prefix: encode/mod.rs:227-246, encode/deletion_fill.rs:544-554,
// dense_encoding.rs:728-757, determine_chunks.rs:520-538, consensus/mod.rs:563-614).  Specification: DESIGN.md section 4.
//
// One (template, read) pair per workgroup, restricted to the diagonals k = j - i of a band that is certain to hold every
// optimal path when the distance is <= t; the host doubles t for the pairs that come back above it.
//   fill: anti-diagonal d = i + j by anti-diagonal.  The last value of every diagonal lives in LDS, even and odd band slots
//         in separate arrays: a step on one parity reads its own array (the diagonal move, two anti-diagonals back) and the
//         other array (Del from slot + 1, Ins from slot - 1, one anti-diagonal back) and writes only its own, so one barrier
//         per anti-diagonal is enough.  A thread updates 8 consecutive cells of one parity (three 16-byte LDS reads, one
//         write) and produces their 2-bit move codes (16 bits); 8 anti-diagonals of them leave as one 16-byte store.
//   walk: wave 0 pulls an 8-block (64 anti-diagonal) x 11-group tile of move codes into LDS with two coalesced 16-byte loads
//         per lane, follows the path through the tile, and stores that stretch of ops, reversed, with one store per lane.
// Mode and free side are compile-time parameters of the one body: infix forces the free boundary to 0 in the fill; infix and
// prefix take the end cell as the minimum over the last row / column (the last value of the diagonals that close there, read
// from the LDS arrays; smallest index wins) and infix stops the walk at the free boundary.  The global instantiation
// compiles none of this (align_kernel<THREADS> is instruction for instruction what it was before the modes existed).
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "device_common.h"
#include "host_common.h"
#include "wave_util.h"

#define ALIGN_MAX_LEN 32000u  // tl + rl stays below the 16-bit infinity
#define ALIGN_INF 0xFFFFu
#define ALIGN_PAD 16          // bytes in front of and behind every sequence: a thread loads its 8 bases unaligned
#define ALIGN_WALK_LOST 0xFFFFFFFEu  // dist marker: the walk left the band (an internal error, reported as such)
#define ALIGN_TILE_GROUPS 11
#define ALIGN_TILE_BLOCKS 8
#define ALIGN_MODE_MAX_BAND JTK_ALIGN_MODE_MAX_BAND  // widest band an infix / prefix pair may need: 96 KB of LDS (jtk_lc.h)

namespace {

struct AlignPair {
    uint64_t tmpl_off, read_off;  // into the padded base buffer (first base)
    uint64_t scratch_off;         // into the move-code scratch, in 16-byte units
    uint64_t ops_off;             // slot of tl + rl bytes; the ops end at its end
    uint32_t tmpl_len, read_len;
    int32_t klo, khi;             // band: diagonals j - i in [klo, khi], clipped to the matrix
    uint32_t t;                   // distance the band certifies
    uint32_t out;                 // index into dist / n_ops
};

enum { MV_MATCH = 0, MV_MISMATCH = 1, MV_DEL = 2, MV_INS = 3 };
enum { AM_GLOBAL = JTK_ALIGN_GLOBAL, AM_INFIX = JTK_ALIGN_INFIX, AM_PREFIX = JTK_ALIGN_PREFIX };
enum { AF_TEMPLATE = JTK_ALIGN_FREE_TEMPLATE, AF_READ = JTK_ALIGN_FREE_READ };

__device__ __forceinline__ uint64_t load_u64_unaligned(const uint8_t *p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

// the walk goes on: infix stops at the first cell on the free boundary (j == 0 or i == 0; d + k = 2j, d - k = 2i), the
// other modes at (0, 0)
template <int MODE, int FREE>
__device__ __forceinline__ bool walk_on(int d, int k) {
    if constexpr (MODE == AM_INFIX) return (FREE == AF_TEMPLATE ? d + k : d - k) != 0;
    return d > 0;
}

// bounds[2 * out], [2 * out + 1] = start, end (MODE != AM_GLOBAL only; the global instantiation never looks at the pointer)
template <int THREADS, int MODE, int FREE>
__global__ __launch_bounds__(THREADS) void align_kernel(const AlignPair *pairs, const uint8_t *bases, uint4 *scratch,
                                                        uint8_t *ops_all, uint32_t *dist, uint32_t *n_ops, uint32_t *bounds) {
    extern __shared__ uint4 lds4[];
    __shared__ uint4 tile[ALIGN_TILE_BLOCKS * ALIGN_TILE_GROUPS];
    __shared__ uint8_t opbuf[64];
    const AlignPair pr = pairs[blockIdx.x];
    const int tl = (int)pr.tmpl_len, rl = (int)pr.read_len, klo = pr.klo, khi = pr.khi;
    const int W = khi - klo + 1;                // band slots; slot s is diagonal klo + s
    const int G = ((W + 1) / 2 + 7) / 8;        // groups of 8 same-parity cells
    const int stride = 8 * G + 16;              // 8 cells of infinity in front of and behind each parity array
    uint16_t *val = (uint16_t *)lds4;           // val[par * stride + 8 + cell]
    uint16_t *stage = val + 2 * stride;         // stage[dd * G + g]: codes of 8 anti-diagonals
    const uint8_t *x = bases + pr.tmpl_off, *y = bases + pr.read_off;
    const int tid = threadIdx.x;

    for (int a = tid; a < 2 * stride; a += THREADS) val[a] = ALIGN_INF;
    __syncthreads();
    if (tid == 0) val[((-klo) & 1) * stride + 8 + ((-klo) >> 1)] = 0;  // D(0,0)
    __syncthreads();

    const int dmax = tl + rl;
    for (int d = 1; d <= dmax; d++) {
        const int p = (d - klo) & 1;
        uint16_t *P = val + p * stride + 8;
        const uint16_t *Q = val + (p ^ 1) * stride + 8;
        for (int g = tid; g < G; g += THREADS) {
            const int k0 = klo + 2 * (8 * g) + p;     // diagonal of cell 0 of the group; d - k0 is even
            const int i0 = (d - k0) >> 1, j0 = (d + k0) >> 1;  // cell e is (i0 - e, j0 + e)
            int e_lo = i0 - tl > -j0 ? i0 - tl : -j0;
            if (e_lo < 0) e_lo = 0;
            int e_hi = i0 < rl - j0 ? i0 : rl - j0;
            const int e_band = (khi - k0) >> 1;       // arithmetic shift: negative when the group lies beyond the band
            if (e_band < e_hi) e_hi = e_band;
            if (e_hi > 7) e_hi = 7;
            uint32_t codes = 0;
            if (e_lo <= e_hi) {
                // x[i - 1] for cell e is byte 7 - e of xw, y[j - 1] is byte e of yw
                const uint64_t xw = load_u64_unaligned(x + i0 - 8), yw = load_u64_unaligned(y + j0 - 1);
                const uint64_t diff = __builtin_bswap64(xw) ^ yw;
                const uint4 pv = *(const uint4 *)(P + 8 * g), qv = *(const uint4 *)(Q + 8 * g);
                // Ins comes from slot - 1, Del from slot + 1: cells e - 1 + p and e + p of the other parity
                const uint32_t qx = p ? Q[8 * g + 8] : Q[8 * g - 1];
                const uint32_t pw[4] = {pv.x, pv.y, pv.z, pv.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
                uint32_t q9[9];
                if (p) {
#pragma unroll
                    for (int e = 0; e < 8; e++) q9[e] = (qw[e >> 1] >> (16 * (e & 1))) & 0xFFFFu;
                    q9[8] = qx;
                } else {
                    q9[0] = qx;
#pragma unroll
                    for (int e = 0; e < 8; e++) q9[e + 1] = (qw[e >> 1] >> (16 * (e & 1))) & 0xFFFFu;
                }
                uint32_t nw[4] = {pw[0], pw[1], pw[2], pw[3]};
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const uint32_t mm = ((diff >> (8 * e)) & 0xFFu) ? 1u : 0u;
                    const uint32_t a = ((pw[e >> 1] >> (16 * (e & 1))) & 0xFFFFu) + mm;
                    const uint32_t b = q9[e + 1] + 1u, c = q9[e] + 1u;  // Del, Ins
                    uint32_t m = a < b ? a : b;
                    m = m < c ? m : c;
                    m = m < ALIGN_INF ? m : ALIGN_INF;
                    const uint32_t code = a == m ? mm : (b == m ? (uint32_t)MV_DEL : (uint32_t)MV_INS);
                    if constexpr (MODE == AM_INFIX) {  // the free boundary; the walk stops there, so its code is never read
                        if ((FREE == AF_TEMPLATE ? j0 + e : i0 - e) == 0) m = 0;
                    }
                    if (e >= e_lo && e <= e_hi) {
                        codes |= code << (2 * e);
                        nw[e >> 1] = (nw[e >> 1] & ~(0xFFFFu << (16 * (e & 1)))) | (m << (16 * (e & 1)));
                    }
                }
                *(uint4 *)(P + 8 * g) = make_uint4(nw[0], nw[1], nw[2], nw[3]);
            }
            stage[(d & 7) * G + g] = (uint16_t)codes;
            if ((d & 7) == 7 || d == dmax) {  // the thread reads back what it wrote itself
                uint32_t w[4];
#pragma unroll
                for (int q = 0; q < 4; q++) w[q] = (uint32_t)stage[(2 * q) * G + g] | ((uint32_t)stage[(2 * q + 1) * G + g] << 16);
                scratch[pr.scratch_off + (uint64_t)(d >> 3) * G + g] = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
        __syncthreads();
    }

    int s_end = rl - tl - klo, d_end = dmax;
    uint32_t D, end = 0;
    if constexpr (MODE == AM_GLOBAL) {
        D = val[(s_end & 1) * stride + 8 + (s_end >> 1)];
    } else {
        // the diagonals that close in the last row (template free: cell (i, rl) closes k = rl - i) or the last column (read
        // free: (tl, j) closes k = j - tl) still hold that cell; value << 16 | index orders by value, then by smallest index
        __shared__ uint32_t best;
        if (tid == 0) best = 0xFFFFFFFFu;
        __syncthreads();
        const int k_a = FREE == AF_TEMPLATE ? (klo > rl - tl ? klo : rl - tl) : klo;
        const int k_b = FREE == AF_TEMPLATE ? khi : (khi < rl - tl ? khi : rl - tl);
        uint32_t mine = 0xFFFFFFFFu;
        for (int k = k_a + tid; k <= k_b; k += THREADS) {
            const int s = k - klo;
            const uint32_t key = ((uint32_t)val[(s & 1) * stride + 8 + (s >> 1)] << 16) | (uint32_t)(FREE == AF_TEMPLATE ? rl - k : k + tl);
            mine = key < mine ? key : mine;
        }
        if (mine != 0xFFFFFFFFu) atomicMin(&best, mine);
        __syncthreads();
        D = best >> 16;
        end = best & 0xFFFFu;
        s_end = (FREE == AF_TEMPLATE ? rl - (int)end : (int)end - tl) - klo;
        d_end = (FREE == AF_TEMPLATE ? rl : tl) + (int)end;
    }
    if (D > pr.t) {  // the band certifies nothing: the host widens it
        if (tid == 0) {
            dist[pr.out] = 0xFFFFFFFFu;
            n_ops[pr.out] = 0;
        }
        return;
    }
    if (tid >= 64) return;
    __threadfence_block();  // the wave reads back move codes other waves of the workgroup stored

    // ---- walk from (tl, rl) to (0, 0); every lane of wave 0 follows the same path, lane L stores op L of each stretch
    uint8_t *slot_end = ops_all + pr.ops_off + (uint64_t)(tl + rl);
    const uint16_t *tile16 = (const uint16_t *)tile;
    int d = d_end, s = s_end;
    uint32_t n = 0;
    while (walk_on<MODE, FREE>(d, klo + s)) {
        const int db_hi = d >> 3, db_lo = db_hi - (ALIGN_TILE_BLOCKS - 1);
        int g_lo = ((s >> 1) >> 3) - ALIGN_TILE_GROUPS / 2;
        if (g_lo < 0) g_lo = 0;
        for (int a = tid; a < ALIGN_TILE_BLOCKS * ALIGN_TILE_GROUPS; a += 64) {
            const int db = db_lo + a / ALIGN_TILE_GROUPS, g = g_lo + a % ALIGN_TILE_GROUPS;
            if (db >= 0 && g < G) tile[a] = scratch[pr.scratch_off + (uint64_t)db * G + g];
        }
        jtk_wave_sync();
        uint32_t nl = 0;
        while (walk_on<MODE, FREE>(d, klo + s) && nl < 64) {
            const int db = (d >> 3) - db_lo, c = s >> 1, g = (c >> 3) - g_lo;
            if (db < 0 || g < 0 || g >= ALIGN_TILE_GROUPS) break;
            const uint32_t w = tile16[(db * ALIGN_TILE_GROUPS + g) * 8 + (d & 7)];
            const uint32_t code = (w >> (2 * (c & 7))) & 3u;
            if (code <= MV_MISMATCH) {
                d -= 2;
            } else {
                d -= 1;
                s += code == MV_DEL ? 1 : -1;
            }
            if (tid == (int)nl) opbuf[tid] = (uint8_t)(code == MV_DEL ? JTK_OP_DEL : code == MV_INS ? JTK_OP_INS : code);
            nl++;
        }
        jtk_wave_sync();
        if ((uint32_t)tid < nl) *(slot_end - 1 - (n + tid)) = opbuf[tid];
        n += nl;
        jtk_wave_sync();
        if (nl == 0) break;  // cannot happen with the codes the fill wrote; never spin on anything else
    }
    if (tid == 0) {
        dist[pr.out] = (MODE == AM_INFIX ? !walk_on<MODE, FREE>(d, klo + s) : d == 0) ? D : ALIGN_WALK_LOST;
        n_ops[pr.out] = n;
        if constexpr (MODE != AM_GLOBAL) {  // at an infix stop the free index is d (the other one is 0)
            bounds[2 * pr.out] = MODE == AM_INFIX ? (uint32_t)d : 0u;
            bounds[2 * pr.out + 1] = end;
        }
    }
}

// ops of read r: the last n_ops[r] bytes of its slot -> ops_out[dst_off[r] ..]
__global__ __launch_bounds__(256) void align_pack_kernel(const uint8_t *ops_all, const uint64_t *slot_end, const uint64_t *dst_off,
                                                         uint32_t n_reads, uint8_t *ops_out) {
    const uint32_t r = blockIdx.x;
    if (r >= n_reads) return;
    const uint64_t a = dst_off[r], len = dst_off[r + 1] - a;
    const uint8_t *src = ops_all + slot_end[r] - len;
    for (uint64_t q = threadIdx.x; q < len; q += 256) ops_out[a + q] = src[q];
}

inline int groups_of(int W) { return ((W + 1) / 2 + 7) / 8; }
inline size_t lds_bytes_of(int G) { return (size_t)(2 * (8 * G + 16) + 8 * G) * 2 + 16; }

// The band of DESIGN section 4 for a distance bound t >= |rl - tl|, clipped to the matrix.
void band_of(uint32_t tl, uint32_t rl, uint32_t t, int32_t &klo, int32_t &khi) {
    const int32_t delta = (int32_t)rl - (int32_t)tl, e = (int32_t)(t - (uint32_t)std::abs(delta)) / 2;
    klo = (delta >= 0 ? 0 : delta) - e;
    khi = (delta >= 0 ? delta : 0) + e;
    klo = std::max(klo, -(int32_t)tl);
    khi = std::min(khi, (int32_t)rl);
}

// The band of DESIGN section 4 for infix / prefix and a distance bound t >= max(0, whole length - free length), clipped to
// the matrix: the free end may lie anywhere, so no halving as in band_of.
void mode_band_of(int mode, int free_seq, uint32_t tl, uint32_t rl, uint32_t t, int32_t &klo, int32_t &khi) {
    const int32_t delta = (int32_t)rl - (int32_t)tl, ti = (int32_t)t;
    klo = free_seq == AF_TEMPLATE ? delta - ti : -ti;
    khi = free_seq == AF_TEMPLATE ? ti : delta + ti;
    if (mode == AM_PREFIX) {  // the start is pinned to diagonal 0
        klo = std::max(klo, -ti);
        khi = std::min(khi, ti);
    }
    klo = std::max(klo, -(int32_t)tl);
    khi = std::min(khi, (int32_t)rl);
}

template <int THREADS, int MODE, int FREE>
int launch_align(size_t n, size_t lds, const AlignPair *d_pairs, const uint8_t *d_bases, uint4 *d_scratch, uint8_t *d_ops,
                 uint32_t *d_dist, uint32_t *d_nops, uint32_t *d_bounds) {
    if (lds > 48 * 1024)
        JTK_HIP_TRY(hipFuncSetAttribute((const void *)align_kernel<THREADS, MODE, FREE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((align_kernel<THREADS, MODE, FREE>), dim3((unsigned)n), dim3(THREADS), lds, 0, d_pairs, d_bases, d_scratch, d_ops,
                       d_dist, d_nops, d_bounds);
    JTK_HIP_TRY(hipGetLastError());
    return 0;
}

template <int THREADS>
int launch_align_any(int mode, int free_seq, size_t n, size_t lds, const AlignPair *d_pairs, const uint8_t *d_bases, uint4 *d_scratch,
                     uint8_t *d_ops, uint32_t *d_dist, uint32_t *d_nops, uint32_t *d_bounds) {
    if (mode == AM_GLOBAL) return launch_align<THREADS, AM_GLOBAL, AF_TEMPLATE>(n, lds, d_pairs, d_bases, d_scratch, d_ops, d_dist, d_nops, d_bounds);
    if (mode == AM_INFIX)
        return free_seq == AF_TEMPLATE
                   ? launch_align<THREADS, AM_INFIX, AF_TEMPLATE>(n, lds, d_pairs, d_bases, d_scratch, d_ops, d_dist, d_nops, d_bounds)
                   : launch_align<THREADS, AM_INFIX, AF_READ>(n, lds, d_pairs, d_bases, d_scratch, d_ops, d_dist, d_nops, d_bounds);
    return free_seq == AF_TEMPLATE
               ? launch_align<THREADS, AM_PREFIX, AF_TEMPLATE>(n, lds, d_pairs, d_bases, d_scratch, d_ops, d_dist, d_nops, d_bounds)
               : launch_align<THREADS, AM_PREFIX, AF_READ>(n, lds, d_pairs, d_bases, d_scratch, d_ops, d_dist, d_nops, d_bounds);
}

// Both entry points.  mode == AM_GLOBAL: start_out / end_out may be null and free_seq is not looked at.
int align_impl(size_t n_chunks, const jtk_lc_chunk_t *chunks, const uint8_t *tmpl_bases, const uint8_t *read_bases,
               const uint64_t *read_off, int mode, int free_seq, uint32_t max_dist, uint8_t *ops_out, uint64_t *ops_out_off,
               uint64_t ops_cap, uint32_t *dist_out, uint32_t *start_out, uint32_t *end_out, int32_t *read_status, int device) {
    g_last_error.clear();
    if (n_chunks && (!chunks || !tmpl_bases || !read_bases || !read_off)) return jtk_fail(JTK_ERR_INVALID_ARG, "null input");
    if (!ops_out || !ops_out_off || !dist_out || !read_status) return jtk_fail(JTK_ERR_INVALID_ARG, "null output");
    if (mode != AM_GLOBAL && (!start_out || !end_out)) return jtk_fail(JTK_ERR_INVALID_ARG, "null output");
    uint64_t n_reads = 0;
    if (int bad = check_contiguous(chunks, n_chunks, &n_reads)) return bad;
    for (uint64_t r = 0; r < n_reads; r++)
        if (read_off[r + 1] < read_off[r]) return jtk_fail(JTK_ERR_INVALID_ARG, "read_off is not ascending");
    auto acgt = [](const uint8_t *b, uint64_t n) {
        for (uint64_t q = 0; q < n; q++)
            if (b[q] != 'A' && b[q] != 'C' && b[q] != 'G' && b[q] != 'T') return false;
        return true;
    };
    for (size_t c = 0; c < n_chunks; c++)
        if (!acgt(tmpl_bases + chunks[c].tmpl_off, chunks[c].tmpl_len)) return jtk_fail(JTK_ERR_INVALID_ARG, "non-ACGT base in a template");
    if (n_reads && !acgt(read_bases + read_off[0], read_off[n_reads] - read_off[0]))
        return jtk_fail(JTK_ERR_INVALID_ARG, "non-ACGT base in a read");
    if (int bad = jtk_require_device(device)) return bad;

    // ---- padded base buffer and per-read work items
    struct Item {
        uint64_t tmpl_off, read_off, ops_off;
        uint32_t tl, rl, t, bound;
    };
    std::vector<Item> items(n_reads);
    std::vector<uint8_t> h_bases;
    std::vector<uint32_t> n_ops(n_reads, 0);
    std::vector<uint64_t> slot_end(n_reads, 0);
    std::vector<uint32_t> pending;
    std::vector<uint32_t> settled;  // infix / prefix reads with an empty side: decided here
    {
        uint64_t need = ALIGN_PAD;
        for (size_t c = 0; c < n_chunks; c++) need += chunks[c].tmpl_len + ALIGN_PAD;
        need += (n_reads ? read_off[n_reads] - read_off[0] : 0) + ALIGN_PAD * n_reads;
        h_bases.assign(need, 0);
    }
    uint64_t bo = ALIGN_PAD, slot = 0;
    for (size_t c = 0; c < n_chunks; c++) {
        const jtk_lc_chunk_t &ch = chunks[c];
        const uint64_t t_at = bo;
        memcpy(h_bases.data() + bo, tmpl_bases + ch.tmpl_off, ch.tmpl_len);
        bo += ch.tmpl_len + ALIGN_PAD;
        for (uint32_t q = 0; q < ch.n_reads; q++) {
            const uint64_t r = ch.read_first + q, rl = read_off[r + 1] - read_off[r], tl = ch.tmpl_len;
            Item &it = items[r];
            it.tmpl_off = t_at;
            it.read_off = bo;
            memcpy(h_bases.data() + bo, read_bases + read_off[r], rl);
            bo += rl + ALIGN_PAD;
            read_status[r] = 0;
            dist_out[r] = 0xFFFFFFFFu;
            if (mode != AM_GLOBAL) start_out[r] = end_out[r] = 0;
            if (tl > ALIGN_MAX_LEN || rl > ALIGN_MAX_LEN) {
                read_status[r] = JTK_ERR_UNSUPPORTED;
                continue;
            }
            it.tl = (uint32_t)tl;
            it.rl = (uint32_t)rl;
            it.ops_off = slot;
            slot += tl + rl;
            slot_end[r] = slot;
            if (mode != AM_GLOBAL) {
                const uint64_t wl = free_seq == AF_TEMPLATE ? rl : tl, fl = free_seq == AF_TEMPLATE ? tl : rl;
                if (wl == 0 || fl == 0) {  // nothing to place, or nowhere to place it: the whole sequence as Ins (Del)
                    it.t = (uint32_t)wl;  // its distance and its op count
                    settled.push_back((uint32_t)r);
                    continue;
                }
                const uint32_t low = (uint32_t)(wl > fl ? wl - fl : 0);  // the whole sequence cannot lose fewer bases
                it.bound = max_dist && max_dist < wl ? max_dist : (uint32_t)wl;  // the distance never exceeds the whole sequence
                int32_t klo, khi;
                mode_band_of(mode, free_seq, it.tl, it.rl, it.bound, klo, khi);
                if (low > it.bound || khi - klo + 1 > ALIGN_MODE_MAX_BAND) {
                    read_status[r] = JTK_ERR_UNSUPPORTED;
                    continue;
                }
                // first try: a sixth of the whole sequence, as the global schedule's twelfth of two equal lengths
                it.t = std::min<uint32_t>(it.bound, low + std::max<uint32_t>(32u, (uint32_t)(wl / 6)));
                pending.push_back((uint32_t)r);
                continue;
            }
            const uint32_t delta = (uint32_t)(tl > rl ? tl - rl : rl - tl), longest = (uint32_t)std::max(tl, rl);
            it.bound = max_dist && max_dist < longest ? max_dist : longest;  // the distance never exceeds the longer sequence
            if (delta > it.bound) {
                read_status[r] = JTK_ERR_UNSUPPORTED;
                continue;
            }
            // first try: the length difference plus a twelfth of the summed lengths (a 2 kbp ONT read at 12 % passes at once)
            it.t = std::min<uint32_t>(it.bound, delta + std::max<uint32_t>(32u, (uint32_t)((tl + rl) / 12)));
            pending.push_back((uint32_t)r);
        }
    }

    DevBuf d_bases, d_ops, d_dist, d_nops, d_pairs, d_scratch, d_bounds;
    JTK_HIP_TRY(d_bases.alloc(h_bases.size()));
    JTK_HIP_TRY(hipMemcpy(d_bases.p, h_bases.data(), h_bases.size(), hipMemcpyHostToDevice));
    JTK_HIP_TRY(d_ops.alloc(slot + 16));
    JTK_HIP_TRY(d_dist.alloc((n_reads + 1) * 4));
    JTK_HIP_TRY(d_nops.alloc((n_reads + 1) * 4));
    JTK_HIP_TRY(hipMemset(d_nops.p, 0, (n_reads + 1) * 4));
    JTK_HIP_TRY(hipMemset(d_dist.p, 0xFF, (n_reads + 1) * 4));
    if (mode != AM_GLOBAL) {
        JTK_HIP_TRY(d_bounds.alloc((n_reads + 1) * 8));
        JTK_HIP_TRY(hipMemset(d_bounds.p, 0, (n_reads + 1) * 8));
        for (uint32_t r : settled)  // with the free side empty the slot of tl + rl bytes is the whole sequence's
            if (items[r].t)
                JTK_HIP_TRY(hipMemset((uint8_t *)d_ops.p + items[r].ops_off, free_seq == AF_TEMPLATE ? JTK_OP_INS : JTK_OP_DEL, items[r].t));
    }

    // ---- rounds: every pending pair with its current t; those that come back above it double t
    const uint64_t budget16 = (uint64_t)4 << (30 - 4);  // move-code scratch per launch: 4 GiB, in 16-byte units
    uint64_t scratch_have = 0;
    size_t pairs_have = 0;
    std::vector<uint32_t> h_dist(n_reads);
    while (!pending.empty()) {
        // wide bands first; a launch holds pairs of one workgroup size
        std::vector<AlignPair> prs(pending.size());
        for (size_t a = 0; a < pending.size(); a++) {
            const Item &it = items[pending[a]];
            AlignPair &p = prs[a];
            p.tmpl_off = it.tmpl_off;
            p.read_off = it.read_off;
            p.ops_off = it.ops_off;
            p.tmpl_len = it.tl;
            p.read_len = it.rl;
            p.t = it.t;
            p.out = pending[a];
            if (mode == AM_GLOBAL)
                band_of(it.tl, it.rl, it.t, p.klo, p.khi);
            else
                mode_band_of(mode, free_seq, it.tl, it.rl, it.t, p.klo, p.khi);
        }
        std::stable_sort(prs.begin(), prs.end(), [](const AlignPair &a, const AlignPair &b) { return a.khi - a.klo > b.khi - b.klo; });
        if (prs.size() > pairs_have) {
            JTK_HIP_TRY(d_pairs.alloc(prs.size() * sizeof(AlignPair)));
            pairs_have = prs.size();
        }
        size_t a = 0;
        while (a < prs.size()) {
            const int G0 = groups_of(prs[a].khi - prs[a].klo + 1);
            const int threads = G0 <= 64 ? 64 : G0 <= 256 ? 256 : 1024;
            const int g_min = threads == 64 ? 0 : threads == 256 ? 65 : 257;
            uint64_t used = 0;
            size_t b = a;
            while (b < prs.size()) {
                const int G = groups_of(prs[b].khi - prs[b].klo + 1);
                const uint64_t sz = (uint64_t)((prs[b].tmpl_len + prs[b].read_len) / 8 + 1) * G;
                if (G < g_min || (b > a && used + sz > budget16)) break;
                prs[b].scratch_off = used;
                used += sz;
                b++;
            }
            if (used > scratch_have) {
                scratch_have = 0;
                JTK_HIP_TRY(d_scratch.alloc(used * 16));
                scratch_have = used;
            }
            JTK_HIP_TRY(hipMemcpy((AlignPair *)d_pairs.p + a, prs.data() + a, (b - a) * sizeof(AlignPair), hipMemcpyHostToDevice));
            const size_t lds = lds_bytes_of(G0);  // the launch's widest band comes first
            int rc;
            if (threads == 64)
                rc = launch_align_any<64>(mode, free_seq, b - a, lds, (AlignPair *)d_pairs.p + a, (uint8_t *)d_bases.p, (uint4 *)d_scratch.p,
                                          (uint8_t *)d_ops.p, (uint32_t *)d_dist.p, (uint32_t *)d_nops.p, (uint32_t *)d_bounds.p);
            else if (threads == 256)
                rc = launch_align_any<256>(mode, free_seq, b - a, lds, (AlignPair *)d_pairs.p + a, (uint8_t *)d_bases.p, (uint4 *)d_scratch.p,
                                           (uint8_t *)d_ops.p, (uint32_t *)d_dist.p, (uint32_t *)d_nops.p, (uint32_t *)d_bounds.p);
            else
                rc = launch_align_any<1024>(mode, free_seq, b - a, lds, (AlignPair *)d_pairs.p + a, (uint8_t *)d_bases.p, (uint4 *)d_scratch.p,
                                            (uint8_t *)d_ops.p, (uint32_t *)d_dist.p, (uint32_t *)d_nops.p, (uint32_t *)d_bounds.p);
            if (rc) return rc;
            JTK_HIP_TRY(hipDeviceSynchronize());  // the next launch reuses the scratch
            a = b;
        }
        JTK_HIP_TRY(hipMemcpy(h_dist.data(), d_dist.p, n_reads * 4, hipMemcpyDeviceToHost));
        std::vector<uint32_t> again;
        for (uint32_t r : pending) {
            Item &it = items[r];
            if (h_dist[r] == ALIGN_WALK_LOST) return jtk_fail(JTK_ERR_INTERNAL, "align: the walk left the band");
            if (h_dist[r] != 0xFFFFFFFFu) continue;
            if (it.t >= it.bound) {
                read_status[r] = JTK_ERR_UNSUPPORTED;  // farther than max_dist
                continue;
            }
            it.t = (uint32_t)std::min<uint64_t>((uint64_t)it.t * 2, it.bound);
            again.push_back(r);
        }
        pending.swap(again);
    }

    // ---- pack the ops of every read behind each other and fetch them with one copy
    JTK_HIP_TRY(hipMemcpy(n_ops.data(), d_nops.p, n_reads * 4, hipMemcpyDeviceToHost));
    JTK_HIP_TRY(hipMemcpy(h_dist.data(), d_dist.p, n_reads * 4, hipMemcpyDeviceToHost));
    for (uint32_t r : settled) n_ops[r] = h_dist[r] = items[r].t;
    if (mode != AM_GLOBAL) {
        std::vector<uint32_t> h_bounds(2 * n_reads + 2);
        JTK_HIP_TRY(hipMemcpy(h_bounds.data(), d_bounds.p, n_reads * 8, hipMemcpyDeviceToHost));
        for (uint64_t r = 0; r < n_reads; r++)
            if (!read_status[r]) {
                start_out[r] = h_bounds[2 * r];
                end_out[r] = h_bounds[2 * r + 1];
            }
    }
    int rc = 0;
    uint64_t total = 0;
    for (uint64_t r = 0; r < n_reads; r++) {
        ops_out_off[r] = total;
        if (read_status[r]) {
            rc = JTK_ERR_CHUNK_FAILED;
            n_ops[r] = 0;
            continue;
        }
        dist_out[r] = h_dist[r];
        total += n_ops[r];
    }
    ops_out_off[n_reads] = total;
    if (total > ops_cap) return jtk_fail(JTK_ERR_INVALID_ARG, "ops_cap is smaller than the ops of the batch");
    if (total) {
        DevBuf d_off, d_end, d_out;
        JTK_HIP_TRY(d_off.alloc((n_reads + 1) * 8));
        JTK_HIP_TRY(d_end.alloc(n_reads * 8));
        JTK_HIP_TRY(d_out.alloc(total));
        JTK_HIP_TRY(hipMemcpy(d_off.p, ops_out_off, (n_reads + 1) * 8, hipMemcpyHostToDevice));
        JTK_HIP_TRY(hipMemcpy(d_end.p, slot_end.data(), n_reads * 8, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(align_pack_kernel, dim3((unsigned)n_reads), dim3(256), 0, 0, (const uint8_t *)d_ops.p, (const uint64_t *)d_end.p,
                           (const uint64_t *)d_off.p, (uint32_t)n_reads, (uint8_t *)d_out.p);
        JTK_HIP_TRY(hipGetLastError());
        JTK_HIP_TRY(hipMemcpy(ops_out, d_out.p, total, hipMemcpyDeviceToHost));
    }
    if (rc)
        return jtk_fail(rc, mode == AM_GLOBAL
                                ? "a read lies farther from its template than max_dist (or is longer than 32,000 bases)"
                                : "a pair lies farther apart than max_dist (or is longer than 32,000 bases, or its band at the "
                                  "largest distance allowed is wider than 32,768 diagonals: give max_dist)");
    return 0;
}

}  // namespace

extern "C" int jtk_lc_align_reads(size_t n_chunks, const jtk_lc_chunk_t *chunks, const uint8_t *tmpl_bases,
                                  const uint8_t *read_bases, const uint64_t *read_off, uint32_t max_dist, uint8_t *ops_out,
                                  uint64_t *ops_out_off, uint64_t ops_cap, uint32_t *dist_out, int32_t *read_status, int device) {
    return align_impl(n_chunks, chunks, tmpl_bases, read_bases, read_off, AM_GLOBAL, AF_TEMPLATE, max_dist, ops_out, ops_out_off,
                      ops_cap, dist_out, nullptr, nullptr, read_status, device);
}

extern "C" int jtk_lc_align_reads_mode(size_t n_chunks, const jtk_lc_chunk_t *chunks, const uint8_t *tmpl_bases,
                                       const uint8_t *read_bases, const uint64_t *read_off, int mode, int free_seq,
                                       uint32_t max_dist, uint8_t *ops_out, uint64_t *ops_out_off, uint64_t ops_cap,
                                       uint32_t *dist_out, uint32_t *start_out, uint32_t *end_out, int32_t *read_status, int device) {
    if (mode != JTK_ALIGN_GLOBAL && mode != JTK_ALIGN_INFIX && mode != JTK_ALIGN_PREFIX) return jtk_fail(JTK_ERR_INVALID_ARG, "unknown alignment mode");
    if (mode != JTK_ALIGN_GLOBAL && free_seq != JTK_ALIGN_FREE_TEMPLATE && free_seq != JTK_ALIGN_FREE_READ)
        return jtk_fail(JTK_ERR_INVALID_ARG, "unknown free sequence");
    if (!start_out || !end_out) return jtk_fail(JTK_ERR_INVALID_ARG, "null output");
    const int rc = align_impl(n_chunks, chunks, tmpl_bases, read_bases, read_off, mode, free_seq, max_dist, ops_out, ops_out_off, ops_cap,
                              dist_out, start_out, end_out, read_status, device);
    if (mode == JTK_ALIGN_GLOBAL && (rc == 0 || rc == JTK_ERR_CHUNK_FAILED))  // everything is consumed: [0, template length)
        for (size_t c = 0; c < n_chunks; c++)
            for (uint32_t q = 0; q < chunks[c].n_reads; q++) {
                const uint64_t r = chunks[c].read_first + q;
                start_out[r] = 0;
                end_out[r] = read_status[r] ? 0 : (uint32_t)chunks[c].tmpl_len;
            }
    return rc;
}
