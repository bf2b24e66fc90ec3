// align_kernels.hip -- jtk_lc_align_reads: batched global unit-cost alignment of reads to their templates (the reference's
// edlib Global / Alignment calls: consensus/mod.rs:424-435, polish_chunks.rs:114-120).  Specification: DESIGN.md section 4.
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
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "device_common.h"

extern "C" void jtk_internal_set_error(const char *msg);

#define ALIGN_MAX_LEN 32000u  // tl + rl stays below the 16-bit infinity
#define ALIGN_INF 0xFFFFu
#define ALIGN_PAD 16          // bytes in front of and behind every sequence: a thread loads its 8 bases unaligned
#define ALIGN_WALK_LOST 0xFFFFFFFEu  // dist marker: the walk left the band (an internal error, reported as such)
#define ALIGN_TILE_GROUPS 11
#define ALIGN_TILE_BLOCKS 8

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

__device__ __forceinline__ uint64_t load_u64_unaligned(const uint8_t *p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

// LDS written by some lanes of the wave, read by others
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void align_kernel(const AlignPair *pairs, const uint8_t *bases, uint4 *scratch,
                                                        uint8_t *ops_all, uint32_t *dist, uint32_t *n_ops) {
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

    const int s_end = rl - tl - klo;
    const uint32_t D = val[(s_end & 1) * stride + 8 + (s_end >> 1)];
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
    int d = dmax, s = s_end;
    uint32_t n = 0;
    while (d > 0) {
        const int db_hi = d >> 3, db_lo = db_hi - (ALIGN_TILE_BLOCKS - 1);
        int g_lo = ((s >> 1) >> 3) - ALIGN_TILE_GROUPS / 2;
        if (g_lo < 0) g_lo = 0;
        for (int a = tid; a < ALIGN_TILE_BLOCKS * ALIGN_TILE_GROUPS; a += 64) {
            const int db = db_lo + a / ALIGN_TILE_GROUPS, g = g_lo + a % ALIGN_TILE_GROUPS;
            if (db >= 0 && g < G) tile[a] = scratch[pr.scratch_off + (uint64_t)db * G + g];
        }
        wave_sync();
        uint32_t nl = 0;
        while (d > 0 && nl < 64) {
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
        wave_sync();
        if ((uint32_t)tid < nl) *(slot_end - 1 - (n + tid)) = opbuf[tid];
        n += nl;
        wave_sync();
        if (nl == 0) break;  // cannot happen with the codes the fill wrote; never spin on anything else
    }
    if (tid == 0) {
        dist[pr.out] = d == 0 ? D : ALIGN_WALK_LOST;
        n_ops[pr.out] = n;
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

int afail(int rc, const std::string &msg) {
    jtk_internal_set_error(msg.c_str());
    return rc;
}

#define ALIGN_HIP(expr)                                                                                  \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess)                                                                            \
            return afail(e_ == hipErrorOutOfMemory ? JTK_ERR_ALLOC : JTK_ERR_NO_DEVICE,                  \
                         std::string(#expr) + ": " + hipGetErrorString(e_));                             \
    } while (0)

struct DevMem {
    void *p = nullptr;
    ~DevMem() {
        if (p) (void)hipFree(p);
    }
};

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

template <int THREADS>
int launch_align(size_t n, size_t lds, const AlignPair *d_pairs, const uint8_t *d_bases, uint4 *d_scratch, uint8_t *d_ops,
                 uint32_t *d_dist, uint32_t *d_nops) {
    if (lds > 48 * 1024)
        ALIGN_HIP(hipFuncSetAttribute((const void *)align_kernel<THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(align_kernel<THREADS>, dim3((unsigned)n), dim3(THREADS), lds, 0, d_pairs, d_bases, d_scratch, d_ops, d_dist,
                       d_nops);
    ALIGN_HIP(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" int jtk_lc_align_reads(size_t n_chunks, const jtk_lc_chunk_t *chunks, const uint8_t *tmpl_bases,
                                  const uint8_t *read_bases, const uint64_t *read_off, uint32_t max_dist, uint8_t *ops_out,
                                  uint64_t *ops_out_off, uint64_t ops_cap, uint32_t *dist_out, int32_t *read_status, int device) {
    jtk_internal_set_error("");
    if (n_chunks && (!chunks || !tmpl_bases || !read_bases || !read_off)) return afail(JTK_ERR_INVALID_ARG, "null input");
    if (!ops_out || !ops_out_off || !dist_out || !read_status) return afail(JTK_ERR_INVALID_ARG, "null output");
    uint64_t n_reads = 0;
    for (size_t c = 0; c < n_chunks; c++) {
        if (chunks[c].read_first != n_reads) return afail(JTK_ERR_INVALID_ARG, "chunks must list their reads contiguously in order");
        n_reads += chunks[c].n_reads;
    }
    for (uint64_t r = 0; r < n_reads; r++)
        if (read_off[r + 1] < read_off[r]) return afail(JTK_ERR_INVALID_ARG, "read_off is not ascending");
    auto acgt = [](const uint8_t *b, uint64_t n) {
        for (uint64_t q = 0; q < n; q++)
            if (b[q] != 'A' && b[q] != 'C' && b[q] != 'G' && b[q] != 'T') return false;
        return true;
    };
    for (size_t c = 0; c < n_chunks; c++)
        if (!acgt(tmpl_bases + chunks[c].tmpl_off, chunks[c].tmpl_len)) return afail(JTK_ERR_INVALID_ARG, "non-ACGT base in a template");
    if (n_reads && !acgt(read_bases + read_off[0], read_off[n_reads] - read_off[0]))
        return afail(JTK_ERR_INVALID_ARG, "non-ACGT base in a read");
    if (!jtk_lc_device_ok(device)) return afail(JTK_ERR_NO_DEVICE, "no gfx950 device (jtk_lc has no CPU fallback)");
    ALIGN_HIP(hipSetDevice(device));

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
            if (tl > ALIGN_MAX_LEN || rl > ALIGN_MAX_LEN) {
                read_status[r] = JTK_ERR_UNSUPPORTED;
                continue;
            }
            it.tl = (uint32_t)tl;
            it.rl = (uint32_t)rl;
            it.ops_off = slot;
            slot += tl + rl;
            slot_end[r] = slot;
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

    DevMem d_bases, d_ops, d_dist, d_nops, d_pairs, d_scratch;
    ALIGN_HIP(hipMalloc(&d_bases.p, h_bases.size()));
    ALIGN_HIP(hipMemcpy(d_bases.p, h_bases.data(), h_bases.size(), hipMemcpyHostToDevice));
    ALIGN_HIP(hipMalloc(&d_ops.p, slot + 16));
    ALIGN_HIP(hipMalloc(&d_dist.p, (n_reads + 1) * 4));
    ALIGN_HIP(hipMalloc(&d_nops.p, (n_reads + 1) * 4));
    ALIGN_HIP(hipMemset(d_nops.p, 0, (n_reads + 1) * 4));
    ALIGN_HIP(hipMemset(d_dist.p, 0xFF, (n_reads + 1) * 4));

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
            band_of(it.tl, it.rl, it.t, p.klo, p.khi);
        }
        std::stable_sort(prs.begin(), prs.end(), [](const AlignPair &a, const AlignPair &b) { return a.khi - a.klo > b.khi - b.klo; });
        if (prs.size() > pairs_have) {
            if (d_pairs.p) (void)hipFree(d_pairs.p);
            d_pairs.p = nullptr;
            ALIGN_HIP(hipMalloc(&d_pairs.p, prs.size() * sizeof(AlignPair)));
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
                if (d_scratch.p) (void)hipFree(d_scratch.p);
                d_scratch.p = nullptr;
                scratch_have = 0;
                ALIGN_HIP(hipMalloc(&d_scratch.p, used * 16));
                scratch_have = used;
            }
            ALIGN_HIP(hipMemcpy((AlignPair *)d_pairs.p + a, prs.data() + a, (b - a) * sizeof(AlignPair), hipMemcpyHostToDevice));
            const size_t lds = lds_bytes_of(G0);  // the launch's widest band comes first
            int rc;
            if (threads == 64)
                rc = launch_align<64>(b - a, lds, (AlignPair *)d_pairs.p + a, (uint8_t *)d_bases.p, (uint4 *)d_scratch.p, (uint8_t *)d_ops.p,
                                      (uint32_t *)d_dist.p, (uint32_t *)d_nops.p);
            else if (threads == 256)
                rc = launch_align<256>(b - a, lds, (AlignPair *)d_pairs.p + a, (uint8_t *)d_bases.p, (uint4 *)d_scratch.p, (uint8_t *)d_ops.p,
                                       (uint32_t *)d_dist.p, (uint32_t *)d_nops.p);
            else
                rc = launch_align<1024>(b - a, lds, (AlignPair *)d_pairs.p + a, (uint8_t *)d_bases.p, (uint4 *)d_scratch.p, (uint8_t *)d_ops.p,
                                        (uint32_t *)d_dist.p, (uint32_t *)d_nops.p);
            if (rc) return rc;
            ALIGN_HIP(hipDeviceSynchronize());  // the next launch reuses the scratch
            a = b;
        }
        ALIGN_HIP(hipMemcpy(h_dist.data(), d_dist.p, n_reads * 4, hipMemcpyDeviceToHost));
        std::vector<uint32_t> again;
        for (uint32_t r : pending) {
            Item &it = items[r];
            if (h_dist[r] == ALIGN_WALK_LOST) return afail(JTK_ERR_INTERNAL, "align: the walk left the band");
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
    ALIGN_HIP(hipMemcpy(n_ops.data(), d_nops.p, n_reads * 4, hipMemcpyDeviceToHost));
    ALIGN_HIP(hipMemcpy(h_dist.data(), d_dist.p, n_reads * 4, hipMemcpyDeviceToHost));
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
    if (total > ops_cap) return afail(JTK_ERR_INVALID_ARG, "ops_cap is smaller than the ops of the batch");
    if (total) {
        DevMem d_off, d_end, d_out;
        ALIGN_HIP(hipMalloc(&d_off.p, (n_reads + 1) * 8));
        ALIGN_HIP(hipMalloc(&d_end.p, n_reads * 8));
        ALIGN_HIP(hipMalloc(&d_out.p, total));
        ALIGN_HIP(hipMemcpy(d_off.p, ops_out_off, (n_reads + 1) * 8, hipMemcpyHostToDevice));
        ALIGN_HIP(hipMemcpy(d_end.p, slot_end.data(), n_reads * 8, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(align_pack_kernel, dim3((unsigned)n_reads), dim3(256), 0, 0, (const uint8_t *)d_ops.p, (const uint64_t *)d_end.p,
                           (const uint64_t *)d_off.p, (uint32_t)n_reads, (uint8_t *)d_out.p);
        ALIGN_HIP(hipGetLastError());
        ALIGN_HIP(hipMemcpy(ops_out, d_out.p, total, hipMemcpyDeviceToHost));
    }
    if (rc) jtk_internal_set_error("a read lies farther from its template than max_dist (or is longer than 32,000 bases)");
    return rc;
}
