// wave_util.h -- the device helpers the one-wave-per-item primitives share: the wave-local barrier (fill, guided, encode_nodes,
// gpolish, align_kernels) and the band of a guided alignment (guided, gpolish).  The session's kernels do not include it.
#pragma once
#include <hip/hip_runtime.h>

#include "jtk_lc.h"

// memory written by some lanes of the wave, read by others
__device__ __forceinline__ void jtk_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The band of one pair (x of n bases, rows; y of m bases, columns) around its guide, by one wave: the band shape of DESIGN.md
// section 4, which jtk_lc_align_guided, jtk_lc_encode_nodes and jtk_lc_polish_guided share -- "radius" means this.
//   1. The walk over the guide's ops (64 per coalesced load, then lane-uniform steps on registers) from cell (0, 0): Match and
//      Mismatch step diagonally, Del down a row, Ins along the row; an op that would leave the table is skipped.  Row i is opened
//      with lo[i] when the path enters it and closed with hi[i] when it leaves, so [lo[i], hi[i]] are the path's columns in row i.
//   2. The tail: where the guide ends short of (n, m) the path goes on diagonally, then by Del, then by Ins.
//   3. The band: row i spans the columns [max(lo[i] - r, 0), min(hi[i] + r, m)], r = min(radius, max(n, m) + 1) (wider changes
//      nothing).  A prefix sum over the rows' widths, 64 rows per step, leaves
//          lo[i] = the band's first column in row i                  (i = 0 ..= n)
//          hi[i] = the cells of the band in the rows above row i     (i = 0 ..= n + 1; hi[n + 1] = all of them, also *cells)
//      and the widest row is returned.
// lo and hi hold n + 2 entries each.  Every lane of the wave calls it and gets the same results; there is no barrier behind the
// last stores: the caller calls jtk_wave_sync() before other lanes read lo / hi.
__device__ __forceinline__ uint32_t jtk_band_rows(uint32_t n, uint32_t m, uint32_t radius, const uint8_t *guide, uint32_t guide_len, uint32_t *lo,
                                                  uint32_t *hi, uint32_t lane, uint32_t *cells) {
    const uint32_t longest = n > m ? n : m;
    const uint32_t r = radius > longest ? longest + 1 : radius;
    // ---- the walk
    uint32_t i = 0, j = 0;
    if (lane == 0) lo[0] = 0;
    for (uint32_t base = 0; base < guide_len; base += 64) {
        const uint32_t cnt = guide_len - base < 64u ? guide_len - base : 64u;
        const int mine = lane < cnt ? (int)guide[base + lane] : 2;
        for (uint32_t t = 0; t < cnt; t++) {
            const int op = __shfl(mine, (int)t, 64);
            if (op <= JTK_OP_MISMATCH) {
                if (i < n && j < m) {
                    if (lane == 0) {
                        hi[i] = j;
                        lo[i + 1] = j + 1;
                    }
                    i++;
                    j++;
                }
            } else if (op == JTK_OP_DEL) {
                if (i < n) {
                    if (lane == 0) {
                        hi[i] = j;
                        lo[i + 1] = j;
                    }
                    i++;
                }
            } else if (j < m) {
                j++;
            }
        }
    }
    {  // the rest: diagonally, then by Del, then by Ins
        const uint32_t d = n - i < m - j ? n - i : m - j;
        for (uint32_t row = i + lane; row <= n; row += 64) {
            const uint32_t col = j + (row - i < d ? row - i : d);
            if (row > i) lo[row] = col;
            hi[row] = row == n ? m : col;
        }
    }
    jtk_wave_sync();
    // ---- the band and the prefix sum of its widths
    uint32_t carry = 0, widest = 0;
    for (uint32_t base = 0; base <= n; base += 64) {
        const uint32_t row = base + lane;
        uint32_t width = 0, first = 0;
        if (row <= n) {
            const uint32_t l = lo[row], h = hi[row];
            first = l > r ? l - r : 0;
            const uint32_t last = h + r < m ? h + r : m;
            width = last - first + 1;
        }
        uint32_t incl = width;
#pragma unroll
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const uint32_t u = __shfl_up(incl, o, 64);
            if (lane >= o) incl += u;
        }
        if (row <= n) {
            lo[row] = first;
            hi[row] = carry + incl - width;
        }
        carry += __shfl(incl, 63, 64);
        widest = width > widest ? width : widest;
    }
    for (uint32_t o = 32; o; o >>= 1) {
        const uint32_t u = __shfl_xor(widest, o, 64);
        widest = u > widest ? u : widest;
    }
    if (lane == 0) hi[n + 1] = carry;
    *cells = carry;
    return widest;
}
