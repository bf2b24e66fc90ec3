"""Independent numpy restatement of the infix and prefix alignments of DESIGN.md section 4 (what jtk_lc_align_reads_mode
computes), written from the text of the specification; it shares the sequence helpers of tests/align_reference.py and nothing
with the device.

  One sequence is whole, the other free.  With the template x free (index i) and the read y whole (index j):
    infix : D(i,0) = 0, D(0,j) = j;  prefix: D(i,0) = i, D(0,j) = j;  the recurrence of the global alignment inside;
    distance = min_i D(i, rl), end = the smallest i attaining it; the walk starts at (end, rl), takes the first move that
    reproduces D(i,j) in the order diagonal, Del (i-1, j), Ins (i, j-1) and stops at the first cell with j == 0 (infix; its i
    is start) or at (0, 0) (prefix; start = 0).
  With the read free the roles of i and j are exchanged in the boundary, the minimum (over D(tl, j), smallest j) and the stop
  (i == 0); the order of the moves is not.
  Whole sequence empty: distance 0, no ops, start = end = 0.  Free sequence empty: whole-length x Ins (the read is whole) or
  x Del (the template is whole), start = end = 0."""
import numpy as np

import align_reference as A

GLOBAL, INFIX, PREFIX = 0, 1, 2
FREE_TEMPLATE, FREE_READ = 0, 1
MODES = {"global": GLOBAL, "infix": INFIX, "prefix": PREFIX}
FREES = {"template": FREE_TEMPLATE, "read": FREE_READ}
BIG = A.BIG


def band_of(tl, rl, t, mode, free):
    """diagonals j - i the fill may touch for a distance bound t, clipped to the matrix"""
    delta = rl - tl
    klo, khi = (delta - t, t) if free == FREE_TEMPLATE else (-t, delta + t)
    if mode == PREFIX:
        klo, khi = max(klo, -t), min(khi, t)
    return max(klo, -tl), min(khi, rl)


def fill(x, y, mode, free, band=None):
    """(tl+1) x (rl+1) matrix with the boundary of the mode; off the band (klo, khi) cells hold BIG"""
    x, y = A.seq(x), A.seq(y)
    tl, rl = len(x), len(y)
    cols = np.arange(rl + 1, dtype=np.int64)

    def off_band(i):
        return (cols - i < band[0]) | (cols - i > band[1])

    D = np.empty((tl + 1, rl + 1), dtype=np.int64)
    row = np.zeros(rl + 1, dtype=np.int64) if (mode == INFIX and free == FREE_READ) else cols.copy()
    if band is not None:
        row[off_band(0)] = BIG
    D[0] = row
    for i in range(1, tl + 1):
        prev = D[i - 1]
        cur = np.full(rl + 1, BIG, dtype=np.int64)
        cur[0] = 0 if (mode == INFIX and free == FREE_TEMPLATE) else i
        cur[1:] = np.minimum(prev[:-1] + (y != x[i - 1]), prev[1:] + 1)
        if band is not None:
            cur[off_band(i)] = BIG
        cur = np.minimum(np.minimum.accumulate(cur - cols) + cols, BIG)      # D(i,j-1) + 1 along the row
        if band is not None:
            cur[off_band(i)] = BIG
        D[i] = cur
    return D


def end_of(D, free):
    """-> (distance, end): the minimum over the last row (template free: column rl of the matrix) or the last column (read
    free: row tl), the smallest index attaining it"""
    line = D[:, -1] if free == FREE_TEMPLATE else D[-1, :]
    end = int(np.argmin(line))                                                # the first occurrence of the minimum
    return int(line[end]), end


def walk(D, x, y, mode, free, end):
    """-> (ops front to back, start)"""
    x, y = A.seq(x), A.seq(y)
    i, j = (end, len(y)) if free == FREE_TEMPLATE else (len(x), end)
    out = []
    while True:
        if mode == INFIX and (j == 0 if free == FREE_TEMPLATE else i == 0):
            break
        if mode == PREFIX and i == 0 and j == 0:
            break
        here = int(D[i, j])
        if i > 0 and j > 0 and here == int(D[i - 1, j - 1]) + (1 if x[i - 1] != y[j - 1] else 0):
            out.append(A.MATCH if x[i - 1] == y[j - 1] else A.MISMATCH)
            i, j = i - 1, j - 1
        elif i > 0 and here == int(D[i - 1, j]) + 1:
            out.append(A.DEL)
            i -= 1
        else:
            assert j > 0 and here == int(D[i, j - 1]) + 1, (i, j)
            out.append(A.INS)
            j -= 1
    return np.array(out[::-1], dtype=np.uint8), (i if free == FREE_TEMPLATE else j)


def _degenerate(x, y, free):
    whole, free_seq = (y, x) if free == FREE_TEMPLATE else (x, y)
    if len(whole) == 0:
        return np.zeros(0, np.uint8), 0, 0, 0
    if len(free_seq) == 0:
        op = A.INS if free == FREE_TEMPLATE else A.DEL
        return np.full(len(whole), op, np.uint8), len(whole), 0, 0
    return None


def align(x, y, mode, free, t=None):
    """-> (ops, distance, start, end) of template x and read y; with a distance bound t the fill is restricted to band_of
    and the ops are None when the banded distance exceeds t (the distance returned is then the banded value)"""
    x, y = A.seq(x), A.seq(y)
    if mode == GLOBAL:
        ops, d = A.align(x, y) if t is None else A.align_banded(x, y, t)
        return ops, d, 0, len(x)
    deg = _degenerate(x, y, free)
    if deg is not None:
        return deg
    D = fill(x, y, mode, free, band=None if t is None else band_of(len(x), len(y), t, mode, free))
    d, end = end_of(D, free)
    if t is not None and d > t:
        return None, d, None, None
    ops, start = walk(D, x, y, mode, free, end)
    return ops, d, start, end


def first_t(tl, rl, free, max_dist=0):
    """the schedule of DESIGN section 5: (first t, its cap)"""
    wl, fl = (rl, tl) if free == FREE_TEMPLATE else (tl, rl)
    bound = max_dist if max_dist and max_dist < wl else wl
    return min(bound, max(wl - fl, 0) + max(32, wl // 6)), bound


def widenings(tl, rl, free, d):
    """how often the schedule doubles t before it reaches d"""
    t, bound = first_t(tl, rl, free)
    n = 0
    while t < d:
        t, n = min(2 * t, bound), n + 1
    return n


def semiglobal(refr, query):
    """`semiglobal` of encode/mod.rs:227-246 on this specification: refr (the template) whole, query (the read) free, infix;
    start x Ins, the ops, the rest x Ins -> ops that consume both sequences whole"""
    refr, query = A.seq(refr), A.seq(query)
    if len(refr) == 0:
        return np.full(len(query), A.INS, np.uint8)
    if len(query) == 0:
        return np.full(len(refr), A.DEL, np.uint8)
    ops, d, start, end = align(refr, query, INFIX, FREE_READ)
    return np.concatenate([np.full(start, A.INS, np.uint8), ops, np.full(len(query) - end, A.INS, np.uint8)])
