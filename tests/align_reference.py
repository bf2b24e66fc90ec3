"""Independent numpy restatement of the global alignment of DESIGN.md section 4 (what jtk_lc_align_reads computes), written
from the text of the specification and sharing no code with the device or with oracle/phmm.c:

  D(i,0) = i, D(0,j) = j, D(i,j) = min(D(i-1,j-1) + [x[i-1] != y[j-1]], D(i-1,j) + 1, D(i,j-1) + 1);
  the ops are read off a walk from (tl, rl) back to (0, 0) that takes the first move reproducing D(i,j) in the order
  diagonal (Match where the bases agree, else Mismatch), Del (i-1, j), Ins (i, j-1), and are reported front to back.

The matrix is filled row by row; the insertion chain of a row is a running minimum of (value - column) + column."""
import numpy as np

MATCH, MISMATCH, INS, DEL = 0, 1, 2, 3
BIG = 1 << 28


def seq(s):
    return np.frombuffer(s.encode("ascii"), dtype=np.uint8) if isinstance(s, str) else np.asarray(s, dtype=np.uint8)


def band_of(tl, rl, t):
    """diagonals j - i the fill may touch for a distance bound t >= |rl - tl|"""
    delta = rl - tl
    e = (t - abs(delta)) // 2
    return min(delta, 0) - e, max(delta, 0) + e


def fill(x, y, band=None, dtype=np.int32):
    """(tl+1) x (rl+1) matrix; with band = (klo, khi) cells off those diagonals hold BIG and are never read as less"""
    x, y = seq(x), seq(y)
    tl, rl = len(x), len(y)
    cols = np.arange(rl + 1, dtype=np.int64)
    D = np.empty((tl + 1, rl + 1), dtype=dtype)
    cap = BIG if dtype == np.int32 else int(np.iinfo(dtype).max) // 2
    prev = cols.copy()
    if band is not None:
        prev[(cols - 0 < band[0]) | (cols - 0 > band[1])] = cap
    D[0] = prev
    for i in range(1, tl + 1):
        cur = np.full(rl + 1, cap, dtype=np.int64)
        cur[0] = i
        cur[1:] = np.minimum(prev[:-1] + (y != x[i - 1]), prev[1:] + 1)
        if band is not None:
            cur[(cols - i < band[0]) | (cols - i > band[1])] = cap
        cur = np.minimum(np.minimum.accumulate(cur - cols) + cols, cap)   # D(i,j-1) + 1 along the row
        if band is not None:
            cur[(cols - i < band[0]) | (cols - i > band[1])] = cap
        D[i] = cur
        prev = cur
    return D


def walk(D, x, y):
    x, y = seq(x), seq(y)
    i, j = len(x), len(y)
    out = []
    while i > 0 or j > 0:
        here = int(D[i, j])
        if i > 0 and j > 0 and here == int(D[i - 1, j - 1]) + (1 if x[i - 1] != y[j - 1] else 0):
            out.append(MATCH if x[i - 1] == y[j - 1] else MISMATCH)
            i -= 1
            j -= 1
        elif i > 0 and here == int(D[i - 1, j]) + 1:
            out.append(DEL)
            i -= 1
        else:
            out.append(INS)
            j -= 1
    return np.array(out[::-1], dtype=np.uint8)


def align(x, y, dtype=np.int32):
    """-> (ops, distance) of read y against template x on the full matrix"""
    D = fill(x, y, dtype=dtype)
    return walk(D, x, y), int(D[len(seq(x)), len(seq(y))])


def align_banded(x, y, t):
    """-> (ops or None, banded D(tl, rl)); the ops only when the band certifies them (value <= t)"""
    x, y = seq(x), seq(y)
    D = fill(x, y, band=band_of(len(x), len(y), t))
    d = int(D[len(x), len(y)])
    return (walk(D, x, y) if d <= t else None), d


# ---- sequences for the tests (CPU and GPU files share them)

def random_seq(rng, n, alphabet=4):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, alphabet, n)]


def mutate(rng, s, rate):
    """substitutions, insertions and deletions at `rate` per base, a third each"""
    out = []
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    for b in s:
        u = rng.random()
        if u < rate / 3:
            out.append(acgt[rng.integers(0, 4)])
        elif u < 2 * rate / 3:
            out.append(b)
            out.append(acgt[rng.integers(0, 4)])
        elif u < rate:
            continue
        else:
            out.append(b)
    return np.array(out, dtype=np.uint8)


def low_complexity(rng, n):
    """homopolymer runs and tandem repeats: ties abound"""
    out = []
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    while len(out) < n:
        unit = acgt[rng.integers(0, 4, rng.integers(1, 4))]
        out.extend(np.tile(unit, rng.integers(2, 9)).tolist())
    return np.array(out[:n], dtype=np.uint8)
