"""An independent restatement of the guided polish of DESIGN.md section 4, "Guided polishing" (jtk_lc_polish_guided, gpolish.hip).

The polish is this repository's own specification of what kiley's `bialignment::guided::polish_until_converge(_with)` does for
the reference (kiley is not part of the reference tree): parity with kiley's polish is NOT pinned.

Structured unlike the kernel on purpose: the band is a dictionary of cells, F and B are both stored whole (a missing key is plus
infinity), every cell is filled from its neighbours one by one (no scan), and the table is written out by explicit loops over
positions, rows and columns.  The band, `edited`, `apply_edits`, `rethread` and `inactive` are those of the existing references.

x: the template (Del consumes a base of it); y: a read (Ins consumes a base of it).  Ops: 0 Match, 1 Mismatch, 2 Ins, 3 Del.
Sequences are uint8 arrays of ASCII bases.
"""
import functools

import numpy as np

from guided_reference import band_cells
from phmm_reference import apply_edits, edited, inactive, rethread

MATCH, MISMATCH, INS, DEL = 0, 1, 2, 3
INF = float("inf")
NUM_ROW = 14
DEAD = 0xFFFFFFFF            # a dead entry, as jtk_lc_debug_guided_table writes it
MAX_ROUNDS = 20
ACGT = b"ACGT"


def as_seq(s):
    if isinstance(s, (bytes, str)):
        s = np.frombuffer(s.encode() if isinstance(s, str) else s, dtype=np.uint8)
    return np.asarray(s, dtype=np.uint8)


def _ints(s):
    """plain Python integers: the loops below compare them millions of times"""
    return s.tolist() if hasattr(s, "tolist") else list(s)


def forward(x, y, band):
    x, y = _ints(x), _ints(y)
    n, m = len(x), len(y)
    F = {}
    for i in range(n + 1):
        for j in range(band[i][0], band[i][1] + 1):
            if i == 0 and j == 0:
                F[i, j] = 0
                continue
            best = INF
            if i > 0 and j > 0:
                best = min(best, F.get((i - 1, j - 1), INF) + (x[i - 1] != y[j - 1]))
            if i > 0:
                best = min(best, F.get((i - 1, j), INF) + 1)
            if j > 0:
                best = min(best, F.get((i, j - 1), INF) + 1)
            F[i, j] = best
    return F


def backward(x, y, band):
    x, y = _ints(x), _ints(y)
    n, m = len(x), len(y)
    B = {}
    for i in range(n, -1, -1):
        for j in range(band[i][1], band[i][0] - 1, -1):
            if i == n and j == m:
                B[i, j] = 0
                continue
            best = INF
            if i < n and j < m:
                best = min(best, B.get((i + 1, j + 1), INF) + (x[i] != y[j]))
            if i < n:
                best = min(best, B.get((i + 1, j), INF) + 1)
            if j < m:
                best = min(best, B.get((i, j + 1), INF) + 1)
            B[i, j] = best
    return B


def walk(F, x, y):
    """ops from (n, m) back to (0, 0): the first move that reproduces the value, in the order diagonal, Del, Ins"""
    x, y = _ints(x), _ints(y)
    i, j = len(x), len(y)
    ops = []
    while i > 0 or j > 0:
        v = F[i, j]
        if i > 0 and j > 0 and F.get((i - 1, j - 1), INF) + (x[i - 1] != y[j - 1]) == v:
            ops.append(MISMATCH if x[i - 1] != y[j - 1] else MATCH)
            i, j = i - 1, j - 1
        elif i > 0 and F.get((i - 1, j), INF) + 1 == v:
            ops.append(DEL)
            i -= 1
        else:
            assert j > 0 and F.get((i, j - 1), INF) + 1 == v
            ops.append(INS)
            j -= 1
    return np.array(ops[::-1], dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def exists(n, p, row):
    """whether edit (p, row) exists on a template of n bases: `edited` decides, asked once per (n, p, row)"""
    return edited(np.full(n, ACGT[0], dtype=np.uint8), p, row) is not None


def fill(x, y, guide, radius):
    """-> (dist, ops, F, band) of one read along its guide"""
    x, y = as_seq(x), as_seq(y)
    band = band_cells(len(x), len(y), np.asarray(guide).tolist(), radius)
    F = forward(x, y, band)
    dist = F[len(x), len(y)]
    assert dist < INF, "the guide's own path lies in the band"
    return int(dist), walk(F, x, y), F, band


def table(x, y, guide, radius):
    """-> (dist, T [n + 1, 14] as int64 with DEAD for a dead entry, ops)"""
    x, y = as_seq(x), as_seq(y)
    n, m = len(x), len(y)
    dist, ops, F, band = fill(x, y, guide, radius)
    B = backward(x, y, band)
    y = _ints(y)
    T = np.full((n + 1, NUM_ROW), DEAD, dtype=np.int64)
    for p in range(n + 1):
        cols = list(range(band[p][0], band[p][1] + 1))
        # the cells of F and B that the 14 entries of position p name, column by column
        Fr = [[F.get((p + k, j), INF) for j in cols] for k in range(4)]
        Br = [[B.get((p + k, j), INF) for j in cols] for k in range(4)]
        Bp_right = [B.get((p, j + 1), INF) for j in cols]
        Bn_right = [B.get((p + 1, j + 1), INF) for j in cols]
        for row in range(NUM_ROW):
            if not exists(n, p, row):
                continue
            best = INF
            for k, j in enumerate(cols):
                if row < 4:
                    if j < m:
                        best = min(best, Fr[0][k] + (ACGT[row] != y[j]) + Bn_right[k])
                    best = min(best, Fr[0][k] + 1 + Br[1][k])
                elif row < 8:
                    if j < m:
                        best = min(best, Fr[0][k] + (ACGT[row - 4] != y[j]) + Bp_right[k])
                    best = min(best, Fr[0][k] + 1 + Br[0][k])
                elif row < 11:
                    best = min(best, Fr[row - 7][k] + Br[0][k])
                else:
                    best = min(best, Fr[0][k] + Br[row - 10][k])
            if best < INF:
                T[p, row] = int(best)
    return dist, T, ops


def edit_distance(x, y):
    """the unbanded unit-cost distance (two rolling rows)"""
    x, y = as_seq(x), as_seq(y)
    prev = list(range(len(y) + 1))
    for i in range(1, len(x) + 1):
        cur = [i] + [0] * len(y)
        for j in range(1, len(y) + 1):
            cur[j] = min(prev[j - 1] + (x[i - 1] != y[j - 1]), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[len(y)]


def gains(x, reads, opss, radius, take_num):
    """-> (gain [n + 1, 14] int64, dead [n + 1, 14] bool, ops of every read, dist of every read)"""
    n = len(x)
    gain = np.zeros((n + 1, NUM_ROW), dtype=np.int64)
    dead = np.zeros((n + 1, NUM_ROW), dtype=bool)
    new_ops, dists = [], []
    voters = len(reads) if take_num == 0 else min(take_num, len(reads))
    for r, (rd, op) in enumerate(zip(reads, opss)):
        if r < voters:
            dist, T, ops = table(x, rd, op, radius)
            dead |= T == DEAD
            gain += np.where(T == DEAD, 0, dist - T)
        else:
            dist, ops, _, _ = fill(x, rd, op, radius)
        new_ops.append(ops)
        dists.append(dist)
    return gain, dead, new_ops, dists


def select(gain, dead, ignore_edge, t, n):
    """the left-to-right scan of round t -> [(pos, row)]"""
    edits = []
    pos = ignore_edge
    while pos + ignore_edge < n:
        best, row = None, None
        for q in range(NUM_ROW):
            if not dead[pos, q] and (best is None or gain[pos, q] > best):
                best, row = int(gain[pos, q]), q
        if best is not None and best >= 1:
            edits.append((pos, row))
            pos += (row - 10 if row >= 11 else 1) + inactive(t)
        else:
            pos += 1
    return edits


def polish(tmpl, reads, opss, radius, take_num=0, ignore_edge=0, max_rounds=0, log=None):
    """-> (consensus, ops of every read, dist of every read, rounds); log: a list that gets (t, n, gain, dead, edits) of every
    round that scanned"""
    cur = as_seq(tmpl).copy()
    reads = [as_seq(r) for r in reads]
    opss = [np.asarray(o, dtype=np.uint8).copy() for o in opss]
    dists = [None] * len(reads)
    rounds, stale = 0, True        # stale: ops and dists do not belong to `cur`
    for t in range(max_rounds if max_rounds else MAX_ROUNDS):
        rounds = t + 1
        if 2 * ignore_edge >= len(cur):
            break
        gain, dead, opss, dists = gains(cur, reads, opss, radius, take_num)
        stale = False
        edits = select(gain, dead, ignore_edge, t, len(cur))
        if log is not None:
            log.append((t, len(cur), gain, dead, list(edits)))
        if not edits:
            break
        nxt = apply_edits(cur, edits)
        opss = [rethread(o, len(cur), edits, nxt, rd) for o, rd in zip(opss, reads)]
        cur, stale = nxt, True
    if stale:
        filled = [fill(cur, rd, op, radius) for rd, op in zip(reads, opss)]
        opss, dists = [f[1] for f in filled], [f[0] for f in filled]
    return cur, opss, dists, rounds


def consumes(ops, x, y):
    """the ops consume both sequences whole and tell Match from Mismatch; -> the distance they spell"""
    x, y = as_seq(x), as_seq(y)
    i = j = d = 0
    for op in np.asarray(ops).tolist():
        if op in (MATCH, MISMATCH):
            assert (x[i] == y[j]) == (op == MATCH)
            d += op == MISMATCH
            i, j = i + 1, j + 1
        elif op == DEL:
            i, d = i + 1, d + 1
        else:
            assert op == INS
            j, d = j + 1, d + 1
    assert i == len(x) and j == len(y)
    return d


def global_ops(x, y):
    """unbanded unit-cost ops under the project's tie rule (the input a caller gets from jtk_lc_align_reads)"""
    x, y = as_seq(x), as_seq(y)
    return fill(x, y, [], len(x) + len(y) + 1)[1]
