"""An independent restatement of the guided affine-gap aligner of DESIGN.md section 4 (jtk_lc_align_guided, guided.hip).

The aligner is this repository's own specification of what kiley's `bialignment::guided::global_guided` / `infix_guided` do
for the reference (kiley is not part of the reference tree): parity with kiley's band shape and tie-breaking is NOT pinned.

Structured unlike the kernel on purpose: the band is a set of cells, the three states live in one dictionary keyed by
(i, j), a missing key is minus infinity, I is filled cell by cell from its left neighbour (no scan), and the traceback
recomputes every predecessor from the table (no stored traceback bits).

x: the sequence whose ends may be free (Del consumes an x base); y: consumed whole (Ins consumes a y base).
Ops: 0 Match, 1 Mismatch, 2 Ins, 3 Del.
"""
MATCH, MISMATCH, INS, DEL = 0, 1, 2, 3
NEG = float("-inf")
ALN_PARAMETER = (2, -6, -5, -1)   # (match, mismatch, open, ext) of deletion_fill.rs


def guide_path(n, m, guide):
    """The cells of the guide's path from (0, 0) to (n, m): ops that do not fit are skipped, a short guide is extended
    diagonally, then by Del, then by Ins."""
    i = j = 0
    cells = [(0, 0)]
    for op in guide:
        if op in (MATCH, MISMATCH):
            if i < n and j < m:
                i, j = i + 1, j + 1
                cells.append((i, j))
        elif op == DEL:
            if i < n:
                i += 1
                cells.append((i, j))
        elif op == INS:
            if j < m:
                j += 1
                cells.append((i, j))
        else:
            raise ValueError("op code %r" % (op,))
    while i < n and j < m:
        i, j = i + 1, j + 1
        cells.append((i, j))
    while i < n:
        i += 1
        cells.append((i, j))
    while j < m:
        j += 1
        cells.append((i, j))
    return cells


def band_cells(n, m, guide, radius):
    """row -> (first column, last column) of the band"""
    lo, hi = {}, {}
    for i, j in guide_path(n, m, guide):
        lo[i] = min(lo.get(i, j), j)
        hi[i] = max(hi.get(i, j), j)
    return {i: (max(0, lo[i] - radius), min(m, hi[i] + radius)) for i in range(n + 1)}


def check_scores(scores):
    match, mismatch, gap_open, gap_ext = scores
    if not (gap_open <= gap_ext <= 0 and mismatch <= 0 <= match):
        raise ValueError("scores need open <= ext <= 0 and mismatch <= 0 <= match")


def align_guided(x, y, guide, radius, infix=False, scores=ALN_PARAMETER, trace=None):
    """-> dict(score, start, end, ops); x and y are sequences of comparable items (bytes, str, lists).
    trace: a dict that gets the band, the steps of the walk back as (state, i, j, state of the predecessor) with 0 = M, 1 = D,
    2 = I, the number of end rows that hold the best score and the number of states that hold it in the end cell"""
    check_scores(scores)
    match, mismatch, gap_open, gap_ext = scores
    n, m = len(x), len(y)
    band = band_cells(n, m, guide, radius)
    M, D, I = {}, {}, {}

    def get(t, i, j):
        return t.get((i, j), NEG)

    for i in range(n + 1):
        for j in range(band[i][0], band[i][1] + 1):
            if (i == 0 and j == 0) or (infix and j == 0):
                M[i, j] = 0
            elif i > 0 and j > 0:
                s = match if x[i - 1] == y[j - 1] else mismatch
                M[i, j] = max(get(M, i - 1, j - 1), get(D, i - 1, j - 1), get(I, i - 1, j - 1)) + s
            if i > 0:
                D[i, j] = max(get(M, i - 1, j) + gap_open, get(D, i - 1, j) + gap_ext, get(I, i - 1, j) + gap_open)
            if j > 0:
                I[i, j] = max(get(M, i, j - 1) + gap_open, get(D, i, j - 1) + gap_open, get(I, i, j - 1) + gap_ext)

    def best_of(i, j):
        return max(get(M, i, j), get(D, i, j), get(I, i, j))

    end = n
    if infix:
        rows = [i for i in range(n + 1) if band[i][1] == m]
        top = max(best_of(i, m) for i in rows)
        end = min(i for i in rows if best_of(i, m) == top)
    score = best_of(end, m)
    assert score > NEG, "the guide's own path lies in the band"
    tables = (M, D, I)
    state = [get(t, end, m) for t in tables].index(score)
    i, j = end, m
    ops = []
    steps = []
    if trace is not None:
        trace.update(band=band, steps=steps, tied_states=[get(t, end, m) for t in tables].count(score),
                     tied_end_rows=sum(best_of(r, m) == score for r in range(n + 1) if band[r][1] == m) if infix else 1)
    while True:
        at = (state, i, j)
        if state == 0:
            if j == 0 and (infix or i == 0):
                break
            value = get(M, i, j) - (match if x[i - 1] == y[j - 1] else mismatch)
            ops.append(MATCH if x[i - 1] == y[j - 1] else MISMATCH)
            i, j = i - 1, j - 1
            cand = [get(t, i, j) for t in tables]
        elif state == 1:
            value = get(D, i, j)
            ops.append(DEL)
            i -= 1
            cand = [get(M, i, j) + gap_open, get(D, i, j) + gap_ext, get(I, i, j) + gap_open]
        else:
            value = get(I, i, j)
            ops.append(INS)
            j -= 1
            cand = [get(M, i, j) + gap_open, get(D, i, j) + gap_open, get(I, i, j) + gap_ext]
        state = cand.index(value)
        steps.append(at + (state,))
    start = i
    ops = [DEL] * start + ops[::-1] + [DEL] * (n - end)
    return dict(score=int(score), start=start, end=end, ops=ops)


def score_of_ops(x, y, ops, start, end, scores=ALN_PARAMETER):
    """The score the ops spell, the free runs (start leading and len(x) - end trailing Dels) excluded; checks on the way that
    the ops consume both sequences whole and tell matches from mismatches."""
    match, mismatch, gap_open, gap_ext = scores
    n = len(x)
    assert all(op == DEL for op in ops[:start]) and all(op == DEL for op in ops[len(ops) - (n - end):])
    core = ops[start:len(ops) - (n - end)]
    i, j, total, prev = start, 0, 0, None
    for op in core:
        if op in (MATCH, MISMATCH):
            assert (x[i] == y[j]) == (op == MATCH)
            total += match if op == MATCH else mismatch
            i, j = i + 1, j + 1
        elif op == DEL:
            total += gap_ext if prev == DEL else gap_open
            i += 1
        else:
            assert op == INS
            total += gap_ext if prev == INS else gap_open
            j += 1
        prev = op
    assert i == end and j == len(y)
    return total


def unbanded(x, y, infix=False, scores=ALN_PARAMETER):
    """The best score of the three-state recurrence without a band (two rolling rows; no traceback)."""
    match, mismatch, gap_open, gap_ext = scores
    n, m = len(x), len(y)
    best = NEG
    prev = None
    for i in range(n + 1):
        row = [[NEG, NEG, NEG] for _ in range(m + 1)]
        for j in range(m + 1):
            c = row[j]
            if (i == 0 and j == 0) or (infix and j == 0):
                c[0] = 0
            elif i > 0 and j > 0:
                c[0] = max(prev[j - 1]) + (match if x[i - 1] == y[j - 1] else mismatch)
            if i > 0:
                u = prev[j]
                c[1] = max(u[0] + gap_open, u[1] + gap_ext, u[2] + gap_open)
            if j > 0:
                l = row[j - 1]
                c[2] = max(l[0] + gap_open, l[1] + gap_open, l[2] + gap_ext)
        if infix or i == n:
            best = max(best, max(row[m]))
        prev = row
    return int(best)
