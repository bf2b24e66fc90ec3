"""An independent reference of the pair-HMM, written from the prose of DESIGN section 4 and the header of oracle/model_fit.c.

It shares nothing with oracle/phmm.c or the HIP kernels but the specification.  Every probability is a float64 natural log and
every sum is np.logaddexp: there are no 64-diagonal exponents, no fma order, no row-crossing accumulators.  A banded sweep is
stored as (T + 1) x W arrays: row t is anti-diagonal t = i + j, column w is template coordinate i = base[t] + w, and every cell
outside the band or outside the matrix holds -inf.  The forward and backward recursions loop over anti-diagonals (a few numpy
calls each); the modification table and the expected counts are single vectorised passes over the whole band.

  forward   F_M(i,j) = eM[x[i-1]][y[j-1]] toM(i-1,j-1)   F_I(i,j) = eI[ctx(j)][y[j-1]] toI(i,j-1)   F_D(i,j) = toD(i-1,j)
            toS = F_M a_MS + F_I a_IS + F_D a_DS;   F_M(0,0) = 1;   lk = F_M + F_I + F_D at (L,n)
  backward  b_S(L,n) = 1;   b_S(i,j) = a_SM hatM(i+1,j+1) + a_SI hatI(i,j+1) + a_SD b_D(i+1,j)
            hatM(i,j) = eM[x[i-1]][y[j-1]] b_M(i,j),   hatI(i,j) = eI[ctx(j)][y[j-1]] b_I(i,j)
  ctx(j)    the read base before y[j-1], 4 for j = 1
  band      |i - c[t]| <= r, c[t] the ops path's i on diagonal t (a Match step: i + 1 on both of its diagonals)
  table     V(i1,i2,b) = sum_j toM(i1,j) eM[b][y[j]] b_M(i2,j+1) + toD(i1,j) b_D(i2,j)
  counts    S->M: F_S a_SM hatM(i+1,j+1)   S->I: F_S a_SI hatI(i,j+1)   S->D: F_S a_SD b_D(i+1,j)
            mat_emit[x[i-1]][y[j-1]]: F_M b_M   ins_emit[ctx(j)][y[j-1]]: F_I b_I   (each / lk)
"""
import numpy as np

NEG = -np.inf
SENTINEL = -1.0e300            # the oracle's JO_LOG_ZERO: an edit no path reaches
NUM_ROW = 14
OP_MATCH, OP_MISMATCH, OP_INS, OP_DEL = 0, 1, 2, 3   # enum jtk_op
TRANS = ("mat_mat", "mat_ins", "mat_del", "ins_mat", "ins_ins", "ins_del", "del_mat", "del_ins", "del_del")

_CODE = np.zeros(256, dtype=np.int64)
for _k, _b in enumerate(b"ACGT"):
    _CODE[_b] = _k
    _CODE[_b + 32] = _k


def codes(s):
    """ASCII bases -> 0..3 (anything else reads as A, like the oracle's base_code)"""
    return _CODE[np.asarray(s, dtype=np.uint8)]


class Model:
    """a pair-HMM in probability space: trans[from][to] over (M, I, D), mat[4][4] = eM, ins[5][4] = eI"""

    def __init__(self, trans, mat, ins):
        self.trans = np.array(trans, dtype=np.float64).reshape(3, 3)
        self.mat = np.array(mat, dtype=np.float64).reshape(4, 4)
        self.ins = np.array(ins, dtype=np.float64).reshape(5, 4)
        with np.errstate(divide="ignore"):
            self.la, self.lm, self.li = np.log(self.trans), np.log(self.mat), np.log(self.ins)

    @classmethod
    def of(cls, h):
        """from a jtk_hmm_t ctypes structure"""
        return cls([getattr(h, f) for f in TRANS], list(h.mat_emit), list(h.ins_emit))

    def fill(self, h):
        """write into a jtk_hmm_t ctypes structure; returns it"""
        for f, v in zip(TRANS, self.trans.ravel()):
            setattr(h, f, float(v))
        for k, v in enumerate(self.mat.ravel()):
            h.mat_emit[k] = float(v)
        for k, v in enumerate(self.ins.ravel()):
            h.ins_emit[k] = float(v)
        return h

    def flat(self):
        return np.concatenate([self.trans.ravel(), self.mat.ravel(), self.ins.ravel()])


def default_model():
    """HMMParam::default(): 0.97 / 0.01 / 0.01 rows, 0.97 on the emission diagonal, uniform insertions"""
    trans = [[0.97, 0.01, 0.01]] * 3
    return Model(trans, np.where(np.eye(4) > 0, 0.97, 0.01), np.full((5, 4), 0.25))


def random_model(rng, zero=None):
    """every row drawn at random (rows sum to one, no entry tiny); zero = (table, row, col) sets one entry to 0 and renormalises"""
    tr = np.empty((3, 3))
    tr[0] = rng.dirichlet([30.0, 2.0, 2.0])
    tr[1] = rng.dirichlet([10.0, 4.0, 2.0])
    tr[2] = rng.dirichlet([10.0, 2.0, 4.0])
    mat = np.array([rng.dirichlet(np.where(np.arange(4) == k, 40.0, 1.5)) for k in range(4)])
    ins = rng.dirichlet([3.0] * 4, 5)
    if zero is not None:
        which, r, c = zero
        arr = {"trans": tr, "mat": mat, "ins": ins}[which]
        arr[r, c] = 0.0
        arr[r] /= arr[r].sum()
    return Model(tr, mat, ins)


def band_centers(ops, L, n):
    """c[t] for t = 0..L+n: the template coordinate of the ops path on anti-diagonal t.  A Match / Mismatch step from (i, j)
    crosses diagonals t+1 and t+2 and puts i + 1 on both; a Del step puts i + 1 on t + 1, an Ins step i.  ValueError when
    the ops do not walk from (0, 0) to (L, n)."""
    c, i, j = [0], 0, 0
    for op in np.asarray(ops).tolist():
        if op in (OP_MATCH, OP_MISMATCH):
            c += [i + 1, i + 1]
            i, j = i + 1, j + 1
        elif op == OP_DEL:
            c.append(i + 1)
            i += 1
        elif op == OP_INS:
            c.append(i)
            j += 1
        else:
            raise ValueError("op %r" % op)
    if (i, j) != (L, n) or len(c) != L + n + 1:
        raise ValueError("ops walk to (%d, %d), not (%d, %d)" % (i, j, L, n))
    return np.array(c, dtype=np.int64)


class Band:
    """the cells of one sweep: diagonal t holds template coordinates base[t] .. base[t] + W - 1; `valid` marks the cells that are
    inside the matrix and inside the band"""

    def __init__(self, L, n, base, W, radius=None, centers=None):
        self.L, self.n, self.T, self.W = L, n, L + n, W
        self.base = np.asarray(base, dtype=np.int64)
        self.I = self.base[:, None] + np.arange(W)[None, :]
        self.J = np.arange(self.T + 1)[:, None] - self.I
        self.valid = (self.I >= 0) & (self.I <= L) & (self.J >= 0) & (self.J <= n)
        if radius is not None:
            self.valid &= np.abs(self.I - np.asarray(centers)[:, None]) <= radius

    def at(self, arr, t, i):
        """values of arr on diagonal t at template coordinates i (a vector); -inf where there is no cell"""
        if t < 0 or t > self.T:
            return np.full(np.shape(i), NEG)
        col = i - self.base[t]
        ok = (col >= 0) & (col < self.W)
        return np.where(ok, arr[t, np.clip(col, 0, self.W - 1)], NEG)

    def shifted(self, arr, dt, di):
        """for every cell (t, i) of the band: arr at diagonal t + dt, coordinate i + di (-inf where there is no cell)"""
        t = np.arange(self.T + 1) + dt
        ok_t = (t >= 0) & (t <= self.T)
        tc = np.clip(t, 0, self.T)
        col = self.I + di - self.base[tc][:, None]
        ok = ok_t[:, None] & (col >= 0) & (col < self.W)
        return np.where(ok, arr[tc[:, None], np.clip(col, 0, self.W - 1)], NEG)


def banded(L, n, ops, radius):
    c = band_centers(ops, L, n)
    return Band(L, n, c - radius, 2 * radius + 1, radius, c)


def unbanded(L, n):
    return Band(L, n, np.zeros(L + n + 1, dtype=np.int64), L + 1)


def _lae3(a, b, c):
    return np.logaddexp(np.logaddexp(a, b), c)


class Sweep:
    """forward (and on demand backward) log values of one read against one template on one band"""

    def __init__(self, model, tmpl, read, band, backward=True):
        self.m, self.b = model, band
        self.x, self.y = codes(tmpl), codes(read)
        L, n, T = band.L, band.n, band.T
        assert len(self.x) == L and len(self.y) == n
        # ctx(j) for j = 1..n (index j), eI[ctx(j)][y[j-1]] and its index in ins_emit
        self.ctx = np.full(n + 2, 4, dtype=np.int64)
        self.ctx[2:n + 2] = self.y[:n]
        self.yj = np.zeros(n + 2, dtype=np.int64)          # y[j-1] at index j
        self.yj[1:n + 1] = self.y
        self.xi = np.zeros(L + 2, dtype=np.int64)          # x[i-1] at index i
        self.xi[1:L + 1] = self.x
        self._forward()
        if backward:
            self._backward()

    def _emit_m(self, i, j):
        """log eM[x[i-1]][y[j-1]] (meaningful where 1 <= i <= L, 1 <= j <= n)"""
        L, n = self.b.L, self.b.n
        return self.m.lm[self.xi[np.clip(i, 0, L + 1)], self.yj[np.clip(j, 0, n + 1)]]

    def _emit_i(self, j):
        """log eI[ctx(j)][y[j-1]] (meaningful where 1 <= j <= n)"""
        jj = np.clip(j, 0, self.b.n + 1)
        return self.m.li[self.ctx[jj], self.yj[jj]]

    def _forward(self):
        b, la = self.b, self.m.la
        shape = (b.T + 1, b.W)
        self.FM, self.FI, self.FD = np.full(shape, NEG), np.full(shape, NEG), np.full(shape, NEG)
        self.toM, self.toI, self.toD = np.full(shape, NEG), np.full(shape, NEG), np.full(shape, NEG)
        for t in range(b.T + 1):
            i, j, v = b.I[t], b.J[t], b.valid[t]
            if t == 0:
                self.FM[0] = np.where(v & (i == 0), 0.0, NEG)
            else:
                self.FM[t] = np.where(v & (i >= 1) & (j >= 1), self._emit_m(i, j) + b.at(self.toM, t - 2, i - 1), NEG)
                self.FI[t] = np.where(v & (j >= 1), self._emit_i(j) + b.at(self.toI, t - 1, i), NEG)
                self.FD[t] = np.where(v & (i >= 1), b.at(self.toD, t - 1, i - 1), NEG)
            fm, fi, fd = self.FM[t], self.FI[t], self.FD[t]
            self.toM[t] = _lae3(fm + la[0, 0], fi + la[1, 0], fd + la[2, 0])
            self.toI[t] = _lae3(fm + la[0, 1], fi + la[1, 1], fd + la[2, 1])
            self.toD[t] = _lae3(fm + la[0, 2], fi + la[1, 2], fd + la[2, 2])
        end = np.array([b.L])
        self.lk = float(_lae3(b.at(self.FM, b.T, end), b.at(self.FI, b.T, end), b.at(self.FD, b.T, end))[0])

    def _backward(self):
        b, la = self.b, self.m.la
        shape = (b.T + 1, b.W)
        self.bM, self.bI, self.bD = np.full(shape, NEG), np.full(shape, NEG), np.full(shape, NEG)
        for t in range(b.T, -1, -1):
            i, j, v = b.I[t], b.J[t], b.valid[t]
            if t == b.T:
                end = np.where(v & (i == b.L), 0.0, NEG)
                self.bM[t], self.bI[t], self.bD[t] = end, end.copy(), end.copy()
                continue
            hm = self._emit_m(i + 1, j + 1) + b.at(self.bM, t + 2, i + 1)     # hatM(i+1, j+1)
            hi = self._emit_i(j + 1) + b.at(self.bI, t + 1, i)                 # hatI(i, j+1)
            nd = b.at(self.bD, t + 1, i + 1)                                   # b_D(i+1, j)
            for S, arr in enumerate((self.bM, self.bI, self.bD)):
                arr[t] = np.where(v, _lae3(la[S, 0] + hm, la[S, 1] + hi, la[S, 2] + nd), NEG)

    # ---- the modification table
    def table(self):
        """the 14 x (L + 1) table of log V (the sentinel where V = 0), rows 0-3 sub, 4-7 ins, 8-10 copy 1-3, 11-13 del 1-3:
        sub b@p = V(p, p+1, b), ins b@p = V(p, p, b), copy c@p = V(p+c, p+1, x[p]), del d@p = V(p, p+d+1, x[p+d])"""
        b, L, n = self.b, self.b.L, self.b.n
        I, J = b.I, b.J
        yj = np.clip(J, 0, n - 1) if n else np.zeros_like(J)
        ycode = self.y[yj] if n else np.zeros_like(J)
        has_y = J < n                                     # the M term emits y[j]

        def crossing(di, base_of):
            """V(i1, i2, base) over all forward cells (t, i1 = I): M term toM(i1,j) eM[base][y[j]] b_M(i2, j+1), D term toD(i1,j)
            b_D(i2,j), i2 = i1 + di"""
            mt = self.toM + np.where(has_y, self.m.lm[base_of, ycode], NEG) + b.shifted(self.bM, di + 1, di)
            dt = self.toD + b.shifted(self.bD, di, di)
            return np.logaddexp(mt, dt)

        out = np.full((L + 1, NUM_ROW), NEG)

        def put(row, keys, vals):
            ok = b.valid & (keys >= 0) & (keys <= L) & np.isfinite(vals)
            out[:, row] = _group_lse(keys[ok], vals[ok], L + 1)

        for base in range(4):
            put(base, I, crossing(1, np.full_like(I, base)))           # sub: i1 = p, i2 = p + 1
            put(4 + base, I, crossing(0, np.full_like(I, base)))       # ins: i1 = i2 = p
        xs = np.zeros(L + 4, dtype=np.int64)
        xs[:L] = self.x
        for c in (1, 2, 3):                                                  # copy: i1 = p + c, i2 = p + 1
            p = I - c
            put(7 + c, p, crossing(1 - c, xs[np.clip(p, 0, L + 3)]))
        for d in (1, 2, 3):                                                  # del: i1 = p, i2 = p + d + 1
            put(10 + d, I, crossing(d + 1, xs[np.clip(I + d, 0, L + 3)]))
        return np.where(np.isfinite(out), out, SENTINEL)

    # ---- expected counts
    def counts(self):
        """45 expected counts (9 transitions [from M, I, D][to M, I, D], 16 mat_emit, 20 ins_emit) of this read"""
        b, la, lk = self.b, self.m.la, self.lk
        cnt = np.zeros(45)
        if not np.isfinite(lk):
            return cnt
        I, J, v = b.I, b.J, b.valid
        hm = self._emit_m(I + 1, J + 1) + b.shifted(self.bM, 2, 1)        # hatM(i+1, j+1)
        hi = self._emit_i(J + 1) + b.shifted(self.bI, 1, 0)                # hatI(i, j+1)
        nd = b.shifted(self.bD, 1, 1)                                      # b_D(i+1, j)
        for S, F in enumerate((self.FM, self.FI, self.FD)):
            for q, nxt in enumerate((hm, hi, nd)):
                w = np.where(v, F + la[S, q] + nxt - lk, NEG)
                cnt[3 * S + q] = np.exp(w).sum()
        em = np.where(v & (I >= 1) & (J >= 1), self.FM + self.bM - lk, NEG)
        key = 4 * self.xi[np.clip(I, 0, b.L + 1)] + self.yj[np.clip(J, 0, b.n + 1)]
        cnt[9:25] = np.bincount(key.ravel(), weights=np.exp(em).ravel(), minlength=16)[:16]
        ei = np.where(v & (J >= 1), self.FI + self.bI - lk, NEG)
        jj = np.clip(J, 0, b.n + 1)
        key = 4 * self.ctx[jj] + self.yj[jj]
        cnt[25:45] = np.bincount(key.ravel(), weights=np.exp(ei).ravel(), minlength=20)[:20]
        return cnt


def _group_lse(keys, vals, size):
    """log of the sum of exp(vals) per key (-inf for a key without terms)"""
    m = np.full(size, NEG)
    np.maximum.at(m, keys, vals)
    s = np.bincount(keys, weights=np.exp(vals - m[keys]), minlength=size)
    with np.errstate(divide="ignore"):
        return np.where(s > 0, m + np.log(s), NEG)


def likelihood(model, tmpl, read, ops, radius):
    """banded log-likelihood (-inf when no path)"""
    return Sweep(model, tmpl, read, banded(len(tmpl), len(read), ops, radius), backward=False).lk


def likelihood_unbanded(model, tmpl, read):
    """log P(read | tmpl) over every alignment"""
    return Sweep(model, tmpl, read, unbanded(len(tmpl), len(read)), backward=False).lk


def modification_table(model, tmpl, read, ops, radius):
    """(table [L + 1, 14] of log V, the sentinel for impossible edits; lk)"""
    s = Sweep(model, tmpl, read, banded(len(tmpl), len(read), ops, radius))
    return s.table(), s.lk


def edited(tmpl, p, row):
    """the template of table entry (p, row), or None where the edit does not exist"""
    tmpl = np.asarray(tmpl, dtype=np.uint8)
    L = len(tmpl)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    if row < 4:
        return None if p >= L else np.concatenate([tmpl[:p], acgt[row:row + 1], tmpl[p + 1:]])
    if row < 8:
        return np.concatenate([tmpl[:p], acgt[row - 4:row - 3], tmpl[p:]])
    if row < 11:
        c = row - 7
        return None if p + c > L else np.concatenate([tmpl[:p + c], tmpl[p:]])
    d = row - 10
    return None if p + d >= L else np.concatenate([tmpl[:p], tmpl[p + d:]])


def counts(model, tmpl, read, ops, radius):
    """(45 expected counts, lk) of one read on the banded sweep"""
    s = Sweep(model, tmpl, read, banded(len(tmpl), len(read), ops, radius))
    return s.counts(), s.lk


def mstep(old, cnt):
    """every transition / mat_emit / ins_emit row divided by its sum; a row whose sum is not positive keeps the old values"""
    cnt = np.asarray(cnt, dtype=np.float64)
    rows = []
    for new_rows, old_rows in ((cnt[:9].reshape(3, 3), old.trans), (cnt[9:25].reshape(4, 4), old.mat),
                               (cnt[25:45].reshape(5, 4), old.ins)):
        s = new_rows.sum(axis=1, keepdims=True)
        rows.append(np.where(s > 0, new_rows / np.where(s > 0, s, 1.0), old_rows))
    return Model(*rows)


def fit_step(forward, reverse, packs, radius):
    """one Baum-Welch step on both strands (model_tune.rs:144-151): every read's counts under its strand's model (strand != 0:
    forward), pooled per strand over all pile-ups, then the M-step of each strand.  packs: [(tmpl, reads, ops, strands)]."""
    pooled = [np.zeros(45), np.zeros(45)]
    for tmpl, reads, opss, strands in packs:
        for rd, op, st in zip(reads, opss, strands):
            c, _ = counts(forward if st else reverse, tmpl, rd, op, radius)
            pooled[0 if st else 1] += c
    return mstep(forward, pooled[0]), mstep(reverse, pooled[1]), pooled


# ---- a 50-digit evaluation of the same quantities (unbanded, plain loops): bounds the float64 reference's own error

def mp_forward_backward(model, tmpl, read, digits=50):
    """(lk, 45 counts) as mpmath numbers, every alignment, for templates and reads of a few tens of bases"""
    import mpmath
    with mpmath.workdps(digits):
        return _mp_forward_backward(mpmath, model, tmpl, read)


def _mp_forward_backward(mpmath, model, tmpl, read):
    f = mpmath.mpf
    a = [[f(float(v)) for v in r] for r in model.trans]
    eM = [[f(float(v)) for v in r] for r in model.mat]
    eI = [[f(float(v)) for v in r] for r in model.ins]
    x, y = codes(tmpl).tolist(), codes(read).tolist()
    L, n = len(x), len(y)
    ctx = lambda j: y[j - 2] if j >= 2 else 4
    Z = f(0)
    F = [[[Z, Z, Z] for _ in range(n + 1)] for _ in range(L + 1)]
    F[0][0][0] = f(1)
    to = lambda c, q: c[0] * a[0][q] + c[1] * a[1][q] + c[2] * a[2][q]
    for i in range(L + 1):
        for j in range(n + 1):
            if i == 0 and j == 0:
                continue
            F[i][j][0] = eM[x[i - 1]][y[j - 1]] * to(F[i - 1][j - 1], 0) if i >= 1 and j >= 1 else Z
            F[i][j][1] = eI[ctx(j)][y[j - 1]] * to(F[i][j - 1], 1) if j >= 1 else Z
            F[i][j][2] = to(F[i - 1][j], 2) if i >= 1 else Z
    B = [[[Z, Z, Z] for _ in range(n + 2)] for _ in range(L + 2)]
    for i in range(L, -1, -1):
        for j in range(n, -1, -1):
            if i == L and j == n:
                B[i][j] = [f(1), f(1), f(1)]
                continue
            hm = eM[x[i]][y[j]] * B[i + 1][j + 1][0] if i < L and j < n else Z
            hi = eI[ctx(j + 1)][y[j]] * B[i][j + 1][1] if j < n else Z
            nd = B[i + 1][j][2] if i < L else Z
            B[i][j] = [a[S][0] * hm + a[S][1] * hi + a[S][2] * nd for S in range(3)]
    P = sum(F[L][n])
    cnt = [Z] * 45
    for i in range(L + 1):
        for j in range(n + 1):
            hm = eM[x[i]][y[j]] * B[i + 1][j + 1][0] if i < L and j < n else Z
            hi = eI[ctx(j + 1)][y[j]] * B[i][j + 1][1] if j < n else Z
            nd = B[i + 1][j][2] if i < L else Z
            for S in range(3):
                for q, nx in enumerate((hm, hi, nd)):
                    cnt[3 * S + q] += F[i][j][S] * a[S][q] * nx / P
            if i >= 1 and j >= 1:
                cnt[9 + 4 * x[i - 1] + y[j - 1]] += F[i][j][0] * B[i][j][0] / P
            if j >= 1:
                cnt[25 + 4 * ctx(j) + y[j - 1]] += F[i][j][1] * B[i][j][1] / P
    return mpmath.log(P), cnt


# ---- polishing, from the prose of DESIGN section 4 and the rule comment over select_edits in oracle/phmm.c
#
# Round t: column totals = sum over the first take_num reads of (table - lk); scan p = ignore_edge .. L - ignore_edge - 1 from the
# left; at p take the best row; if its total exceeds MIN_GAIN apply it and jump over the bases it touches (d for a deletion of d
# bases, one otherwise) plus inactive(t) = 5 + (5 t mod 21) further positions; a round that applies nothing is the last, and there
# are at most MAX_POLISH_ROUNDS.  The ops of every read follow the template: see rethread().
#
# Two rows at one position whose edited templates are byte-identical (insert tmpl[p] before p = copy 1 at p) have equal totals
# up to rounding and the same outcome, so rows are grouped by edited() and a decision is `decidable` when it does not hang on
# rounding: |best - MIN_GAIN| > tol, and every row of another group is below best - tol.

MIN_GAIN = 0.1
MAX_POLISH_ROUNDS = 20
DECISION_TOL = 1e-6


def inactive(t):
    return 5 + (5 * t) % 21


def column_totals(fwd, rev, tmpl, reads, opss, strands, radius, take_num):
    """[L, 14]: sum over the first min(take_num, n) reads of table - lk (strand != 0: forward model); an entry that is the
    sentinel for any read stays the sentinel"""
    L = len(tmpl)
    tot = np.zeros((L + 1, NUM_ROW))
    dead = np.zeros((L + 1, NUM_ROW), dtype=bool)
    for r in range(min(take_num, len(reads))):
        tab, lk = modification_table(fwd if strands[r] else rev, tmpl, reads[r], opss[r], radius)
        assert np.isfinite(lk), "read %d has no path inside the band" % r
        dead |= tab <= SENTINEL / 2
        tot += np.where(tab <= SENTINEL / 2, 0.0, tab - lk)
    return np.where(dead, SENTINEL, tot)[:L]


def _edit_span(row):
    return row - 10 if row >= 11 else 1


def select_edits(totals, ignore_edge, round, tmpl):
    """-> (edits [(pos, row)], log): the left-to-right scan of one round.  log holds one dict per scanned position: pos, row (the
    first best row), best, applied, gain_margin = |best - MIN_GAIN|, row_margin = best - the largest total among rows whose edited
    template differs from the best row's (inf when there is none), decidable"""
    L = len(tmpl)
    assert totals.shape == (L, NUM_ROW)
    edits, log = [], []
    pos = ignore_edge
    while pos + ignore_edge < L:
        t = totals[pos]
        row = int(np.argmax(t))                       # the first of equal maxima
        best = float(t[row])
        mine = edited(tmpl, pos, row)
        others = [float(t[q]) for q in range(NUM_ROW)
                  if q != row and (mine is None or edited(tmpl, pos, q) is None
                                   or bytes(edited(tmpl, pos, q)) != bytes(mine))]
        row_margin = best - max(others) if others else np.inf
        applied = best > MIN_GAIN
        assert not (applied and mine is None), "an edit that does not exist was selected"
        log.append(dict(round=round, pos=pos, row=row, best=best, applied=applied, gain_margin=abs(best - MIN_GAIN),
                        row_margin=row_margin,
                        decidable=abs(best - MIN_GAIN) > DECISION_TOL and row_margin > DECISION_TOL))
        if applied:
            edits.append((pos, row))
            pos += _edit_span(row) + inactive(round)
        else:
            pos += 1
    return edits, log


def apply_edits(tmpl, edits):
    """the template after every (pos, row) of one round, through edited(): applied from the right, so that the positions left of
    an edit keep their meaning"""
    out = np.asarray(tmpl, dtype=np.uint8)
    for pos, row in sorted(edits, reverse=True):
        out = edited(out, pos, row)
        assert out is not None, (pos, row)
    return out


def rethread(ops, L, edits, new_tmpl, read):
    """the ops of one read after the edits of one round.  The alignment is a list of columns (template index | None, read index |
    None).  A deleted template base leaves its column (the column goes when it held no read base); the k bases of an insertion /
    copy edit at pos are k read-less columns directly after the column of old base pos - 1 (at the very front for pos = 0);
    template indices are then renumbered and Match / Mismatch is tagged from the new template and the read."""
    cols, i, j = [], 0, 0
    for op in np.asarray(ops).tolist():
        if op == OP_INS:
            cols.append((None, j))
            j += 1
        elif op == OP_DEL:
            cols.append((i, None))
            i += 1
        else:
            cols.append((i, j))
            i, j = i + 1, j + 1
    assert i == L and j == len(read)
    gone, after = set(), {}
    for pos, row in edits:
        if row >= 11:
            gone.update(range(pos, pos + row - 10))
        elif row >= 8:
            after[pos - 1] = after.get(pos - 1, 0) + (row - 7)
        elif row >= 4:
            after[pos - 1] = after.get(pos - 1, 0) + 1
    new = [("new", None)] * after.pop(-1, 0)
    for ti, rj in cols:
        keep_t = ti is not None and ti not in gone
        if keep_t or rj is not None:
            new.append(("old" if keep_t else None, rj))
        if ti is not None and ti in after:
            assert ti not in gone
            new += [("new", None)] * after.pop(ti)
    assert not after, after
    out, i = [], 0
    for t, rj in new:
        if t is None:
            out.append(OP_INS)
        elif rj is None:
            out.append(OP_DEL)
            i += 1
        else:
            out.append(OP_MATCH if new_tmpl[i] == read[rj] else OP_MISMATCH)
            i += 1
    assert i == len(new_tmpl) and sum(1 for _, rj in new if rj is not None) == len(read)
    return np.array(out, dtype=np.uint8)


def polish(fwd, rev, tmpl, reads, opss, strands, radius, take_num, ignore_edge):
    """-> (consensus, ops of all reads, rounds, log).  rounds counts the round that applied nothing; log is the concatenation of
    every round's select_edits log."""
    cur = np.asarray(tmpl, dtype=np.uint8).copy()
    opss = [np.asarray(o, dtype=np.uint8).copy() for o in opss]
    log, rounds = [], 0
    for t in range(MAX_POLISH_ROUNDS):
        rounds = t + 1
        if 2 * ignore_edge >= len(cur):
            break                                      # nothing to scan: no need for the totals
        tot = column_totals(fwd, rev, cur, reads, opss, strands, radius, take_num)
        edits, lg = select_edits(tot, ignore_edge, t, cur)
        log += lg
        if not edits:
            break
        nxt = apply_edits(cur, edits)
        opss = [rethread(o, len(cur), edits, nxt, rd) for o, rd in zip(opss, reads)]
        cur = nxt
    return cur, opss, rounds, log
