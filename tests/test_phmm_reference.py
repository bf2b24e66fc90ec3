"""The oracle's pair-HMM (oracle/phmm.c, oracle/model_fit.c) against tests/phmm_reference.py, a log-space restatement written
from DESIGN section 4 and the model_fit.c header.  The GPU suite pins the kernels to the oracle bit for bit; these tests pin the
oracle to the specification, at the shapes where a band, a scaling block or a context bug carries probability mass: radii 1-8 on
reads with 10-15 % errors and indel runs, T = L + n at the edges of the 8- and 64-diagonal blocks, reads much longer or shorter
than their template, ops that open or close with an indel run, homopolymers, and forward / reverse models that differ."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_ffi as O
import phmm_reference as R

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


# ---- inputs

def noisy_read(rng, tmpl, err, run_rate=0.0, lead=(), tail=()):
    """a read of `tmpl` (ASCII) with substitutions, single insertions and deletions at `err` in all, indel runs of 3-6 bases at
    `run_rate` per template base, and (op, k) runs before the first / after the last template base; -> (read, ops)"""
    L = len(tmpl)
    read, ops = [], []

    def run(op, k, i):
        if op == R.OP_INS:
            read.extend(ACGT[rng.integers(0, 4, k)].tolist())
            ops.extend([R.OP_INS] * k)
            return i
        k = min(k, L - i)
        ops.extend([R.OP_DEL] * k)
        return i + k

    i = 0
    for op, k in lead:
        i = run(op, k, i)
    end = L - sum(k for op, k in tail if op == R.OP_DEL)
    while i < end:
        u = rng.random()
        if u < run_rate:
            i = run(R.OP_INS if rng.random() < 0.5 else R.OP_DEL, int(rng.integers(3, 7)), i) if end - i > 6 else i
            if i >= end:
                break
        u = rng.random()
        if u < err / 3:                                     # deletion
            ops.append(R.OP_DEL)
            i += 1
            continue
        if u < 2 * err / 3:                                 # insertion before the base
            read.append(int(ACGT[rng.integers(0, 4)]))
            ops.append(R.OP_INS)
        b = int(tmpl[i])
        if 2 * err / 3 <= u < err:                          # substitution
            b = int(ACGT[(list(ACGT).index(b) + rng.integers(1, 4)) % 4])
        read.append(b)
        ops.append(R.OP_MATCH if b == tmpl[i] else R.OP_MISMATCH)
        i += 1
    for op, k in tail:
        i = run(op, k, i)
    return np.array(read, dtype=np.uint8), np.array(ops, dtype=np.uint8)


def shaped_read(rng, tmpl, n, err):
    """a read of exactly n bases: min(L, n) - k Match / Mismatch columns (k <= 2), the remaining Ins and Del columns placed at
    random, in runs where there are several; substitutions at `err`"""
    L = len(tmpl)
    m = max(min(L, n) - int(rng.integers(0, 3)), 0)
    cols = [R.OP_MATCH] * m + [R.OP_DEL] * (L - m) + [R.OP_INS] * (n - m)
    ops = np.array(cols, dtype=np.uint8)[rng.permutation(len(cols))]
    read, i = [], 0
    for k, op in enumerate(ops.tolist()):
        if op == R.OP_INS:
            read.append(int(ACGT[rng.integers(0, 4)]))
        elif op == R.OP_DEL:
            i += 1
        else:
            b = int(tmpl[i]) if rng.random() >= err else int(ACGT[rng.integers(0, 4)])
            read.append(b)
            ops[k] = R.OP_MATCH if b == tmpl[i] else R.OP_MISMATCH
            i += 1
    return np.array(read, dtype=np.uint8), ops


def random_tmpl(rng, L):
    return ACGT[rng.integers(0, 4, L)].copy()


def homopolymer_tmpl(rng, L):
    """runs of 1-7 equal bases"""
    out = []
    while len(out) < L:
        out += [int(ACGT[rng.integers(0, 4)])] * int(rng.integers(1, 8))
    return np.array(out[:L], dtype=np.uint8)


def models():
    """the default model; distinct forward / reverse models with random rows; a model whose Del row holds a zero (a_DI = 0)"""
    rng = np.random.default_rng(2024)
    return {"default": (R.default_model(), R.default_model()),
            "asym": (R.random_model(rng), R.random_model(rng)),
            "zero": (R.random_model(rng, zero=("trans", 2, 1)), R.random_model(rng, zero=("mat", 1, 2)))}


def params_of(fwd, rev, tmpl_len, radius):
    """oracle params whose band_width_of(band_frac, tmpl_len) / 2 is `radius` (mod.rs:96,112)"""
    p = O.Params()
    fwd.fill(p.forward)
    rev.fill(p.reverse)
    p.band_frac = (2 * radius + 0.5) / tmpl_len
    p.haploid_coverage = 10.0
    assert int(np.ceil(tmpl_len * p.band_frac)) // 2 == radius
    return p


def oracle_pileup_table(p, tmpl, reads, opss, strands):
    """jo_modification_table: (table - lk [n, L + 1, 14], lk [n]); the model follows each read's strand"""
    n = len(reads)
    ro = np.zeros(n + 1, np.uint64)
    oo = np.zeros(n + 1, np.uint64)
    ro[1:] = np.cumsum([len(r) for r in reads])
    oo[1:] = np.cumsum([len(o) for o in opss])
    rb = np.concatenate(reads).astype(np.uint8)
    ob = np.concatenate(opss).astype(np.uint8)
    tab = np.zeros((n, R.NUM_ROW * (len(tmpl) + 1)))
    lk = np.zeros(n)
    O.lib().jo_modification_table(C.byref(p), O.u8p(tmpl), len(tmpl), n, O.u8p(rb), O.u64p(ro), O.u8p(ob), O.u64p(oo),
                                  O.u8p(np.array(strands, np.uint8)), O.f64p(tab), O.f64p(lk))
    return tab.reshape(n, len(tmpl) + 1, R.NUM_ROW), lk


def oracle_counts(model, tmpl, read, ops, radius):
    h = model.fill(O.Hmm())
    cnt = np.zeros(45)
    lk = O.lib().jo_phmm_counts(C.byref(h), O.u8p(tmpl), len(tmpl), O.u8p(read), len(read), O.u8p(ops), len(ops), radius,
                                O.f64p(cnt))
    return cnt, lk


def oracle_centers(ops, L, n):
    c = np.zeros(L + n + 1, dtype=np.uint32)
    rc = O.lib().jo_band_centers(O.u8p(np.ascontiguousarray(ops, np.uint8)), len(ops), L, n, O.u32p(c))
    return rc, c.astype(np.int64)


# ---- comparisons (the tolerances of the issue that asked for this file: lk 1e-11 relative, table - lk 1e-8, counts 1e-9)

LK_RTOL = 1e-11   # (tests/test_gains_reference.py and tests/test_gpu_gains_reference.py take the bound on lk from here)


def assert_table_matches(ref_tab, ref_lk, tab_minus_lk, lk, where=""):
    """ref_tab: log V [L + 1, 14] (sentinel for impossible edits); tab_minus_lk: the oracle's or the device's table - lk"""
    assert abs(lk - ref_lk) <= LK_RTOL * abs(ref_lk), (where, lk, ref_lk)
    fin = ref_tab > -1e299
    assert np.array_equal(fin, tab_minus_lk > -1e299), (where, np.argwhere(fin != (tab_minus_lk > -1e299))[:5])
    err = np.abs(tab_minus_lk[fin] - (ref_tab[fin] - ref_lk))
    assert err.max(initial=0.0) < 1e-8, (where, err.max(), np.argwhere(np.abs(np.where(fin, tab_minus_lk - ref_tab + ref_lk, 0))
                                                                     >= 1e-8)[:5])


def assert_counts_match(ref, got, rtol=1e-9, where=""):
    ref, got = np.asarray(ref), np.asarray(got)
    assert np.array_equal(ref > 0, got > 0), (where, ref, got)
    rel = np.abs(got - ref) / np.where(ref > 0, ref, 1.0)
    assert rel.max() <= rtol, (where, int(rel.argmax()), rel.max())


def check_read(m, tmpl, read, ops, radius, where=""):
    """one read through the oracle's single-read entries under model m: band centres, lk, table, counts"""
    L, n = len(tmpl), len(read)
    rc, c = oracle_centers(ops, L, n)
    assert rc == 0 and np.array_equal(c, R.band_centers(ops, L, n)), where
    ref_tab, ref_lk = R.modification_table(m, tmpl, read, ops, radius)
    h = m.fill(O.Hmm())
    otab, olk = O.modification_table(h, tmpl, read, ops, radius)
    assert O.likelihood(h, tmpl, read, ops, radius) == olk
    assert_table_matches(ref_tab, ref_lk, otab.reshape(L + 1, R.NUM_ROW) - olk, olk, where)
    ocnt, clk = oracle_counts(m, tmpl, read, ops, radius)
    assert clk == olk
    rcnt, _ = R.counts(m, tmpl, read, ops, radius)
    assert_counts_match(rcnt, ocnt, where=where)
    return ref_lk


# ---- the reference itself

def test_reference_agrees_with_a_50_digit_evaluation():
    """the float64 log-space reference against mpmath at 50 digits, every alignment, on templates of about 20 bases: its own
    error is far below the tolerances the other tests use"""
    rng = np.random.default_rng(5)
    for name, (fwd, _) in models().items():
        for L, n_err in [(20, 0.15), (22, 0.3), (17, 0.1)]:
            tmpl = random_tmpl(rng, L)
            read, _ = noisy_read(rng, tmpl, n_err, run_rate=0.05)
            mlk, mcnt = R.mp_forward_backward(fwd, tmpl, read)
            s = R.Sweep(fwd, tmpl, read, R.unbanded(L, len(read)))
            assert abs(s.lk - float(mlk)) < 1e-13 * abs(float(mlk)), (name, s.lk, float(mlk))
            assert_counts_match(np.array([float(v) for v in mcnt]), s.counts(), rtol=1e-12, where=name)
            # the banded sweep at full band is the unbanded one
            assert abs(R.likelihood(fwd, tmpl, read, O.edit_ops(tmpl, read), L + len(read)) - s.lk) < 1e-13 * abs(s.lk)


def test_band_centers_match_the_oracle():
    """jo_band_centers == the centres the reference derives from the ops (Ins = op 2 keeps i, Del = op 3 advances it), runs at
    both ends included; ops that do not end at (L, n) are refused by both"""
    rng = np.random.default_rng(17)
    for k in range(40):
        L = int(rng.integers(1, 60))
        tmpl = random_tmpl(rng, L)
        lead = [(int(rng.integers(2, 4)), int(rng.integers(1, 5)))] if k % 2 else []
        tail = [(int(rng.integers(2, 4)), int(rng.integers(1, 5)))] if k % 3 else []
        read, ops = noisy_read(rng, tmpl, 0.2, run_rate=0.05, lead=lead, tail=tail)
        rc, c = oracle_centers(ops, L, len(read))
        assert rc == 0 and np.array_equal(c, R.band_centers(ops, L, len(read)))
    tmpl = random_tmpl(rng, 30)
    read, ops = noisy_read(rng, tmpl, 0.1)
    for bad, n in [(ops[:-1], len(read)), (ops, len(read) + 1), (np.append(ops, R.OP_INS), len(read))]:
        rc, _ = oracle_centers(bad, 30, n)
        assert rc != 0
        with pytest.raises(ValueError):
            R.band_centers(bad, 30, n)


# ---- tables, likelihoods and counts

@pytest.mark.parametrize("radius", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("model", ["default", "asym", "zero"])
def test_pileup_tables_at_narrow_bands(radius, model):
    """a pile-up of six reads with 10-15 % errors and indel runs of 3-6 bases, strands mixed, forward and reverse models
    distinct: every read's lk, table - lk and sentinel mask through jo_modification_table (which picks the model by strand)
    against the reference under the read's own strand's model"""
    fwd, rev = models()[model]
    rng = np.random.default_rng(100 + radius)
    L = 150 + 7 * radius
    tmpl = random_tmpl(rng, L)
    reads, opss = [], []
    for r in range(6):
        rd, op = noisy_read(rng, tmpl, 0.10 + 0.01 * r, run_rate=0.02,
                            lead=[(R.OP_INS, 3)] if r == 2 else [], tail=[(R.OP_DEL, 3)] if r == 3 else [])
        reads.append(rd)
        opss.append(op)
    strands = [1, 0, 1, 0, 0, 1]
    p = params_of(fwd, rev, L, radius)
    tab, lk = oracle_pileup_table(p, tmpl, reads, opss, strands)
    edge_mass = 0.0
    for r in range(6):
        m = fwd if strands[r] else rev
        ref_tab, ref_lk = R.modification_table(m, tmpl, reads[r], opss[r], radius)
        assert_table_matches(ref_tab, ref_lk, tab[r], lk[r], where=(model, radius, r))
        edge_mass = max(edge_mass, R.likelihood_unbanded(m, tmpl, reads[r]) - ref_lk)
    if radius <= 3:   # the band edge carries mass: a sweep one cell narrower or wider gives another answer
        assert edge_mass > 1e-3


@pytest.mark.parametrize("T", [1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129])
def test_block_boundaries(T):
    """T = L + n at the edges of the 8-diagonal unroll / checkpoint and of the 64-diagonal scaling block: a read shorter and a
    read longer than its template, under distinct models, at radius 2 and at full band; counts included"""
    fwd, rev = models()["asym"]
    rng = np.random.default_rng(T)
    shapes = [(T, 0)] if T == 1 else [((T + 1) // 2, T // 2), (T // 2, (T + 1) // 2)]
    if T >= 9:
        shapes.append((T // 3, T - T // 3))
    for L, n in shapes:
        tmpl = random_tmpl(rng, L)
        read, ops = shaped_read(rng, tmpl, n, 0.15)
        assert len(read) == n and len(read) + len(tmpl) == T
        for m in (fwd, rev):
            for radius in (2, T):
                check_read(m, tmpl, read, ops, radius, where=(T, L, n, radius))


def test_edge_shapes():
    """L = 1; reads much longer and much shorter than their template; ops that open and close with Ins / Del runs (the band is
    clipped at both corners); homopolymer templates (ctx)"""
    fwd, rev = models()["asym"]
    rng = np.random.default_rng(31)
    cases = []
    for n in (1, 2, 5):                                                 # L = 1
        tmpl = random_tmpl(rng, 1)
        read = random_tmpl(rng, n)
        cases.append((tmpl, read, O.edit_ops(tmpl, read)))
    cases.append((random_tmpl(rng, 1), np.zeros(0, np.uint8), np.array([R.OP_DEL], np.uint8)))
    tmpl = random_tmpl(rng, 30)                                         # read 3x longer
    read, ops = noisy_read(rng, tmpl, 0.1, lead=[(R.OP_INS, 30)], tail=[(R.OP_INS, 31)])
    cases.append((tmpl, read, ops))
    tmpl = random_tmpl(rng, 90)                                         # read 3x shorter
    read, ops = noisy_read(rng, tmpl[:30], 0.1)
    cases.append((tmpl, read, np.concatenate([[R.OP_DEL] * 30, ops, [R.OP_DEL] * 30]).astype(np.uint8)))
    for lead, tail in [([(R.OP_INS, 4)], [(R.OP_DEL, 5)]), ([(R.OP_DEL, 6)], [(R.OP_INS, 3)]),
                       ([(R.OP_INS, 3), (R.OP_DEL, 3)], [(R.OP_DEL, 3), (R.OP_INS, 4)])]:
        tmpl = random_tmpl(rng, 70)
        read, ops = noisy_read(rng, tmpl, 0.12, run_rate=0.02, lead=lead, tail=tail)
        cases.append((tmpl, read, ops))
    for _ in range(2):                                                  # homopolymers
        tmpl = homopolymer_tmpl(rng, 120)
        read, ops = noisy_read(rng, tmpl, 0.12, run_rate=0.02)
        cases.append((tmpl, read, ops))
    for k, (tmpl, read, ops) in enumerate(cases):
        for m in (fwd, rev):
            for radius in (1, 3, 8):
                check_read(m, tmpl, read, ops, radius, where=(k, radius))


def test_long_noisy_read():
    """2 kbp at 15 % error and indel runs, radius 30: lk far below the double range (the scaling blocks carry it), table and
    counts"""
    fwd, _ = models()["asym"]
    rng = np.random.default_rng(2)
    tmpl = random_tmpl(rng, 2000)
    read, ops = noisy_read(rng, tmpl, 0.15, run_rate=0.004)
    lk = check_read(fwd, tmpl, read, ops, 30, where="2kbp")
    assert lk < -1000 * np.log(10) / 2     # below 1e-500


@pytest.mark.parametrize("model", ["default", "zero"])
def test_full_band_table_is_the_likelihood_of_the_edited_template(model):
    """r >= L + n: every table entry is the unbanded likelihood of the explicitly edited template (the reference's unbanded
    sweep), an impossible edit is the sentinel"""
    fwd, _ = models()[model]
    rng = np.random.default_rng(9)
    for L in (1, 4, 23):
        tmpl = homopolymer_tmpl(rng, L) if L > 4 else random_tmpl(rng, L)
        read, ops = noisy_read(rng, tmpl, 0.2, run_rate=0.05)
        h = fwd.fill(O.Hmm())
        otab, olk = O.modification_table(h, tmpl, read, ops, L + len(read))
        otab = otab.reshape(L + 1, R.NUM_ROW)
        assert abs(olk - R.likelihood_unbanded(fwd, tmpl, read)) < 1e-11 * abs(olk)
        for pos in range(L + 1):
            for row in range(R.NUM_ROW):
                t2 = R.edited(tmpl, pos, row)
                if t2 is None:
                    assert otab[pos, row] <= -1e299, (pos, row)
                    continue
                want = R.likelihood_unbanded(fwd, t2, read)
                assert abs(otab[pos, row] - want) < 1e-9, (L, pos, row, otab[pos, row], want)


# ---- the refit

def test_mstep_matches_the_reference():
    """jo_fit_mstep == row normalisation; a row without mass keeps its old values"""
    fwd, rev = models()["asym"]
    rng = np.random.default_rng(4)
    tmpl = random_tmpl(rng, 200)
    read, ops = noisy_read(rng, tmpl, 0.12, run_rate=0.01)
    cnt, _ = R.counts(fwd, tmpl, read, ops, 5)
    cnt[3:6] = 0.0                                          # the Ins row without mass
    cnt[25 + 8:25 + 12] = 0.0                               # ins_emit context G without mass
    new = O.Hmm()
    O.lib().jo_fit_mstep(C.byref(rev.fill(O.Hmm())), O.f64p(cnt), C.byref(new))
    want = R.mstep(rev, cnt)
    got = R.Model.of(new)
    assert np.allclose(got.flat(), want.flat(), rtol=1e-14, atol=0)
    assert np.array_equal(got.trans[1], rev.trans[1]) and np.array_equal(got.ins[2], rev.ins[2])


def _fixed_point(batch, p, radius):
    """polish every pile-up of `batch` (HMMPolishConfig::new(radius, N, 0)) until the oracle leaves it unchanged"""
    from jtk_amd import batch as jb
    for _ in range(8):
        out = O.polish_chunks(p, batch, radius=radius, take_num=0, ignore_edge=0)
        assert out["rc"] == 0
        piles, same = [], True
        for c in range(len(batch.chunks)):
            cons = out["cons"][int(out["cons_off"][c]):int(out["cons_off"][c + 1])].copy()
            same &= bytes(cons) == bytes(batch.template(c))
            rs = list(batch.chunk_reads(c))
            piles.append((int(batch.chunks["chunk_id"][c]), 2, cons, [batch.read(r) for r in rs],
                          [out["ops_out"][int(out["ops_out_off"][r]):int(out["ops_out_off"][r + 1])].copy() for r in rs],
                          [int(batch.strand[r]) for r in rs], None))
        if same:
            return batch
        batch = jb.pack(piles)
    raise AssertionError("polishing did not converge")


@functools.lru_cache(maxsize=None)
def fit_pileups():
    """two pile-ups (270 and 290 bp, 5 % errors, both strands) that are fixed points of the fit's polish, and params with
    distinct forward / reverse models; -> (batch, params, fit radius).  The fit's polish then changes nothing and one round of
    jo_fit_model is one E-step + M-step on the pile-ups as given."""
    from jtk_amd import batch as jb, synth
    fwd, rev = models()["asym"]
    piles = []
    for cid, L in [(500, 270), (501, 290)]:
        cfg = dict(synth.CONFIGS["ont_noisy"])
        cfg.update(tmpl_len=L, reads_per_hap=4)
        piles.append(synth.make_pileup(cid, cfg))
    b = jb.pack(piles)
    p = O.Params()
    fwd.fill(p.forward)
    rev.fill(p.reverse)
    p.band_frac = 0.05
    p.haploid_coverage = 4.0
    radii = [int(np.ceil(int(t) * p.band_frac)) // 2 for t in b.chunks["tmpl_len"]]
    b = _fixed_point(b, p, max(radii))
    radii = [int(np.ceil(int(t) * p.band_frac)) // 2 for t in b.chunks["tmpl_len"]]
    assert len(set(radii)) == 1, radii          # each pile-up's polish radius is the fit's radius
    assert set(b.strand.tolist()) == {0, 1}
    return b, p, max(int(np.ceil(int(t) * p.band_frac)) for t in b.chunks["tmpl_len"]) // 2


def reference_fit(b, p, radius):
    packs = [(b.template(c), [b.read(r) for r in b.chunk_reads(c)], [b.read_ops(r) for r in b.chunk_reads(c)],
              [int(b.strand[r]) for r in b.chunk_reads(c)]) for c in range(len(b.chunks))]
    return R.fit_step(R.Model.of(p.forward), R.Model.of(p.reverse), packs, radius)


def test_counts_and_one_fit_round_match_the_reference():
    """every read's jo_phmm_counts against the reference's posterior sums, and one round of jo_fit_model (polish at a fixed
    point, counts pooled per strand, M-step per strand) against the reference's E-step + M-step"""
    b, p, radius = fit_pileups()
    fwd, rev = R.Model.of(p.forward), R.Model.of(p.reverse)
    for r in range(len(b.strand)):
        m = fwd if b.strand[r] else rev
        c = next(c for c in range(len(b.chunks)) if r in b.chunk_reads(c))
        ocnt, _ = oracle_counts(m, b.template(c), b.read(r), b.read_ops(r), radius)
        rcnt, _ = R.counts(m, b.template(c), b.read(r), b.read_ops(r), radius)
        assert_counts_match(rcnt, ocnt, where=r)
    nf, nr, _ = reference_fit(b, p, radius)
    rc, of, orv = O.fit_model(p, b, rounds=1)
    assert rc == 0
    assert np.allclose(R.Model.of(of).flat(), nf.flat(), rtol=1e-9, atol=0)
    assert np.allclose(R.Model.of(orv).flat(), nr.flat(), rtol=1e-9, atol=0)
    assert not np.allclose(nf.flat(), nr.flat(), rtol=1e-3)      # the strands' refits differ
