"""The variant filter and the pick on planted tables and row sums, on the CPU: tests/clustering_reference.py (filter_candidates,
pick_filtered_profiles, compress_small_gains, homopolymer_lengths, pvalues -- written from the Rust) evaluates the cases of
tests/filter_cases.py.  Here
  * the committed record tests/golden/filter_reference.json (what tests/test_gpu_filter.py holds the kernels to) is the live one,
  * every case reaches the branch it was built for, asserted from the reference's own record (dropped, candidates, picks),
  * the oracle's jo_filter_profiles agrees with the reference on every chunk: the TOTAL / CAND rows (column, row, score to one
    decimal, count), the PICK rows (the pick order), the picked columns and their score bits -- the row-sum cases through
    filter_cases.table_from_row_sums, which is written from DESIGN.md section 4 ("Row sums") with an exact-rational fma,
  * table_from_row_sums itself is held to a rational evaluation of the same sums on a random row.
"""
import ctypes as C
import functools
import json
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import clustering_reference as R
import filter_cases as F
import oracle_ffi as O
from helpers import oracle_params

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "filter_reference.json")
NAMES = list(F.CASES)


@functools.lru_cache(maxsize=None)
def case_and_reference(name):
    cs = F.CASES[name]()
    B = R.ProjectMath()
    tables = F.tables_of(cs, B.log)
    return cs, tables, F.reference(cs, B, tables)


def fixture_of(name):
    cs, _, ref = case_and_reference(name)
    return dict(input_sha256=F.input_sha256(cs), chunks=[F.as_record(r) for r in ref])


@pytest.mark.parametrize("name", NAMES)
def test_committed_record_is_the_live_one(oracle, name):
    gold = json.load(open(GOLDEN))
    assert sorted(gold) == sorted(NAMES)
    assert gold[name] == json.loads(json.dumps(fixture_of(name)))


# ---------------------------------------------------------------------------------------------------------------------------
# every case reaches its branch
# ---------------------------------------------------------------------------------------------------------------------------
def _cand(ref):
    return {pos: (lk, count) for pos, lk, count in ref["cands"]}


def _col(bp, row):
    return bp * 14 + row


def reaches_planted_60(cs, ref):
    _, _, _, where, why = F.planted_profiles()
    (r,) = ref
    for name, (bp, row) in where.items():
        assert r["dropped"].get(_col(bp, row)) == why[name] and (_col(bp, row) in _cand(r)) == (why[name] is None), name
    assert set(why.values()) == {None, "edge", "homopolymer", "strand", "gain_per_count", "row"}


def reaches_tile_edges(cs, ref):
    assert [len(ch["tmpl"]) for ch in cs["chunks"]] == [126, 127, 128, 129, 141]
    for ch, r in zip(cs["chunks"], ref):
        L = len(ch["tmpl"])
        last, c = L + 1 - 7, _cand(r)
        assert r["dropped"][_col(6, 1)] == "edge" and r["dropped"][_col(last + 1, 3)] == "edge"
        assert {_col(7, 2), _col(9, 1), _col(9, 2), _col(last, 0), _col(last, 11), _col(60, 5)} <= set(c)
        assert {127, 128} <= set(c)   # either side of the first 128-column block
    assert 14 * 128 in _cand(ref[4]) and ref[4]["dropped"][14 * 128 - 1] == "row"


def reaches_short_templates(cs, ref):
    assert [len(ch["tmpl"]) for ch in cs["chunks"]] == [12, 13, 14]
    assert [sorted(_cand(r)) for r in ref] == [[], [_col(7, 2)], [_col(7, 2), _col(8, 1)]]
    assert all(set(r["dropped"].values()) == {"edge"} for r in ref) and [len(r["probes"]) for r in ref] == [0, 1, 1]


def reaches_thresholds(cs, ref):
    (r,) = ref
    c = _cand(r)
    # |x| == min_req is kept, one ulp less is zeroed: a seventh count, or a seventh entry of the strand x sign table
    assert c[_col(10, 1)][1] == 7 and c[_col(20, 1)][1] == 6 and c[_col(10, 1)][0] != c[_col(20, 1)][0]
    comp = r["comp"]
    assert comp[6, _col(10, 1)] == 2.5 and comp[6, _col(20, 1)] == 0.0 and comp[6, _col(30, 1)] == -2.5 and comp[6, _col(40, 1)] == 0.0
    assert c[_col(30, 1)][1] == c[_col(40, 1)][1] == 6
    # count x expt == gain exactly: dropped; 2^-40 more: kept
    assert r["dropped"][_col(50, 2)] == "gain_per_count" and c[_col(60, 2)][1] == 6
    assert sum(float(x) for x in comp[:6, _col(50, 2)]) == 6 * (F.THRESHOLD_GAIN * 0.8) == 24.0


def reaches_thresholds_pos_thr(cs, ref):
    (r,) = ref
    c, comp = _cand(r), r["comp"]
    assert R.Gains.from_params(F.params_of(cs)).expected(1, R.SUBST) * 0.5 == R.POS_THR
    assert np.array_equal(comp, cs["chunks"][0]["table"] + 0.0)   # nothing is compressed away (-0.0 aside)
    assert c[_col(10, 1)][1] == 6 and c[_col(20, 1)][1] == 7      # a value of POS_THR is not counted, the next double is
    assert c[_col(60, 0)][1] == 7                                 # 0.0001 is counted ...

    def table(pos):
        return sorted((bool(s), x > 0) for x, s in zip(comp[:, pos], cs["chunks"][0]["strands"]) if abs(x) > 0.0001)
    assert len(table(_col(60, 0))) == 11 and len(table(_col(30, 2))) == 11 and len(table(_col(40, 2))) == 12   # ... but not in the table
    assert math.copysign(1.0, cs["chunks"][0]["table"][11, _col(50, 3)]) == -1.0 and _col(50, 3) in r["probes"]
    assert math.copysign(1.0, r["feat"][11, r["probes"].index(_col(50, 3))]) == 1.0   # compress_small_gains writes +0.0


def chi_square(cells):
    r_neg, r_pos, f_neg, f_pos = cells
    obs, total = [[r_neg, r_pos], [f_neg, f_pos]], sum(cells)
    strand, sign = [r_neg + r_pos, f_neg + f_pos], [r_neg + f_neg, r_pos + f_pos]
    return sum((obs[s][g] - strand[s] * sign[g] / total) ** 2 / (strand[s] * sign[g] / total) for s in range(2) for g in range(2))


def reaches_strand_and_sign(cs, ref):
    one, two = ref
    assert all(cs["chunks"][0]["strands"]) and not one["cands"] and set(one["dropped"].values()) == {"strand"} and len(one["dropped"]) == 2
    assert chi_square(F.CHISQ_BELOW) < 10.0 < chi_square(F.CHISQ_ABOVE) and chi_square(F.CHISQ_ABOVE) - chi_square(F.CHISQ_BELOW) < 2.5
    assert two["dropped"] == {_col(15, 1): "strand", _col(45, 3): "strand"} and sorted(_cand(two)) == [_col(30, 2), _col(55, 0)]
    assert all(x > 0 for x in two["comp"][:, _col(15, 1)] if x != 0.0)   # no negative value: a sign is absent


def _reaches_homopolymers(H):
    def check(cs, ref):
        (r,) = ref
        tmpl, starts = F._run_template()
        homop = R.homopolymer_lengths(tmpl)
        assert [int(homop[starts[run]]) for run in F.RUNS] == list(F.RUNS) and max(homop) == 300 > 255
        c = _cand(r)
        counts = [c[_col(starts[run] + run // 2, (b"ACGT".index(bytes([int(tmpl[starts[run]])])) + 1) % 4)][1] for run in F.RUNS]
        # reads 6 and 7 (1.9 and 3.0) against min_req = half the gain of length min(h, H)
        assert counts == {1: [8] * 6, 3: [8, 8, 7, 7, 7, 7], 8: [8, 8, 7, 6, 6, 6]}[H]
        s2, s3, s9 = starts[2], starts[3], starts[9]
        assert sorted(pos for pos, why in r["dropped"].items() if why == "homopolymer") == sorted(
            [_col(s3 + 1, 4 + (b"ACGT".index(bytes([int(tmpl[s3])])) + 2) % 4), _col(s3, 11), _col(s2 + 2, 4 + b"ACGT".index(bytes([int(tmpl[s2])])))])
        kept_ins = [pos for pos in c if 4 <= pos % 14 < 8]
        assert len(kept_ins) == 3 and _col(s2, 11) in c
        # an insertion next to its own base, on either side, in a run-free stretch
        assert any(tmpl[pos // 14 - 1] == b"ACGT"[pos % 14 - 4] for pos in kept_ins) and any(tmpl[pos // 14] == b"ACGT"[pos % 14 - 4] for pos in kept_ins)
    return check


def reaches_copy_numbers(cs, ref):
    assert [ch["copy_num"] for ch in cs["chunks"]] == [1, 2, 3, 7]
    assert not ref[0]["cands"] and not ref[0]["probes"] and np.all(ref[0]["cand"] == -1.0)
    assert [len(r["cands"]) for r in ref[1:]] == [2, 3, 4]
    B = R.ProjectMath()
    lnfact = R.ln_factorials(20, B)
    best = max(range(1, 8), key=lambda k: R.poisson_lk(6, 2.0 * k, B, lnfact))
    assert best == 3   # an inner k of the chunk of copy number 7, the last of copy number 3, beyond copy number 2
    assert {count for _, _, count in ref[3]["cands"]} == {6, 7, 8}
    assert len({(len(ch["strands"]), len(ch["tmpl"])) for ch in cs["chunks"]}) == 4


def reaches_pick_many(cs, ref):
    (r,) = ref
    cands, comp = r["cands"], r["comp"]
    grid = [c[0] // 14 for i, c in enumerate(cands) if i != 71]   # (candidate 71 is the one planted 6 bp behind a pick)
    assert len(cands) == 74 > 64 and len(grid) >= 70 and all(b - a >= 7 for a, b in zip(grid, grid[1:]))
    t1, t2, t3 = F.PM_TIED
    assert F.bits([cands[t1][1]]) == F.bits([cands[t2][1]]) == F.bits([cands[t3][1]]) and cands[t3][1] == max(c[1] for c in cands)
    assert len({t1 % 64, t2 % 64, t3 % 64}) == 3 and {t1 // 64, t3 // 64} == {0, 1}
    order = r["order"]
    assert len(order) == 12 and order[0] == t3 and order[4] == t2 and order[8] == t1   # the last first; flag 3 in one round, picked in the next
    bp = lambda i: cands[i][0] // 14   # noqa: E731
    assert bp(71) - bp(70) == 6 and 71 not in order and bp(72) - bp(70) == 7 and order[1] == 72   # masked at 6 bp, not at 7
    p2, q80, q56, qcos = (cands[i][0] for i in (F.PM_P2, F.PM_Q80, F.PM_Q56, F.PM_QCOS))
    assert order[2] == F.PM_P2 and order[3] == F.PM_Q80
    assert R._sokal_michener(comp, p2, q80) == 0.8 and abs(R._cosine_similarity(comp, p2, q80)) < 0.8
    assert R._sokal_michener(comp, p2, q56) == 5 / 6 and F.PM_Q56 in order[4:8]
    assert R._sokal_michener(comp, p2, qcos) == 0.8 and 0.8 < abs(R._cosine_similarity(comp, p2, qcos)) < 0.9


def reaches_pick_cap(cs, ref):
    full, few, same = ref
    assert all(ch["copy_num"] == 7 and len(ch["strands"]) == 48 for ch in cs["chunks"])
    assert len(full["cands"]) == 23 and len(full["probes"]) == len(full["order"]) == F.MAX_DIM == 21
    assert len(few["cands"]) == len(few["probes"]) == 5 and len(same["cands"]) == 4 and len(same["probes"]) == 3


def reaches_rows_tile_edges(cs, ref):
    assert [len(ch["tmpl"]) for ch in cs["chunks"]] == [127, 128, 129, 255, 256, 260]
    for ch, r in zip(cs["chunks"], ref):
        L, c = len(ch["tmpl"]), _cand(r)
        assert _col(L - 6, 11) in c and all(pos in c or pos // 14 == 125 for pos in ch["planted"])
        assert ch["lk"][5] == F.LOG_ZERO and np.all(r["comp"][5] == F.LOG_ZERO)                  # the dead read
        assert np.all(ch["rows"][3, F.ROWS_ZERO_ROW] == 0.0)
        assert r["comp"][3, _col(125, 0)] == F.LOG_ZERO - ch["lk"][3]                             # a row without sums
        assert {int(g) for g in ch["exps"][0]} == {-40, -3, 0, 7, 64, 300}
        if L >= 255:
            assert {_col(127, 11)} | {p for p in ch["planted"] if 120 <= p // 14 <= 134 and p // 14 != 125} <= set(c)
            assert r["dropped"][[p for p in ch["planted"] if p // 14 == 125][0]] == "pvalue"
            assert L == 255 or any(250 <= pos // 14 for pos in c)   # (255: the last live position is 249, the deletion's)
        assert len({lk for lk, _ in c.values()}) > len(c) // 2   # the columns do not share their values
    fwd, rev = F.params_of(cs).forward.mat_emit, F.params_of(cs).reverse.mat_emit
    assert list(fwd) != list(rev)


def reaches_rows_deep(cs, ref):
    (r,) = ref
    (ch,) = cs["chunks"]
    assert len(ch["strands"]) == 65535 and len(ch["tmpl"]) == 14
    c = _cand(r)
    assert c[_col(7, 1)][1] == 65534 and c[_col(8, 2)][1] == 32768 and len(c) == 2

    def cells(pos):
        col, s = r["comp"][:, pos], np.array(ch["strands"])
        return [int(((col < 0) & ~s).sum()), int(((col > 0) & ~s).sum()), int(((col < 0) & s).sum()), int(((col > 0) & s).sum())]
    assert cells(_col(7, 1)) == [0, 32767, 1, 32767] and cells(_col(8, 2)) == [16383, 16384, 16384, 16384]
    assert 2 ** 31 - 2 ** 16 == 32768 * 65534 < 2 ** 32   # the largest strand x sign product: 31 of the 32 bits it is computed in


REACHES = dict(planted_60=reaches_planted_60, tile_edges=reaches_tile_edges, short_templates=reaches_short_templates,
               thresholds=reaches_thresholds, thresholds_pos_thr=reaches_thresholds_pos_thr, strand_and_sign=reaches_strand_and_sign,
               homopolymers_h1=_reaches_homopolymers(1), homopolymers_h3=_reaches_homopolymers(3), homopolymers_h8=_reaches_homopolymers(8),
               copy_numbers=reaches_copy_numbers, pick_many=reaches_pick_many, pick_cap=reaches_pick_cap,
               rows_tile_edges=reaches_rows_tile_edges, rows_deep=reaches_rows_deep)


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_its_branch(oracle, name):
    cs, _, ref = case_and_reference(name)
    assert sorted(REACHES) == sorted(NAMES)
    REACHES[name](cs, ref)


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_oracle_filter_profiles_against_the_reference(oracle, name):
    cs, _, ref = case_and_reference(name)
    po = oracle_params(F.params_of(cs))
    L = O.lib()
    for ch, r in zip(cs["chunks"], ref):
        if ch["copy_num"] < 2:
            continue   # clustering() returns before search_variants: the oracle's filter is not called
        cfg = O.ClusterConfig(0, C.pointer(po.gains), cs["coverage"], ch["copy_num"], 1.0)
        buf = C.create_string_buffer(1 << 16)
        t = O.Trace(C.cast(buf, C.c_void_p), len(buf), 0)
        cap = 3 * max(ch["copy_num"], 2)
        pos_out, score_out = np.zeros(cap, dtype=np.uintp), np.zeros(cap)
        st = np.array(ch["strands"], dtype=np.uint8)
        flat = np.ascontiguousarray(r["comp"].ravel())
        tmpl = np.ascontiguousarray(ch["tmpl"])
        L.jo_trace_set(C.byref(t))
        try:
            d = L.jo_filter_profiles(O.u8p(tmpl), len(tmpl), O.f64p(flat), len(st), O.u8p(st), C.byref(cfg), O.szp(pos_out), O.f64p(score_out))
        finally:
            L.jo_trace_set(None)
        rows = buf.raw[:t.len].decode().splitlines()
        cands = r["cands"]
        assert rows[0] == "TOTAL\t%d" % len(cands)
        assert [x.split("\t")[1:] for x in rows if x.startswith("CAND\t")] == [[str(pos // 14), str(pos % 14), "%.1f" % lk, str(c)] for pos, lk, c in cands]
        letter = {R.SUBST: "S", R.INS: "I", R.DEL: "D"}
        assert [x.split("\t")[1:] for x in rows if x.startswith("PICK\t")] == [
            [str(cands[i][0] // 14), letter[R.diff_type_of(cands[i][0] % 14)], "%.3f" % cands[i][1]] for i in r["order"]]
        assert pos_out[:d].tolist() == r["probes"]
        by_pos = {pos: lk for pos, lk, _ in cands}
        assert F.bits(score_out[:d]) == F.bits([by_pos[pos] for pos in r["probes"]])
        # the features are the compressed profiles at the picked columns (pseudo_mcmc.rs:70-75): what the device must leave
        assert np.array_equal(r["feat"].view(np.uint64), flat.reshape(len(st), -1)[:, r["probes"]].view(np.uint64))


# ---------------------------------------------------------------------------------------------------------------------------
# table_from_row_sums
# ---------------------------------------------------------------------------------------------------------------------------
def test_fma_rounds_once():
    a, b = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30          # a * b = 1 - 2^-60: rounds to 1.0, and (a * b) - 1.0 to 0.0
    assert a * b - 1.0 == 0.0 and F.fma(a, b, -1.0) == -(2.0 ** -60)
    assert F.fma(3.0, 0.0, 5.5) == 5.5 and F.fma(0.1, 0.3, 0.0) == 0.1 * 0.3
    rng = np.random.default_rng(7)
    for x, y, z in rng.uniform(0.5, 2.0, (50, 3)):
        assert F.fma(x, y, z) == float(Fraction(x) * Fraction(y) + Fraction(z))


def test_table_from_row_sums_against_exact_sums():
    """one read with every sum non-zero: each entry is log(V) + G ln 2 - lk with V within one rounding per operation of the
    exact rational sum of DESIGN.md section 4 ("Row sums"), and the forward and the reverse model give different tables"""
    rng = np.random.default_rng(11)
    L = 9
    rows, exps, lk = rng.uniform(0.5, 2.0, (L + 1, 16)), rng.integers(-5, 6, L + 1).astype(np.int32), -3.25
    cs = F.rows_tile_edges()
    p = F.params_of(cs)
    fwd, rev = [float(x) for x in p.forward.mat_emit], [float(x) for x in p.reverse.mat_emit]
    tab = F.read_table(rows, exps, lk, fwd, L, math.log).reshape(L + 1, 14)
    assert not np.array_equal(tab, F.read_table(rows, exps, lk, rev, L, math.log).reshape(L + 1, 14))

    def exact(q, first, b):
        return sum(Fraction(fwd[4 * b + c]) * Fraction(float(rows[q][first + c])) for c in range(4)) + Fraction(float(rows[q][first + 4]))
    for pos in range(L + 1):
        for row in range(14):
            if row < 4:
                q, v = pos + 1, None if pos + 1 > L else exact(pos + 1, 0, row)
            elif row < 8:
                q, v = pos, exact(pos, 5, row - 4)
            elif row < 11:
                q, v = pos + 1, None if pos + 1 > L else Fraction(float(rows[pos + 1][10 + row - 8]))
            else:
                q = pos + row - 9
                v = None if q > L else Fraction(float(rows[q][13 + row - 11]))
            if v is None:
                assert tab[pos, row] == F.LOG_ZERO - lk
            else:
                assert abs(tab[pos, row] - (math.log(v) + int(exps[q]) * math.log(2.0) - lk)) < 1e-13
    dead = F.read_table(rows, exps, F.LOG_ZERO, fwd, L, math.log)
    assert np.all(dead == F.LOG_ZERO)
