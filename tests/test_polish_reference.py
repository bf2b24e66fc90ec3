"""The oracle's consensus polishing (oracle/phmm.c: select_edits, apply_edits_template, rethread_ops, retag_ops, jo_phmm_polish)
against the polishing of tests/phmm_reference.py, which is written from DESIGN section 4 and the rule comment over select_edits
and re-threads ops by rebuilding alignment columns, not by walking ops.

Drafts are built from a truth template by planted edits, so the shape of the fix is known, and every case asserts on the
reference's decision log that the path it is named for was taken (a case that stops reaching its path fails).  Outcomes are
compared (consensus, every read's ops, rounds), never row numbers: rows whose edited templates are byte-identical tie up to
rounding.  No decision of any case may hang on rounding (phmm_reference.DECISION_TOL); that is asserted on the reference's log
before the oracle is looked at.

A pile-up is a chain of segments.  A segment whose draft equals its truth is read with random errors; a planted segment is read
as the truth's bases, aligned to the draft's bases column by column (the surplus as an Ins or Del run), unless the case gives a
read its own bases and ops there.

Faults seeded one at a time into a scratch copy of oracle/phmm.c, and the cases of this file that then fail:
  skip shortened by one                              skip_span*, repeat_row*, step_ins / del3 / copy3, dense_many_rounds (17 cases)
  schedule 5 + (5 t mod 20)                          dense_many_rounds (the schedules part at t = 4)
  take_num also limits the re-threaded reads         take_num_and_ignore_edge[voters-1-0, voters-5-0], single_pileup_entry_point
  retag_ops skipped                                  32 cases
  a deleted base under a Match dropped, not Ins      ops_under_deletion, end_surplus_*, repeat_row10 / 12 / 13, step_copy3, dense
  new Del ops before the column of base pos - 1      ops_under_insertion, end_ins_last, end_copy_last, step_ins, step_copy3, ...
  insertion at pos = 0 emitted after the first op    end_ins_first, end_copy_first
  >= MIN_GAIN instead of >                           none, and none can: a total within 1e-6 of 0.1 is undecidable by the rule above
No draft that reaches the 20-round cap was found (drafts with adjacent errors near an end took up to 9 rounds)."""
import functools

import numpy as np
import pytest

import oracle_ffi as O
import phmm_reference as R
from test_phmm_reference import ACGT, homopolymer_tmpl, models, noisy_read, params_of, random_tmpl  # noqa: F401

M, X, I, D = R.OP_MATCH, R.OP_MISMATCH, R.OP_INS, R.OP_DEL


# ---- inputs

def seq(s):
    return np.frombuffer(s.encode(), dtype=np.uint8).copy()


def plain_tmpl(rng, L, avoid=None):
    """random bases, no two neighbours equal (so a planted edit has one position and one row class)"""
    out = [int(ACGT[rng.integers(0, 4)])] if avoid is None else [other_base(rng, avoid)]
    while len(out) < L:
        b = int(ACGT[rng.integers(0, 4)])
        if b != out[-1]:
            out.append(b)
    return np.array(out, dtype=np.uint8)


def other_base(rng, *not_these):
    while True:
        b = int(ACGT[rng.integers(0, 4)])
        if b not in [int(v) for v in not_these]:
            return b


def tagged(draft, read, ops):
    """ops with Match / Mismatch set from the bases"""
    out, i, j = [], 0, 0
    for op in ops:
        if op == I:
            j += 1
        elif op == D:
            i += 1
        else:
            op = M if draft[i] == read[j] else X
            i, j = i + 1, j + 1
        out.append(op)
    assert i == len(draft) and j == len(read), (i, j, len(draft), len(read))
    return out


def default_mid(draft, truth):
    """the truth's bases against the draft's: min(len) Match / Mismatch columns, then the surplus as one run"""
    m = min(len(draft), len(truth))
    return list(truth), [M] * m + [I] * (len(truth) - m) + [D] * (len(draft) - m)


class Seg:
    """one segment of a pile-up: draft bases, truth bases (None: the same) and, per read, what the read holds there:
    mid(r) -> None | (bases, ops);  lead(r) / tail(r) -> [(op, k)] runs for noisy_read on an unplanted segment"""

    def __init__(self, draft, truth=None, mid=None, lead=None, tail=None, err=None):
        self.draft = np.asarray(draft, dtype=np.uint8)
        self.truth = None if truth is None else np.asarray(truth, dtype=np.uint8)
        self.mid, self.lead, self.tail, self.err = mid, lead, tail, err


def build(rng, segs, n, err=0.06, strands=None, pre=None):
    """-> dict(tmpl, truth, reads, opss, strands, starts): the pile-up of n reads over the chained segments; pre(r) = number of
    random bases put before the read as an Ins run; starts[k] = draft offset of segment k"""
    draft = np.concatenate([s.draft for s in segs])
    truth = np.concatenate([s.draft if s.truth is None else s.truth for s in segs])
    reads, opss = [], []
    for r in range(n):
        rd = ACGT[rng.integers(0, 4, pre(r) if pre else 0)].tolist()
        op = [I] * len(rd)
        for s in segs:
            if s.truth is None:
                x, o = noisy_read(rng, s.draft, (err(r) if callable(err) else err) if s.err is None else s.err, lead=s.lead(r) if s.lead else (),
                                  tail=s.tail(r) if s.tail else ())
                x, o = x.tolist(), o.tolist()
            else:
                got = s.mid(r) if s.mid else None
                x, o = got if got is not None else default_mid(s.draft, s.truth)
                x = [int(v) for v in x]
                o = tagged(s.draft, x, o)
            rd += x
            op += o
        reads.append(np.array(rd, dtype=np.uint8))
        opss.append(np.array(op, dtype=np.uint8))
        R.band_centers(opss[-1], len(draft), len(reads[-1]))          # the ops walk from (0, 0) to (L, n)
    starts = np.cumsum([0] + [len(s.draft) for s in segs])[:-1].tolist()
    return dict(tmpl=draft, truth=truth, reads=reads, opss=opss, starts=starts,
                strands=list(strands) if strands is not None else [(r + 1) % 2 for r in range(n)])


def shielded(rng, left, gap=6):
    """the flank `left` with a substitution planted six bases before its end.  The scan takes the first position where ANY row
    gains, and an insertion, copy or deletion already gains one or two positions early (a mismatch is cheaper than a gap), where
    it leaves a substitution for a later round.  A substitution gains only at its own position, so the one planted here is
    selected at len(left) - gap and round 0's scan resumes at 1 + inactive(0) = 6 positions on: exactly on the edit the case is
    about"""
    k = len(left) - gap
    d = other_base(rng, left[k - 1], left[k], left[k + 1])
    return [Seg(left[:k]), Seg([d], [left[k]]), Seg(left[k + 1:])]


def op_index_of_base(ops, base):
    """index of the op that consumes template base `base`"""
    i = 0
    for k, op in enumerate(np.asarray(ops).tolist()):
        if op != I:
            if i == base:
                return k
            i += 1
    raise ValueError(base)


# ---- the cases: name -> dict(pile-up, radius, take_num (0 = all), ignore_edge, census(res))

CASES = {}
# seeds chosen on the CPU, with the reference alone, so that each case's census holds and every decision is decidable (most
# seeds put a chance repeat next to a planted edit, where the greedy scan finds a cheaper partial edit first)
SEEDS = {"skip_span2_-1": 1000, "skip_span2_+0": 1000, "skip_span2_+1": 1002, "skip_span3_-1": 1000, "skip_span3_+0": 1000,
         "skip_span3_+1": 1000, "repeat_row9": 1000, "repeat_row10": 1000, "repeat_row12": 1027, "repeat_row13": 1000,
         "step_sub": 1000, "step_ins": 1000, "step_del3": 1000, "step_copy3": 1000, "end_ins_last": 1000, "end_copy_last": 1000}


def case(radius=8, take_num=0, ignore_edge=0, model="asym", cluster=False):
    def deco(fn):
        name = fn.__name__
        CASES[name] = dict(make=functools.lru_cache(maxsize=None)(fn), radius=radius, take_num=take_num,
                           ignore_edge=ignore_edge, model=model, cluster=cluster)
        return fn
    return deco


def pile_of(name):
    return CASES[name]["make"]()


@functools.lru_cache(maxsize=None)
def reference(name, radius=None, take_num=None, ignore_edge=None, model=None):
    """R.polish of a case (its own radius / take_num / ignore_edge unless given) -> dict(cons, opss, rounds, log); asserts
    that every decision is decidable"""
    c, p = CASES[name], pile_of(name)
    radius = c["radius"] if radius is None else radius
    take_num = c["take_num"] if take_num is None else take_num
    ignore_edge = c["ignore_edge"] if ignore_edge is None else ignore_edge
    fwd, rev = models()[model or c["model"]]
    n = len(p["reads"])
    cons, opss, rounds, log = R.polish(fwd, rev, p["tmpl"], p["reads"], p["opss"], p["strands"], radius,
                                       take_num if take_num else n, ignore_edge)
    bad = [d for d in log if not d["decidable"]]
    assert not bad, (name, radius, bad[:3])
    return dict(cons=cons, opss=opss, rounds=rounds, log=log)


def applied(res, round=None):
    return [(d["round"], d["pos"], d["row"]) for d in res["log"] if d["applied"] and (round is None or d["round"] == round)]


def row_class(tmpl, pos, row):
    """sub / ins / copy / del, where an insertion of tmpl[pos] before pos is a copy (the same edited template)"""
    if row < 4:
        return "sub"
    if row >= 11:
        return "del%d" % (row - 10)
    if row >= 8:
        return "copy%d" % (row - 7)
    return "copy1" if pos < len(tmpl) and ACGT[row - 4] == tmpl[pos] else "ins"


# -- 1. every row class at both template ends

def _end_case(seed, kind, at_start):
    """a 70-base truth; the draft differs at its first (last) position by one planted edit of `kind`.  At the start, read 0 opens
    with an Ins run, read 1 with a Del run, the others with a Match (or with the planted segment's own column)"""
    rng = np.random.default_rng(seed)
    body = plain_tmpl(rng, 70)
    a = other_base(rng, body[0] if at_start else body[-1])
    b = other_base(rng, a, body[0] if at_start else body[-1])
    if at_start:
        if kind == "sub":
            d, t = [b], [a]
        elif kind == "ins":
            d, t = [], [a]
        elif kind == "copy":
            d, t = [a], [a, a]
        mid = lambda r: ([], [D] * len(d)) if r == 1 or (r == 2 and kind == "ins") else None      # noqa: E731
        segs = [Seg(d, t, mid=mid), Seg(body, lead=lambda r: [(D, 2)] if r == 1 else [])]
        return build(rng, segs, 8, pre=lambda r: 3 if r == 0 else 0)
    if kind == "sub":
        d, t = [b], [a]
    elif kind == "ins":                         # the truth's base before the last one is missing from the draft
        d, t = [b], [a, b]
        return build(rng, shielded(rng, body) + [Seg(d, t, mid=lambda r: ([a, b], [I, M]))], 8)
    elif kind == "copy":
        return build(rng, shielded(rng, body) + [Seg([a], [a, a])], 8)
    elif kind == "surplus":                     # one surplus last base
        d, t = [a], []
    elif kind == "surplus_homopolymer":         # a surplus last base that repeats the one before it
        body = np.concatenate([body, [a]]).astype(np.uint8)
        d, t = [a], []
    return build(rng, [Seg(body), Seg(d, t)], 8)


def _end_census(kind, at_start):
    def census(name, res):
        p = pile_of(name)
        L = len(p["tmpl"])
        first = applied(res, 0)
        if kind in ("sub", "ins", "copy"):
            pos = 0 if at_start else L - 1
            hit = [(q, row) for _, q, row in first if q == pos]
            assert hit and row_class(p["tmpl"], pos, hit[0][1]).rstrip("1") == kind, (name, first)
            assert bytes(res["cons"]) == bytes(p["truth"])
        if at_start:
            assert [int(o[0]) for o in p["opss"][:3]].count(I) >= 1 and int(p["opss"][1][0]) == D
            assert any(int(o[0]) in (M, X) for o in p["opss"])
    return census


for _k, (_kind, _start) in enumerate([("sub", True), ("ins", True), ("copy", True), ("sub", False), ("ins", False),
                                      ("copy", False), ("surplus", False), ("surplus_homopolymer", False)]):
    _name = "end_%s_%s" % (_kind, "first" if _start else "last")
    CASES[_name] = dict(make=functools.lru_cache(maxsize=None)(functools.partial(_end_case, SEEDS.get(_name, 100 + _k), _kind, _start)),
                        radius=8, take_num=0, ignore_edge=0, model="asym", cluster=True,
                        census=_end_census(_kind, _start))


# -- 2. rows 9, 10, 12, 13: a unit missing from / added to a di- or tri-nucleotide repeat

def _repeat_case(seed, unit, surplus):
    rng = np.random.default_rng(seed)
    u = seq(unit)
    left = plain_tmpl(rng, 40)
    left[-1] = other_base(rng, u[0], u[-1], left[-2])
    right = plain_tmpl(rng, 40, avoid=u[-1])
    right[0] = other_base(rng, u[0], u[-1], right[1])
    three, four = np.tile(u, 3), np.tile(u, 4)
    return build(rng, shielded(rng, left) + [Seg(four, three) if surplus else Seg(three, four), Seg(right)], 8)


def _repeat_census(row):
    def census(name, res):
        p = pile_of(name)
        assert applied(res)[:2] == [(0, 34, list(b"ACGT").index(p["truth"][34])), (0, 40, row)], (name, applied(res))
        # (round 0's totals also show the same missing / surplus unit at the repeat's far end, 6 positions on, where a second
        # edit overshoots; later rounds take it back)
        assert bytes(res["cons"]) == bytes(p["truth"])
    return census


for _k, (_unit, _surplus, _row) in enumerate([("AC", False, 9), ("ACG", False, 10), ("GT", True, 12), ("GTA", True, 13)]):
    CASES["repeat_row%d" % _row] = dict(make=functools.lru_cache(maxsize=None)(functools.partial(_repeat_case, SEEDS.get("repeat_row%d" % _row, 200 + _k), _unit, _surplus)),
                                        radius=8, take_num=0, ignore_edge=0, model="asym", cluster=False,
                                        census=_repeat_census(_row))


# -- 3. the skip rule

def _skip_case(seed, span, delta):
    """an error of `span` touched bases at draft position 30 (a substitution, or 2 / 3 surplus bases) and a substitution at
    30 + span + inactive(0) + delta: at delta = -1 the second is jumped over in round 0"""
    rng = np.random.default_rng(seed)
    dist = span + R.inactive(0) + delta
    left = plain_tmpl(rng, 30)
    if span == 1:
        first = Seg([other_base(rng, left[-1])], None)
        first.truth = np.array([other_base(rng, left[-1], first.draft[0])], dtype=np.uint8)
    else:
        s = plain_tmpl(rng, span)
        while s[-1] == left[-1] or s[0] == left[-1]:
            s = plain_tmpl(rng, span)
        first = Seg(s, [])
    gap = plain_tmpl(rng, dist - span, avoid=first.draft[-1])
    if span > 1:
        while gap[0] in (left[-1], first.draft[0]):
            gap = plain_tmpl(rng, dist - span, avoid=first.draft[-1])
    t2 = other_base(rng, gap[-1])
    right = plain_tmpl(rng, 30, avoid=t2)
    d2 = other_base(rng, gap[-1], t2, right[0])
    return build(rng, shielded(rng, left) + [first, Seg(gap), Seg([d2], [t2]), Seg(right)], 8)


def _skip_census(span, delta):
    def census(name, res):
        p = pile_of(name)
        second = 30 + span + R.inactive(0) + delta
        got = applied(res)
        assert (0, 30, [None, None, 12, 13][span]) in got or (span == 1 and any(r == 0 and q == 30 and row < 4 for r, q, row in got))
        scanned0 = [d["pos"] for d in res["log"] if d["round"] == 0]
        if delta < 0:
            assert second not in scanned0 and any(r == 1 and q == second - (span if span > 1 else 0) for r, q, _ in got), got
            assert res["rounds"] == 3
        else:
            assert any(r == 0 and q == second for r, q, _ in got), got
            assert res["rounds"] == 2
        assert bytes(res["cons"]) == bytes(p["truth"])
    return census


for _span in (1, 2, 3):
    for _delta in (-1, 0, 1):
        CASES["skip_span%d_%+d" % (_span, _delta)] = dict(
            make=functools.lru_cache(maxsize=None)(functools.partial(_skip_case, SEEDS.get("skip_span%d_%+d" % (_span, _delta), 300 + 10 * _span + _delta), _span, _delta)),
            radius=8, take_num=0, ignore_edge=0, model="asym", cluster=_delta == -1, census=_skip_census(_span, _delta))


def _dense_case(seed, L, lo, hi, n=8, err=0.05):
    """a draft with a planted error (substitution, missing base or surplus base) every lo .. hi bases"""
    rng = np.random.default_rng(seed)
    segs, total = [], 0
    while total < L:
        k = int(rng.integers(lo, hi + 1))
        flank = plain_tmpl(rng, k, avoid=segs[-1].draft[-1] if segs and len(segs[-1].draft) else None)
        segs.append(Seg(flank))
        total += k
        kind = int(rng.integers(0, 3))
        if kind == 0:
            t = other_base(rng, flank[-1])
            segs.append(Seg([other_base(rng, flank[-1], t)], [t]))
        elif kind == 1:
            segs.append(Seg([], [other_base(rng, flank[-1])]))
        else:
            segs.append(Seg([other_base(rng, flank[-1])], []))
        total += len(segs[-1].draft)
    segs.append(Seg(plain_tmpl(rng, 12)))
    return build(rng, segs, n, err=err)


@case(radius=8, cluster=True)
def dense_many_rounds():
    return _dense_case(400, 150, 4, 7)


def _dense_census(name, res):
    """six rounds that apply edits, so the schedule 5 + (5 t mod 21) is used at t = 0 .. 5: 5, 10, 15, 20, 25, 9 (25, not 4: the
    5 is added after the modulus)"""
    rounds_with_edits = sorted({r for r, _, _ in applied(res)})
    assert res["rounds"] >= 6 and rounds_with_edits[:6] == [0, 1, 2, 3, 4, 5], (res["rounds"], rounds_with_edits)
    assert [R.inactive(t) for t in range(6)] == [5, 10, 15, 20, 25, 9]      # 5 + (5 t mod 21)


CASES["dense_many_rounds"]["census"] = _dense_census


# -- 4. take_num and ignore_edge

@case(radius=8)
def voters():
    """12 reads of a 110-base draft.  Site A (30): only read 0 holds a variant.  Site B (60): reads 1-4 hold a variant.  Site C
    (90): the draft is wrong, but reads 0-4 agree with it and reads 5-11 hold the truth"""
    rng = np.random.default_rng(500)
    f = [plain_tmpl(rng, 30)]
    sites = []
    for k in range(3):
        d = other_base(rng, f[-1][-1])
        v = other_base(rng, f[-1][-1], d)
        nxt = plain_tmpl(rng, 29 if k < 2 else 19, avoid=d)
        while nxt[0] == v:
            nxt = plain_tmpl(rng, len(nxt), avoid=d)
        sites.append((d, v))
        f.append(nxt)
    who = [lambda r: r == 0, lambda r: 1 <= r <= 4, lambda r: r >= 5]
    segs = [Seg(f[0])]
    for k, (d, v) in enumerate(sites):
        segs += [Seg([d], [d], mid=(lambda r, k=k, d=d, v=v: ([v], [X]) if who[k](r) else ([d], [M]))), Seg(f[k + 1])]
    return build(rng, segs, 12, err=lambda r: 0.0 if r == 0 else 0.04)


def _voters_census(take):
    def census(name, res):
        want = {1: [30], 5: [60], 0: [90], 15: [90]}[take]
        assert [q for _, q, _ in applied(res)] == want and res["rounds"] == 2, (take, applied(res))
    return census


@case(radius=8)
def edge_errors():
    """substitutions planted at 2, 3, L - 4 and L - 3 of an 80-base draft"""
    rng = np.random.default_rng(511)
    t = plain_tmpl(rng, 80)
    while len(set(t[:5].tolist())) < 4 or len(set(t[-5:].tolist())) < 4:        # no repeat unit under the planted pairs
        t = plain_tmpl(rng, 80)
    segs = []
    for a, b in [(0, 2), (2, 3), (3, 4), (4, 76), (76, 77), (77, 78), (78, 80)]:
        if b - a == 1 and a in (2, 3, 76, 77):
            segs.append(Seg([other_base(rng, t[a - 1], t[a], t[a + 1])], [t[a]]))
        else:
            segs.append(Seg(t[a:b], err=0.0 if b - a < 10 else None))
    return build(rng, segs, 8)


def _edge_census(ignore_edge):
    def census(name, res):
        p = pile_of(name)
        got = [(r, q) for r, q, _ in applied(res)]
        if ignore_edge == 0:
            assert got == [(0, 2), (0, 76), (1, 3), (1, 77)], got
            assert bytes(res["cons"]) == bytes(p["truth"])
        elif ignore_edge == 3:
            assert got == [(0, 3), (0, 76)], got
            diff = np.nonzero(res["cons"] != p["truth"])[0].tolist()
            assert diff == [2, 77]
        else:
            assert not res["log"] and res["rounds"] == 1 and bytes(res["cons"]) == bytes(p["tmpl"])
    return census


# -- 5. ops under an edit

@case(radius=8, cluster=True)
def ops_under_deletion():
    """two surplus bases at 40-41 of the draft; reads hold Match, Mismatch or Del on them, with and without Ins runs before and
    after"""
    rng = np.random.default_rng(520)
    left = plain_tmpl(rng, 40)
    s = plain_tmpl(rng, 2)
    while s[-1] == left[-1] or s[0] == left[-1]:
        s = plain_tmpl(rng, 2)
    right = plain_tmpl(rng, 40, avoid=s[-1])
    while right[0] in (left[-1], s[0]):
        right = plain_tmpl(rng, 40, avoid=s[-1])
    o0, o1 = other_base(rng, s[0]), other_base(rng, s[1])
    g = lambda k: ACGT[rng.integers(0, 4, k)].tolist()                # noqa: E731
    mids = {0: ([s[0], s[1]], [M, M]), 1: ([o0, o1], [X, X]), 2: ([s[0]], [M, D]), 3: ([o1], [D, X]),
            4: (g(2) + g(2), [I, I, D, D, I, I]), 5: (g(2) + [s[0], o1] + g(3), [I, I, M, X, I, I, I]),
            6: (g(3), [I, I, I, D, D]), 7: (g(1), [D, D, I])}
    return build(rng, shielded(rng, left) + [Seg(s, [], mid=lambda r: mids.get(r)), Seg(right, err=0.03)], 14, err=0.03)


def _del_census(name, res):
    assert (0, 40, 12) in applied(res), applied(res)
    p = pile_of(name)
    kinds = {tuple(int(o[op_index_of_base(o, 40) + q]) for q in (0, 1) if op_index_of_base(o, 40) + q < len(o))
             for o in p["opss"][:4]}
    assert {(M, M), (X, X), (M, D), (D, X)} <= kinds, kinds


CASES["ops_under_deletion"]["census"] = _del_census


@case(radius=8, cluster=True)
def ops_under_insertion():
    """the draft lacks the base between 40 and 41; the column of base 40 is a Match, a Del or is followed by an Ins run, in reads
    that hold the missing base and in reads that do not"""
    rng = np.random.default_rng(530)
    left = plain_tmpl(rng, 40)
    pb = other_base(rng, left[-1])
    gb = other_base(rng, pb)
    right = plain_tmpl(rng, 40, avoid=gb)
    xs = lambda k: [other_base(rng, gb) for _ in range(k)]             # noqa: E731
    mids = {0: ([pb, gb], [M, I]), 1: ([gb], [D, I]), 2: ([pb] + xs(1) + [gb], [M, I, I]), 3: ([pb], [M]), 4: ([], [D]),
            5: ([pb] + xs(2), [M, I, I]), 6: (xs(2) + [gb], [D, I, I, I])}
    return build(rng, shielded(rng, left, gap=5) + [Seg([pb], [pb, gb], mid=lambda r: mids.get(r)), Seg(right)], 14, err=0.03)


def _ins_census(name, res):
    got = applied(res, 0)
    p = pile_of(name)
    assert any(q == 41 and row_class(p["tmpl"], q, row) == "ins" for _, q, row in got), got
    out = [res["opss"][r].tolist() for r in range(7)]
    k = [op_index_of_base(res["opss"][r], 41) for r in range(7)]      # the inserted base's column in the final ops
    assert out[3][k[3]] == D and out[3][k[3] - 1] in (M, X)           # Match, then the new Del
    assert out[4][k[4]] == D and out[4][k[4] - 1] == D                # Del, then the new Del
    assert out[5][k[5]] == D and out[5][k[5] + 1] == I                # the new Del, then the Ins run


CASES["ops_under_insertion"]["census"] = _ins_census


# -- 6. the 64-op steps of the device's re-threading

def _step_case(seed, kind):
    """one planted edit of `kind` at draft position 58 of a 100-base draft.  Reads 0-3 open with an Ins run sized so that the op
    which meets the edit (the op on base 58 for a substitution / deletion, on base 57 for an insertion / copy) has index 62, 63,
    64, 65; read 4 is padded with a closing Ins run to exactly 128 ops"""
    rng = np.random.default_rng(seed)
    left = plain_tmpl(rng, 58)
    if kind == "sub":
        t = other_base(rng, left[-1])
        plant = Seg([other_base(rng, left[-1], t)], [t])
        right = plain_tmpl(rng, 41, avoid=t)
    elif kind == "ins":
        t = other_base(rng, left[-1])
        plant = Seg([], [t])
        right = plain_tmpl(rng, 42, avoid=t)
    elif kind == "del3":
        s = plain_tmpl(rng, 3)
        while s[-1] == left[-1] or s[0] == left[-1]:
            s = plain_tmpl(rng, 3)
        plant = Seg(s, [])
        right = plain_tmpl(rng, 39, avoid=s[-1])
        while right[0] in (left[-1], s[0]):
            right = plain_tmpl(rng, 39, avoid=s[-1])
    elif kind == "copy3":
        u = seq("CAT")
        left[-1] = other_base(rng, u[0], u[-1], left[-2])
        plant = Seg(np.tile(u, 2), np.tile(u, 3))
        right = plain_tmpl(rng, 36, avoid=u[-1])
        right[0] = other_base(rng, u[0], u[-1], right[1])
    meet = 58 if kind in ("sub", "del3") else 57
    for _ in range(200):
        p = build(rng, shielded(rng, left) + [plant, Seg(right)], 9, err=0.04)
        ok = True
        for r in range(4):
            k = op_index_of_base(p["opss"][r], meet)
            ok &= k <= 62 + r
        ok &= len(p["opss"][4]) <= 128
        if ok:
            break
    else:
        raise AssertionError("no pile-up")
    for r in range(4):
        k = op_index_of_base(p["opss"][r], meet)
        pad = 62 + r - k
        p["reads"][r] = np.concatenate([ACGT[rng.integers(0, 4, pad)], p["reads"][r]]).astype(np.uint8)
        p["opss"][r] = np.concatenate([np.full(pad, I), p["opss"][r]]).astype(np.uint8)
    pad = 128 - len(p["opss"][4])
    p["reads"][4] = np.concatenate([p["reads"][4], ACGT[rng.integers(0, 4, pad)]]).astype(np.uint8)
    p["opss"][4] = np.concatenate([p["opss"][4], np.full(pad, I)]).astype(np.uint8)
    p["meet"] = meet
    return p


def _step_census(kind):
    def census(name, res):
        p = pile_of(name)
        assert [op_index_of_base(p["opss"][r], p["meet"]) for r in range(4)] == [62, 63, 64, 65]
        assert len(p["opss"][4]) == 128
        got = applied(res, 0)
        want_pos = 58
        assert any(q == want_pos and row_class(p["tmpl"], q, row) == kind for _, q, row in got), (name, got)
        if kind == "del3":       # reads 0 and 1: the three ops on the deleted bases straddle indices 63 | 64
            assert not any(int(v) == I for r in (0, 1) for v in p["opss"][r][62 + r:65 + r])
        assert bytes(res["cons"]) == bytes(p["truth"])
    return census


for _k, _kind in enumerate(["sub", "ins", "del3", "copy3"]):
    CASES["step_" + _kind] = dict(make=functools.lru_cache(maxsize=None)(functools.partial(_step_case, SEEDS.get("step_" + _kind, 600 + _k), _kind)),
                                  radius=8, take_num=0, ignore_edge=0, model="asym", cluster=True, census=_step_census(_kind))


@case(radius=8, cluster=True)
def long_many_edits():
    """about 1,100 bases, 4 reads with more than 1,023 ops each, a planted error every 35-45 bases"""
    return _dense_case(700, 1090, 35, 45, n=4, err=0.05)


def _long_census(name, res):
    p = pile_of(name)
    assert min(len(o) for o in p["opss"]) > 1023 and len(p["tmpl"]) > 1023
    assert len(applied(res, 0)) > 15, len(applied(res, 0))


CASES["long_many_edits"]["census"] = _long_census


# -- 7. a clean draft (the mixed batch's chunk that needs no edit)

@case(radius=8, cluster=True)
def clean_draft():
    rng = np.random.default_rng(800)
    return build(rng, [Seg(plain_tmpl(rng, 64))], 6)


def _clean_census(name, res):
    assert res["rounds"] == 1 and not applied(res) and bytes(res["cons"]) == bytes(pile_of(name)["tmpl"])


CASES["clean_draft"]["census"] = _clean_census
CASES["voters"]["census"] = _voters_census(0)
CASES["edge_errors"]["census"] = _edge_census(0)

MAIN = sorted(CASES)                                   # every case at its own radius, take_num = all, ignore_edge = 0
MIXED = ["clean_draft", "skip_span1_-1", "dense_many_rounds", "ops_under_deletion"]
MIXED_RADII = [8, 20, 40]                              # phmm_pair_kernel, phmm_kernel, phmm_wide_kernel on the device
VARIANTS = [("voters", 1, 0), ("voters", 5, 0), ("voters", 15, 0), ("edge_errors", 0, 3), ("edge_errors", 0, 40)]


# ---- the oracle

def batch_of(names):
    from jtk_amd import batch as jb
    piles = []
    for k, name in enumerate(names):
        p = pile_of(name)
        piles.append((900 + k, 1, p["tmpl"], p["reads"], p["opss"], p["strands"], None))
    return jb.pack(piles)


def outputs_of(b, out, c):
    """(consensus, [ops of every read], rounds) of chunk c from the output arrays of a polish_chunks / cluster_chunks call"""
    cons = out["cons"][int(out["cons_off"][c]):int(out["cons_off"][c + 1])]
    opss = [out["ops_out"][int(out["ops_out_off"][g]):int(out["ops_out_off"][g + 1])] for g in b.chunk_reads(c)]
    return cons, opss, int(out["result"]["polish_rounds"][c])


def assert_same_outcome(res, cons, opss, rounds, where):
    assert bytes(cons) == bytes(res["cons"]), (where, bytes(cons), bytes(res["cons"]))
    assert len(opss) == len(res["opss"])
    for r, (a, b) in enumerate(zip(opss, res["opss"])):
        assert bytes(a) == bytes(b), (where, r, a.tolist(), b.tolist())
    assert rounds == res["rounds"], (where, rounds, res["rounds"])


def oracle_polish(names, radius, take_num, ignore_edge, model="asym"):
    fwd, rev = models()[model]
    b = batch_of(names)
    p = params_of(fwd, rev, 100, 8)                    # the radius is given to the call, not taken from band_frac
    out = O.polish_chunks(p, b, radius=radius, take_num=take_num, ignore_edge=ignore_edge)
    assert out["rc"] == 0 and (out["result"]["status"] == 0).all()
    return b, out


@pytest.mark.parametrize("name", MAIN)
def test_case_matches_the_reference(name):
    c = CASES[name]
    res = reference(name)
    c["census"](name, res)
    b, out = oracle_polish([name], c["radius"], c["take_num"], c["ignore_edge"], c["model"])
    assert_same_outcome(res, *outputs_of(b, out, 0), where=name)


def test_surplus_last_base_is_out_of_the_rule_s_reach():
    """what the rule does with a surplus last base: a deletion that reaches the template's end (p + d >= L) and a copy that
    reaches past it (p + c > L) do not exist (edited()), so their totals are the sentinel at every position and the guard
    `p + q < L` of the copy loop in both apply_edits implementations is never false.  The rule still gets there in two rounds:
    it deletes a base just before the surplus one (p + d <= L - 1 exists) and then substitutes what that leaves wrong"""
    fwd, rev = models()["asym"]
    for name in ("end_surplus_last", "end_surplus_homopolymer_last"):
        p, res = pile_of(name), reference(name)
        L = len(p["tmpl"])
        tot = R.column_totals(fwd, rev, p["tmpl"], p["reads"], p["opss"], p["strands"], 8, len(p["reads"]))
        for q in range(L - 3, L):
            for row in range(8, R.NUM_ROW):
                assert (tot[q, row] <= R.SENTINEL / 2) == (R.edited(p["tmpl"], q, row) is None), (q, row)
        assert all(tot[L - d, 10 + d] <= R.SENTINEL / 2 for d in (1, 2, 3))
        got = applied(res)                       # the base BEFORE the surplus one goes (row 11 at L - 2), a substitution mends the end
        assert got[0][0] == 0 and got[0][1] in (L - 2, L - 3) and got[0][2] == 11 and got[1][0] == 1 and got[1][2] < 4, got
        assert len(got) == 2
        assert bytes(res["cons"]) == bytes(p["truth"]) and res["rounds"] == 3


@pytest.mark.parametrize("name,take_num,ignore_edge", VARIANTS)
def test_take_num_and_ignore_edge(name, take_num, ignore_edge):
    """take_num limits the voters, never the reads that are re-threaded; ignore_edge limits the scan at both ends"""
    res = reference(name, take_num=take_num, ignore_edge=ignore_edge)
    (_voters_census(take_num) if name == "voters" else _edge_census(ignore_edge))(name, res)
    if name == "voters":
        changed = [r for r, (a, b) in enumerate(zip(pile_of(name)["opss"], res["opss"])) if bytes(a) != bytes(b)]
        assert changed and (take_num >= 12 or max(changed) >= take_num), changed           # reads past take_num were re-threaded (re-tagged) too
    b, out = oracle_polish([name], 8, take_num, ignore_edge)
    assert_same_outcome(res, *outputs_of(b, out, 0), where=(name, take_num, ignore_edge))


@pytest.mark.parametrize("radius", MIXED_RADII)
def test_mixed_batch(radius):
    """chunks of different length in one call: 0 edits (one round), two rounds of edits, six and more; both strands under
    forward / reverse models that differ"""
    ress = [reference(name, radius=radius) for name in MIXED]
    assert ress[0]["rounds"] == 1 and ress[1]["rounds"] == 3 and ress[2]["rounds"] >= 6
    assert len({len(pile_of(n)["tmpl"]) for n in MIXED}) == len(MIXED)
    assert {0, 1} <= set(pile_of(MIXED[2])["strands"])
    b, out = oracle_polish(MIXED, radius, 0, 0)
    for c, name in enumerate(MIXED):
        assert_same_outcome(ress[c], *outputs_of(b, out, c), where=(name, radius))


def test_single_pileup_entry_point():
    """jo_phmm_polish called directly (take_num = 5, ignore_edge = 0) gives what the batch call gives"""
    import ctypes as C
    name, take = "voters", 5
    p, res = pile_of(name), reference(name, take_num=take)
    fwd, rev = models()["asym"]
    hf, hr = fwd.fill(O.Hmm()), rev.fill(O.Hmm())
    n = len(p["reads"])
    cap = max(len(o) for o in p["opss"]) + 64
    bufs = [np.zeros(cap + 8, np.uint8) for _ in range(n)]
    for k, o in zip(bufs, p["opss"]):
        k[:len(o)] = o
    reads = [np.ascontiguousarray(r) for r in p["reads"]]
    rp = (C.POINTER(C.c_uint8) * n)(*[O.u8p(r) for r in reads])
    op = (C.POINTER(C.c_uint8) * n)(*[O.u8p(k) for k in bufs])
    rl = (C.c_size_t * n)(*[len(r) for r in reads])
    ol = (C.c_size_t * n)(*[len(o) for o in p["opss"]])
    cons = np.zeros(len(p["tmpl"]) + 72, np.uint8)
    rounds = C.c_uint32(0)
    fn = O.lib().jo_phmm_polish
    fn.restype = C.c_int64
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                   C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    cl = fn(C.byref(hf), C.byref(hr), p["tmpl"].ctypes.data, len(p["tmpl"]), n, rp, rl, op, ol, cap,
            np.array(p["strands"], np.uint8).ctypes.data, 8, take, 0, cons.ctypes.data, len(cons) - 8, C.byref(rounds))
    assert cl == len(res["cons"])
    assert_same_outcome(res, cons[:cl], [bufs[r][:ol[r]] for r in range(n)], rounds.value, where=name)
