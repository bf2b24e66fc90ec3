"""The CPU side of jtk_lc_align_reads: the two references of the global alignment (tests/align_reference.py, numpy, written
from DESIGN section 4; oracle_ffi.edit_ops = jo_edit_ops of oracle/phmm.c) agree op for op; the band certificate the kernel
relies on holds (a fill restricted to the band of a distance bound t >= D gives the full matrix's ops, t < D reports more
than t); cigars round-trip; the entry point is declared, exported and bound, validates its arguments and has no CPU path.
Also decided here, on the CPU: which planted-edit pile-ups of tests/test_polish_reference.py the composition test of
tests/test_gpu_align_reference.py uses (COMPOSITION)."""
import ctypes as C
import functools

import numpy as np
import pytest

import align_reference as A
import oracle_ffi as O
import phmm_reference as R
import test_phmm_reference as T
import test_polish_reference as P
from jtk_amd import api, batch as jb, dataset, ffi


def pairs(seed=20, n=300):
    """lengths 0 - 400, identity 60 - 100 %, a third of them low-complexity"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        L = int(rng.integers(0, 401))
        x = A.low_complexity(rng, L) if k % 3 == 0 else A.random_seq(rng, L)
        y = A.mutate(rng, x, float(rng.uniform(0.0, 0.4)))
        if k % 10 == 0:
            y = y[:int(rng.integers(0, len(y) + 1))]          # a read much shorter than its template
        if k % 17 == 0:
            x, y = y, x
        out.append((x, y))
    out += [(A.seq(""), A.seq("")), (A.seq(""), A.seq("ACG")), (A.seq("ACG"), A.seq("")), (A.seq("A"), A.seq("A")),
            (A.seq("A" * 50), A.seq("A" * 37)), (A.seq("AC" * 40), A.seq("CA" * 40)), (A.seq("ACGT" * 20), A.seq("TGCA" * 20))]
    return out


def test_the_two_references_agree_op_for_op():
    for k, (x, y) in enumerate(pairs()):
        ops, d = A.align(x, y)
        assert bytes(ops) == bytes(O.edit_ops(x, y)), k
        assert d == int(((ops == A.MISMATCH) | (ops == A.INS) | (ops == A.DEL)).sum())
        assert int((ops != A.INS).sum()) == len(x) and int((ops != A.DEL).sum()) == len(y)


def test_the_two_references_agree_on_2kbp_pairs():
    rng = np.random.default_rng(21)
    for rate, dtype in ((0.12, np.uint16), (0.01, np.int32)):
        x = A.random_seq(rng, 2000)
        y = A.mutate(rng, x, rate)
        ops, d = A.align(x, y, dtype=dtype)
        assert bytes(ops) == bytes(O.edit_ops(x, y))


def test_empty_sides():
    assert A.align("ACGT", "")[0].tolist() == [A.DEL] * 4          # consensus/mod.rs:425-428
    assert A.align("", "ACG")[0].tolist() == [A.INS] * 3
    ops, d = A.align("", "")
    assert len(ops) == 0 and d == 0


def test_band_certificate():
    """what the kernel relies on: with the band of a bound t >= D the walk takes the full matrix's moves; t < D says so"""
    seen_below = 0
    for k, (x, y) in enumerate(pairs(seed=22, n=150)):
        ops, d = A.align(x, y)
        delta = abs(len(x) - len(y))
        for t in (d, d + 1):
            bops, bd = A.align_banded(x, y, t)
            assert bd == d and bytes(bops) == bytes(ops), (k, t)
        for t in (d - 1, (d + delta) // 2):
            if delta <= t < d:
                bops, bd = A.align_banded(x, y, t)
                assert bops is None and bd > t, (k, t, bd)
                seen_below += 1
    assert seen_below > 100


def test_cigar_round_trip():
    for x, y in pairs(seed=23, n=60):
        ops = A.align(x, y)[0]
        back = dataset.cigar_to_ops(dataset.ops_to_cigar(ops))
        assert len(back) == len(ops)
        fold = lambda o: np.where(o == A.MISMATCH, A.MATCH, o)      # noqa: E731  (kiley_op_to_ops folds the two)
        assert np.array_equal(fold(ops), back)


# ---- the entry point, without a device

def test_symbol_is_declared_exported_and_bound():
    assert "jtk_lc_align_reads" in ffi.EXPORTED_SYMBOLS
    f = ffi.lib().jtk_lc_align_reads
    assert f.restype is C.c_int and len(f.argtypes) == 12
    assert "jtk_lc_align_reads(" in open(ffi.ROOT + "/include/jtk_lc.h").read()
    assert ffi.lib().jtk_lc_version() == 2


def _call(b, ops_cap=None, nulls=(), max_dist=0, device=0):
    n = b.n_reads
    cap = int(len(b.read_bases)) + int((b.chunks["tmpl_len"] * b.chunks["n_reads"]).sum()) + 64 if ops_cap is None else ops_cap
    ops, off = np.zeros(max(cap, 1), np.uint8), np.zeros(n + 1, np.uint64)
    dist, st = np.zeros(n, np.uint32), np.zeros(n, np.int32)
    a = dict(chunks=b.chunks.ctypes.data, tmpl=ffi.u8p(b.tmpl_bases), reads=ffi.u8p(b.read_bases), read_off=ffi.u64p(b.read_off),
             ops=ffi.u8p(ops), off=ffi.u64p(off), dist=ffi.u32p(dist), st=st.ctypes.data_as(C.POINTER(C.c_int32)))
    for k in nulls:
        a[k] = None
    return ffi.lib().jtk_lc_align_reads(b.n_chunks, a["chunks"], a["tmpl"], a["reads"], a["read_off"], max_dist, a["ops"], a["off"],
                                        cap, a["dist"], a["st"], device)


def _tiny(tmpl="ACGTACGT", reads=("ACGTACGT", "ACGACGT")):
    none = np.zeros(0, np.uint8)
    return jb.pack([(1, 1, A.seq(tmpl), [A.seq(r) for r in reads], [none] * len(reads), [1] * len(reads), None)])


def test_argument_validation_comes_before_the_device():
    b = _tiny()
    for k in ("chunks", "tmpl", "reads", "read_off", "ops", "off", "dist", "st"):
        assert _call(b, nulls=(k,)) == -1, k
    bad = _tiny(reads=("ACGTACGT", "ACGNCGT"))
    assert _call(bad) == -1 and b"ACGT" in ffi.lib().jtk_lc_last_error()
    assert _call(_tiny(tmpl="ACGTACGU")) == -1
    b2 = _tiny()
    b2.read_off[1] = 100                                             # descending offsets
    assert _call(b2) == -1
    b3 = _tiny()
    b3.chunks["read_first"][0] = 1                                   # reads not laid out back to back
    assert _call(b3) == -1


def test_no_device_is_an_error_not_a_cpu_path():
    nowhere = 1 << 20                                                # an ordinal no machine has
    assert _call(_tiny(), device=nowhere) == -2
    with pytest.raises(ffi.JtkError) as e:
        api.align_reads(_tiny(), device=nowhere)
    assert e.value.status == -2
    if ffi.lib().jtk_lc_device_ok(0) != 1:
        assert _call(_tiny()) == -2


def test_with_ops_carries_new_ops():
    b = _tiny()
    ops = [A.align(b.template(0), b.read(r))[0] for r in range(b.n_reads)]
    off = np.concatenate([[0], np.cumsum([len(o) for o in ops])]).astype(np.uint64)
    b2 = b.with_ops(np.concatenate(ops), off)
    assert [b2.read_ops(r).tolist() for r in range(2)] == [o.tolist() for o in ops]
    assert b2.read_bases is b.read_bases and len(b.ops) == 0
    with pytest.raises(ValueError):
        b.with_ops(np.concatenate(ops), off[:-1])


# ---- which pile-ups the composition test on the device uses

def aligned_ops(name):
    p = P.pile_of(name)
    return [A.align(p["tmpl"], r)[0] for r in p["reads"]]


@functools.lru_cache(maxsize=None)
def reference_on_aligned_ops(name):
    """R.polish of a case of tests/test_polish_reference.py, handed the ops of align_reference instead of the case's own;
    -> dict(cons, opss, rounds), or the reason (a string) why the reference cannot run the case with them"""
    c, p = P.CASES[name], P.pile_of(name)
    fwd, rev = T.models()[c["model"]]
    try:
        cons, opss, rounds, log = R.polish(fwd, rev, p["tmpl"], p["reads"], aligned_ops(name), p["strands"], c["radius"],
                                           len(p["reads"]), 0)
    except Exception as e:                                           # noqa: BLE001  (whatever the reference raises is the reason)
        return "the reference raises %s: %s" % (type(e).__name__, e)
    bad = [d for d in log if not d["decidable"]]
    if bad:
        return "a decision of the reference is not decidable in double precision (round %d, position %d)" % (bad[0]["round"], bad[0]["pos"])
    return dict(cons=cons, opss=opss, rounds=rounds)


# cases of MAIN the reference itself cannot run on the aligned ops, each with its reason (checked below)
DROPPED = {}
COMPOSITION = [n for n in P.MAIN if n not in DROPPED and P.CASES[n]["take_num"] == 0 and P.CASES[n]["ignore_edge"] == 0]


def test_composition_cases_are_decided_by_the_reference():
    got = {n: reference_on_aligned_ops(n) for n in P.MAIN if P.CASES[n]["take_num"] == 0 and P.CASES[n]["ignore_edge"] == 0}
    dropped = {n: r for n, r in got.items() if isinstance(r, str)}
    print("dropped:", dropped)
    assert set(dropped) == set(DROPPED), dropped
    assert 2 * len(COMPOSITION) >= len(P.MAIN)
