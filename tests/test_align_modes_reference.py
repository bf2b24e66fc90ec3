"""The CPU side of jtk_lc_align_reads_mode: tests/align_modes_reference.py (numpy, written from DESIGN section 4) against brute
force over every substring / prefix of the free sequence through align_reference's global alignment; mode global is
align_reference.align; the band certificate the kernel relies on, per mode and free side (the band of a bound t >= D gives
the full matrix's ops, start and end, t < D reports more than t); the entry point is declared, exported and bound, refuses
an unknown mode or side before it looks for a device, and has no CPU path."""
import ctypes as C
import functools

import numpy as np
import pytest

import align_modes_reference as M
import align_reference as A
import phmm_reference as R
import test_phmm_reference as T
import test_polish_reference as P
from jtk_amd import api, batch as jb, ffi

CASES = [(m, f) for m in (M.INFIX, M.PREFIX) for f in (M.FREE_TEMPLATE, M.FREE_READ)]


def non_match(ops):
    return int(((ops == A.MISMATCH) | (ops == A.INS) | (ops == A.DEL)).sum())


def small_pairs(seed=40, n=60):
    """(whole, free) of <= 40 bases: a mutated stretch of the free sequence, unrelated, low-complexity, empty"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        free = A.low_complexity(rng, int(rng.integers(1, 41))) if k % 3 == 0 else A.random_seq(rng, int(rng.integers(1, 41)))
        a = int(rng.integers(0, len(free)))
        b = int(rng.integers(a, len(free) + 1))
        whole = A.mutate(rng, free[a:b], float(rng.uniform(0.0, 0.3)))[:40]
        if k % 7 == 0:
            whole = A.random_seq(rng, int(rng.integers(0, 41)))
        out.append((whole, free))
    out += [(A.seq("A" * 10), A.seq("A" * 30)), (A.seq("AC" * 5), A.seq("CA" * 15)), (A.seq("ACGT"), A.seq("")),
            (A.seq(""), A.seq("ACGT")), (A.seq(""), A.seq("")), (A.seq("A" * 30), A.seq("A" * 10))]
    return out


def test_brute_force_over_every_substring_and_prefix():
    for k, (whole, free_seq) in enumerate(small_pairs()):
        for mode, free in CASES:
            x, y = (free_seq, whole) if free == M.FREE_TEMPLATE else (whole, free_seq)
            ops, d, start, end = M.align(x, y, mode, free)
            if len(whole) == 0:
                assert (len(ops), d, start, end) == (0, 0, 0, 0)
                continue
            if len(free_seq) == 0:
                assert ops.tolist() == [A.INS if free == M.FREE_TEMPLATE else A.DEL] * len(whole) and (d, start, end) == (len(whole), 0, 0)
                continue

            def glob(a, b):
                sub = free_seq[a:b]
                return A.align(sub, whole)[1] if free == M.FREE_TEMPLATE else A.align(whole, sub)[1]

            starts = range(len(free_seq) + 1) if mode == M.INFIX else (0,)
            best_at = {b: min(glob(a, b) for a in starts if a <= b) for b in range(len(free_seq) + 1)}
            best = min(best_at.values())
            assert d == best, (k, mode, free)
            assert end == min(b for b, v in best_at.items() if v == best), (k, mode, free)
            assert 0 <= start <= end and (mode == M.INFIX or start == 0)
            n_tmpl, n_read = int((ops != A.INS).sum()), int((ops != A.DEL).sum())
            assert (n_tmpl, n_read) == ((end - start, len(whole)) if free == M.FREE_TEMPLATE else (len(whole), end - start))
            assert non_match(ops) == d
            assert glob(start, end) == d                                  # the stretch the ops consume attains the distance
            # the ops are an alignment of exactly these bases
            i, j = (start, 0) if free == M.FREE_TEMPLATE else (0, start)
            for op in ops.tolist():
                if op in (A.MATCH, A.MISMATCH):
                    assert (x[i] == y[j]) == (op == A.MATCH)
                    i, j = i + 1, j + 1
                elif op == A.DEL:
                    i += 1
                else:
                    j += 1


def test_mode_global_is_the_global_reference():
    rng = np.random.default_rng(41)
    for k in range(30):
        x = A.random_seq(rng, int(rng.integers(0, 200)))
        y = A.mutate(rng, x, 0.2)
        ops, d = A.align(x, y)
        for free in (M.FREE_TEMPLATE, M.FREE_READ):
            got = M.align(x, y, M.GLOBAL, free)
            assert bytes(got[0]) == bytes(ops) and got[1:] == (d, 0, len(x))


def certificate_pairs(seed=42, n=90):
    """(whole, free): a mutated stretch of 0 - 300 bases inside a window with flanks of 0 - 120 bases (random, mutated,
    low-complexity), every sixth pair unrelated, some with the whole sequence the longer one"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        L = int(rng.integers(1, 301))
        core = A.low_complexity(rng, L) if k % 3 == 0 else A.random_seq(rng, L)
        mk = A.low_complexity if k % 3 == 0 else A.random_seq
        free = np.concatenate([mk(rng, int(rng.integers(0, 121))), core, mk(rng, int(rng.integers(0, 121)))])
        whole = A.mutate(rng, core, float(rng.uniform(0.0, 0.35)))
        if k % 6 == 0:
            whole = A.random_seq(rng, int(rng.integers(1, 200)))
        if k % 11 == 0:
            free = free[:max(1, len(whole) // 2)]
        if len(whole) == 0:
            whole = A.seq("A")
        out.append((whole, free))
    return out


@pytest.mark.parametrize("mode,free", CASES)
def test_band_certificate(mode, free):
    """with the band of a bound t >= D the end cell and the walk are the full matrix's; t < D says so"""
    below = 0
    for k, (whole, free_seq) in enumerate(certificate_pairs()):
        x, y = (free_seq, whole) if free == M.FREE_TEMPLATE else (whole, free_seq)
        ops, d, start, end = M.align(x, y, mode, free)
        low = max(0, len(whole) - len(free_seq))
        assert low <= d <= len(whole)
        for t in (d, d + 1):
            bops, bd, bstart, bend = M.align(x, y, mode, free, t=t)
            assert bd == d and (bstart, bend) == (start, end) and bytes(bops) == bytes(ops), (k, t)
        for t in (d - 1, (d + low) // 2, low):
            if low <= t < d:
                bops, bd, _, _ = M.align(x, y, mode, free, t=t)
                assert bops is None and bd > t, (k, t, bd)
                below += 1
    assert below > 100


def test_semiglobal_consumes_both_sequences():
    rng = np.random.default_rng(43)
    for k in range(20):
        t = A.random_seq(rng, int(rng.integers(0, 150)))
        q = np.concatenate([A.random_seq(rng, int(rng.integers(0, 40))), A.mutate(rng, t, 0.1), A.random_seq(rng, int(rng.integers(0, 40)))])
        if k % 9 == 0:
            q = q[:0]
        ops = M.semiglobal(t, q)
        assert int((ops != A.INS).sum()) == len(t) and int((ops != A.DEL).sum()) == len(q)


# ---- the entry point, without a device

def test_symbol_is_declared_exported_and_bound():
    assert "jtk_lc_align_reads_mode" in ffi.EXPORTED_SYMBOLS
    f = ffi.lib().jtk_lc_align_reads_mode
    assert f.restype is C.c_int and len(f.argtypes) == 16
    header = open(ffi.ROOT + "/include/jtk_lc.h").read()
    assert "jtk_lc_align_reads_mode(" in header and "JTK_ALIGN_INFIX = 1" in header and "JTK_ALIGN_FREE_READ = 1" in header
    assert ffi.lib().jtk_lc_version() == 2


def _tiny():
    none = np.zeros(0, np.uint8)
    return jb.pack([(1, 1, A.seq("ACGTACGTAC"), [A.seq("GTACG"), A.seq("ACGAC")], [none] * 2, [1] * 2, None)])


def _call(b, mode, free, device=0, nulls=()):
    n = b.n_reads
    cap = int(len(b.read_bases)) + int((b.chunks["tmpl_len"] * b.chunks["n_reads"]).sum()) + 64
    ops, off = np.zeros(cap, np.uint8), np.zeros(n + 1, np.uint64)
    dist, start, end, st = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.int32)
    a = dict(start=ffi.u32p(start), end=ffi.u32p(end), dist=ffi.u32p(dist))
    for k in nulls:
        a[k] = None
    return ffi.lib().jtk_lc_align_reads_mode(b.n_chunks, b.chunks.ctypes.data, ffi.u8p(b.tmpl_bases), ffi.u8p(b.read_bases),
                                             ffi.u64p(b.read_off), mode, free, 0, ffi.u8p(ops), ffi.u64p(off), cap, a["dist"],
                                             a["start"], a["end"], st.ctypes.data_as(C.POINTER(C.c_int32)), device)


def test_unknown_mode_or_side_is_refused_before_the_device():
    nowhere = 1 << 20                                                # an ordinal no machine has
    b = _tiny()
    for mode, free in ((3, 0), (-1, 0), (M.INFIX, 2), (M.PREFIX, -1)):
        assert _call(b, mode, free, device=nowhere) == -1, (mode, free)
    assert _call(b, M.GLOBAL, 7, device=nowhere) == -2               # global does not look at the side
    for k in ("start", "end", "dist"):
        assert _call(b, M.INFIX, M.FREE_TEMPLATE, device=nowhere, nulls=(k,)) == -1, k
    with pytest.raises(ValueError):
        api.align_reads(b, mode="local")
    with pytest.raises(ValueError):
        api.align_reads(b, mode="infix", free="both")


def test_no_device_is_an_error_not_a_cpu_path():
    nowhere = 1 << 20
    for mode in (M.GLOBAL, M.INFIX, M.PREFIX):
        for free in (M.FREE_TEMPLATE, M.FREE_READ):
            assert _call(_tiny(), mode, free, device=nowhere) == -2
    with pytest.raises(ffi.JtkError) as e:
        api.align_reads(_tiny(), mode="infix", free="read", device=nowhere)
    assert e.value.status == -2
    with pytest.raises(ffi.JtkError) as e:
        api.semiglobal(_tiny(), device=nowhere)
    assert e.value.status == -2
    if ffi.lib().jtk_lc_device_ok(0) != 1:
        assert _call(_tiny(), M.PREFIX, M.FREE_READ) == -2


# ---- which pile-ups the composition test on the device uses, and what the reference makes of them

COMPOSITION = ["clean_draft", "step_sub", "step_ins", "ops_under_deletion", "skip_span2_+0", "repeat_row9"]


@functools.lru_cache(maxsize=None)
def flanked_pile(name):
    """a planted-edit pile-up of tests/test_polish_reference.py whose reads carry 0 - 6 random bases on either side (read r
    of the pile-up: r % 7 in front, (3 r) % 7 behind) -> dict(tmpl, reads, strands)"""
    p = P.pile_of(name)
    rng = np.random.default_rng(4400 + sorted(P.CASES).index(name))
    reads = [np.concatenate([A.random_seq(rng, r % 7), q, A.random_seq(rng, (3 * r) % 7)]) for r, q in enumerate(p["reads"])]
    return dict(tmpl=p["tmpl"], reads=reads, strands=p["strands"])


def semiglobal_ops(name):
    p = flanked_pile(name)
    return [M.semiglobal(p["tmpl"], r) for r in p["reads"]]


@functools.lru_cache(maxsize=None)
def reference_on_semiglobal_ops(name):
    """R.polish of a flanked pile-up handed the reference's own semiglobal ops -> dict(cons, opss, rounds), or the reason
    (a string) why the reference cannot run it"""
    c, p = P.CASES[name], flanked_pile(name)
    fwd, rev = T.models()[c["model"]]
    try:
        cons, opss, rounds, log = R.polish(fwd, rev, p["tmpl"], p["reads"], semiglobal_ops(name), p["strands"], c["radius"],
                                           len(p["reads"]), 0)
    except Exception as e:                                           # noqa: BLE001  (whatever the reference raises is the reason)
        return "the reference raises %s: %s" % (type(e).__name__, e)
    bad = [d for d in log if not d["decidable"]]
    if bad:
        return "a decision of the reference is not decidable in double precision (round %d, position %d)" % (bad[0]["round"], bad[0]["pos"])
    return dict(cons=cons, opss=opss, rounds=rounds)


def test_composition_cases_are_decided_by_the_reference():
    for name in COMPOSITION:
        assert P.CASES[name]["take_num"] == 0 and P.CASES[name]["ignore_edge"] == 0
        res = reference_on_semiglobal_ops(name)
        assert isinstance(res, dict), (name, res)
        p = flanked_pile(name)
        assert any(len(r) > len(q) for r, q in zip(p["reads"], P.pile_of(name)["reads"]))
