"""jtk_lc_align_reads_mode on the device against tests/align_modes_reference.py (numpy, full matrix): op for op, distance,
start and end of every read of every call, no tolerance.  The CPU side (the reference against brute force, the band
certificate, which pile-ups the composition test uses) is tests/test_align_modes_reference.py."""
import numpy as np
import pytest

import align_modes_reference as M
import align_reference as A
import helpers
import test_align_modes_reference as TM
import test_phmm_reference as T
import test_polish_reference as P
from test_gpu_phmm_reference import device_params
from jtk_amd import api, batch as jb, ffi

pytestmark = pytest.mark.gpu

UNSUPPORTED, CHUNK_FAILED, NO_DIST = -3, -6, 0xFFFFFFFF
MODE_NAME = {M.INFIX: "infix", M.PREFIX: "prefix", M.GLOBAL: "global"}
FREE_NAME = {M.FREE_TEMPLATE: "template", M.FREE_READ: "read"}
CASES = TM.CASES


@pytest.fixture(scope="module")
def lib(jtk_lib):
    assert jtk_lib.jtk_lc_device_ok(0) == 1, "needs a gfx950 device"
    return jtk_lib


def pile(tmpl, reads, cid=1):
    none = np.zeros(0, np.uint8)
    return (cid, 1, A.seq(tmpl), [A.seq(r) for r in reads], [none] * len(reads), [1] * len(reads), None)


def pairs_batch(pairs, free):
    """(whole, free sequence) pairs, one chunk each: the free sequence is the template or the read"""
    return jb.pack([pile(f, [w], cid=k) if free == M.FREE_TEMPLATE else pile(w, [f], cid=k) for k, (w, f) in enumerate(pairs)])


def ops_of(out, r):
    return out["ops"][int(out["ops_off"][r]):int(out["ops_off"][r + 1])]


def run(b, mode, free, **kw):
    return api.align_reads(b, mode=MODE_NAME[mode], free=FREE_NAME[free], **kw)


def check_batch(b, out, mode, free):
    """every read of the batch against the full-matrix reference; -> the distances"""
    assert out["rc"] == 0 and (out["status"] == 0).all()
    dists = []
    for c in range(b.n_chunks):
        for r in b.chunk_reads(c):
            ops, d, start, end = M.align(b.template(c), b.read(r), mode, free)
            got = ops_of(out, r)
            print(MODE_NAME[mode], FREE_NAME[free], "chunk", c, "read", r, "tl", len(b.template(c)), "rl", len(b.read(r)), "D", d,
                  "start", start, "end", end, "device", int(out["dist"][r]), int(out["start"][r]), int(out["end"][r]))
            assert (int(out["dist"][r]), int(out["start"][r]), int(out["end"][r])) == (d, start, end), (c, r)
            assert bytes(got) == bytes(ops), (c, r, np.flatnonzero(got[:min(len(got), len(ops))] != ops[:min(len(got), len(ops))])[:5])
            dists.append(d)
    return dists


FLANKS = (0, 1, 63, 64, 65, 500)


@pytest.mark.parametrize("mode,free", CASES)
def test_flank_lengths(lib, mode, free):
    """a mutated copy of a 300 - 2,000-base sequence in windows with flanks of 0, 1, 63, 64, 65 and 500 bases in front,
    behind and on both sides"""
    rng = np.random.default_rng(50)
    combos = sorted({(a, 0) for a in FLANKS} | {(0, a) for a in FLANKS} | {(a, a) for a in FLANKS} | {(63, 500), (500, 1)})
    pairs = []
    for k, (lead, trail) in enumerate(combos):
        core = A.random_seq(rng, (300, 650, 1100, 2000)[k % 4])
        window = np.concatenate([A.random_seq(rng, lead), core, A.random_seq(rng, trail)])
        pairs.append((A.mutate(rng, core, (0.02, 0.12)[k % 2]), window))
    b = pairs_batch(pairs, free)
    check_batch(b, run(b, mode, free), mode, free)


@pytest.mark.parametrize("mode,free", CASES)
def test_exact_substrings_ties_unrelated_and_empty(lib, mode, free):
    """D = 0; homopolymers and tandem repeats, where many ends tie (the smallest must win); unrelated pairs; empty sides"""
    rng = np.random.default_rng(51)
    w = A.random_seq(rng, 1500)
    pairs = [(w[a:b], w) for a, b in ((0, 1500), (0, 700), (800, 1500), (333, 334), (100, 1400))]
    pairs += [(A.seq("A" * 100), A.seq("A" * 300)), (A.seq("AC" * 60), A.seq("CA" * 200)), (A.seq("ACG" * 50), A.seq("ACG" * 90 + "AC")),
              (A.seq("A" * 300), A.seq("A" * 100)), (A.seq("C" * 80), A.seq("A" * 200)), (A.seq("AAC" * 40), A.seq("A" * 150 + "C" * 150))]
    pairs += [(A.low_complexity(rng, 200), A.low_complexity(rng, 500)) for _ in range(3)]
    pairs += [(A.random_seq(rng, 400), A.random_seq(rng, 600)), (A.random_seq(rng, 900), A.random_seq(rng, 700)),
              (A.random_seq(rng, 1), A.random_seq(rng, 1000)), (A.random_seq(rng, 1000), A.random_seq(rng, 1))]
    pairs += [(A.seq(""), A.seq("ACGTAC")), (A.seq("ACGTAC"), A.seq("")), (A.seq(""), A.seq(""))]
    b = pairs_batch(pairs, free)
    out = run(b, mode, free)
    d = check_batch(b, out, mode, free)
    assert d[:5] == [0] * 5 or mode == M.PREFIX
    if mode == M.INFIX:
        assert (int(out["start"][5]), int(out["end"][5]), d[5]) == (0, 100, 0)      # "A" * 100 in "A" * 300: the first one


def widening_pairs(mode):
    rng = np.random.default_rng(52)
    core = A.random_seq(rng, 300)
    window = np.concatenate([A.random_seq(rng, 50 if mode == M.INFIX else 0), core, A.random_seq(rng, 50 if mode == M.INFIX else 100)])
    return [(A.mutate(rng, core, 0.05), window), (A.mutate(rng, core, 0.3), window), (A.random_seq(rng, 300), window),
            (A.seq("C" * 300), A.seq("A" * 400))]


@pytest.mark.parametrize("mode,free", CASES)
def test_widenings_and_max_dist(lib, mode, free):
    """300-base sequences in 400-base windows whose distances need no, one, two and three widenings of the first band (the
    schedule of DESIGN section 5: t starts at max(0, whole - free) + max(32, whole / 6), doubles, never passes the whole
    length); max_dist just below / at / above the distance of one read fails that read alone"""
    b = pairs_batch(widening_pairs(mode), free)
    full = run(b, mode, free)
    dists = check_batch(b, full, mode, free)
    got = [M.widenings(len(b.template(r)), len(b.read(r)), free, d) for r, d in enumerate(dists)]
    print("distances", dists, "widenings", got)
    assert got == [0, 1, 2, 3]
    for k in (1, 2):
        for md, ok in ((dists[k] - 1, False), (dists[k], True), (dists[k] + 1, True)):
            out = run(b, mode, free, max_dist=md, raise_on_read_failure=False)
            far = [r for r in range(b.n_reads) if dists[r] > md]
            assert (k in far) == (not ok) and 3 in far
            assert out["rc"] == CHUNK_FAILED
            for r in range(b.n_reads):
                if r in far:
                    assert out["status"][r] == UNSUPPORTED and int(out["dist"][r]) == NO_DIST and len(ops_of(out, r)) == 0
                    assert int(out["start"][r]) == 0 and int(out["end"][r]) == 0
                else:
                    assert out["status"][r] == 0 and int(out["dist"][r]) == dists[r]
                    assert bytes(ops_of(out, r)) == bytes(ops_of(full, r))
                    assert (out["start"][r], out["end"][r]) == (full["start"][r], full["end"][r])
    with pytest.raises(ffi.JtkError):
        run(b, mode, free, max_dist=10)
    assert run(b, mode, free, max_dist=300)["rc"] == 0


@pytest.mark.parametrize("mode,free", CASES)
def test_over_wide_band_is_refused_per_read(lib, mode, free):
    """17,000 bases against 17,000 with no max_dist: the band of the largest distance allowed (17,000) is the whole matrix,
    34,001 diagonals > JTK_ALIGN_MODE_MAX_BAND = 32,768.  That read alone is refused; with a max_dist whose band fits it is
    taken (the two differ by one substitution, so the expected result needs no 17,000 x 17,000 matrix)."""
    rng = np.random.default_rng(53)
    big = A.random_seq(rng, 17000)
    big2 = big.copy()
    big2[5000] = ord("A") if big[5000] != ord("A") else ord("C")
    small = A.random_seq(rng, 500)
    pairs = [(A.mutate(rng, small[100:400], 0.1), small), (big2, big), (small[:200], small)]
    b = pairs_batch(pairs, free)
    out = run(b, mode, free, raise_on_read_failure=False)
    klo, khi = M.band_of(len(b.template(1)), len(b.read(1)), 17000, mode, free)
    assert khi - klo + 1 == 34001 > 32768
    assert out["rc"] == CHUNK_FAILED and out["status"].tolist() == [0, UNSUPPORTED, 0]
    assert int(out["dist"][1]) == NO_DIST and len(ops_of(out, 1)) == 0
    for r in (0, 2):
        ops, d, start, end = M.align(b.template(r), b.read(r), mode, free)
        assert (int(out["dist"][r]), int(out["start"][r]), int(out["end"][r])) == (d, start, end)
        assert bytes(ops_of(out, r)) == bytes(ops)
    out = run(b.subset([1]), mode, free, max_dist=100)                # distance 1 is attained by the whole sequence alone
    assert (int(out["dist"][0]), int(out["start"][0]), int(out["end"][0])) == (1, 0, 17000)
    ops = ops_of(out, 0)
    assert len(ops) == 17000 and ops[5000] == A.MISMATCH and int((ops == A.MATCH).sum()) == 16999


def test_global_mode_is_jtk_lc_align_reads(lib):
    b, cfg, p = helpers.small_batch(n_chunks=3, tmpl_len=400)
    a = api.align_reads(b)
    for free in (M.FREE_TEMPLATE, M.FREE_READ):
        n = b.n_reads
        cap = len(a["ops"]) + 64
        ops, off = np.zeros(cap, np.uint8), np.zeros(n + 1, np.uint64)
        dist, start, end, st = np.zeros(n, np.uint32), np.ones(n, np.uint32), np.zeros(n, np.uint32), np.ones(n, np.int32)
        rc = lib.jtk_lc_align_reads_mode(b.n_chunks, b.chunks.ctypes.data, ffi.u8p(b.tmpl_bases), ffi.u8p(b.read_bases),
                                         ffi.u64p(b.read_off), M.GLOBAL, free, 0, ffi.u8p(ops), ffi.u64p(off), cap, ffi.u32p(dist),
                                         ffi.u32p(start), ffi.u32p(end), st.ctypes.data_as(ffi.C.POINTER(ffi.C.c_int32)), 0)
        assert rc == 0 and (st == 0).all()
        assert bytes(off) == bytes(a["ops_off"]) and bytes(ops[:int(off[n])]) == bytes(a["ops"]) and bytes(dist) == bytes(a["dist"])
        assert (start == 0).all() and end.tolist() == np.repeat(b.chunks["tmpl_len"], b.chunks["n_reads"]).tolist()


@pytest.mark.parametrize("mode,free", CASES)
def test_same_bytes_twice_and_in_reverse_chunk_order(lib, mode, free):
    b, cfg, p = helpers.small_batch(n_chunks=4, tmpl_len=300, reads_per_hap=6)
    a, a2 = run(b, mode, free), run(b, mode, free)
    rev = b.subset(list(range(b.n_chunks))[::-1])
    c = run(rev, mode, free)
    for ch in range(b.n_chunks):
        for q, r in enumerate(b.chunk_reads(ch)):
            r2 = rev.chunk_reads(b.n_chunks - 1 - ch)[q]
            assert bytes(ops_of(a, r)) == bytes(ops_of(a2, r)) == bytes(ops_of(c, r2))
            for key in ("dist", "start", "end"):
                assert a[key][r] == a2[key][r] == c[key][r2]
    check_batch(b, a, mode, free)


def test_polish_composes_with_semiglobal_ops(lib):
    """api.semiglobal's ops for reads carrying flanks, handed to api.polish_chunks via Batch.with_ops: the consensus, rounds
    and re-threaded ops of tests/phmm_reference.py's polish on the reference's own semiglobal ops"""
    names = TM.COMPOSITION
    for radius in sorted({P.CASES[n]["radius"] for n in names}):
        group = [n for n in names if P.CASES[n]["radius"] == radius]
        piles = [(900 + k, 1, TM.flanked_pile(n)["tmpl"], TM.flanked_pile(n)["reads"],
                  [np.zeros(0, np.uint8)] * len(TM.flanked_pile(n)["reads"]), TM.flanked_pile(n)["strands"], None) for k, n in enumerate(group)]
        b0 = jb.pack(piles)
        sg = api.semiglobal(b0)
        assert sg["rc"] == 0
        for c, name in enumerate(group):
            for r, ops in zip(b0.chunk_reads(c), TM.semiglobal_ops(name)):
                assert bytes(ops_of(sg, r)) == bytes(ops), (name, r)
        b = b0.with_ops(sg["ops"], sg["ops_off"])
        fwd, rev = T.models()[P.CASES[group[0]]["model"]]
        assert all(P.CASES[n]["model"] == P.CASES[group[0]]["model"] for n in group)
        out = api.polish_chunks(device_params(fwd, rev, 100, 8), b, radius=radius, take_num=0, ignore_edge=0)
        assert out["rc"] == 0 and (out["result"]["status"] == 0).all()
        for c, name in enumerate(group):
            P.assert_same_outcome(TM.reference_on_semiglobal_ops(name), *P.outputs_of(b, out, c), where=(name, radius))
