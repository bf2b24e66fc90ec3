"""jtk_lc_align_reads on the device against tests/align_reference.py (numpy, full matrix), op for op and distance for distance:
no tolerance, every read of every call.  The CPU side (the two references agree, the band certificate, which pile-ups the
composition test uses) is tests/test_align_reference.py."""
import copy

import numpy as np
import pytest

import align_reference as A
import helpers
import test_align_reference as TA
import test_phmm_reference as T
import test_polish_reference as P
from test_dataset_json import synthetic_dataset
from test_gpu_phmm_reference import device_params
from jtk_amd import api, batch as jb, dataset as D, ffi

pytestmark = pytest.mark.gpu

UNSUPPORTED, CHUNK_FAILED, NO_DIST = -3, -6, 0xFFFFFFFF


@pytest.fixture(scope="module")
def lib(jtk_lib):
    assert jtk_lib.jtk_lc_device_ok(0) == 1, "needs a gfx950 device"
    return jtk_lib


def pile(tmpl, reads, cid=1):
    none = np.zeros(0, np.uint8)
    return (cid, 1, A.seq(tmpl), [A.seq(r) for r in reads], [none] * len(reads), [1] * len(reads), None)


def ops_of(out, r):
    return out["ops"][int(out["ops_off"][r]):int(out["ops_off"][r + 1])]


def check_batch(b, out, dtype=np.int32):
    """every read of the batch against the full-matrix reference; -> the distances"""
    assert out["rc"] == 0 and (out["status"] == 0).all()
    dists = []
    for c in range(b.n_chunks):
        for r in b.chunk_reads(c):
            ops, d = A.align(b.template(c), b.read(r), dtype=dtype)
            got = ops_of(out, r)
            print("chunk", c, "read", r, "tl", len(b.template(c)), "rl", len(b.read(r)), "D", d, "device", int(out["dist"][r]))
            assert int(out["dist"][r]) == d, (c, r)
            assert bytes(got) == bytes(ops), (c, r, np.flatnonzero(got[:min(len(got), len(ops))] != ops[:min(len(got), len(ops))])[:5])
            dists.append(d)
    return dists


@pytest.mark.parametrize("config,tmpl_len", [("ont_diploid", 400), ("hifi_diploid", 1000)])
def test_synthetic_batches_every_read(lib, config, tmpl_len):
    b, cfg, p = helpers.small_batch(config=config, n_chunks=3, tmpl_len=tmpl_len)
    check_batch(b, api.align_reads(b))


def test_lengths_around_the_lane_and_block_edges(lib):
    """reads of 0, 1, 63, 64, 65, 4095, 4096, 4097 bases against templates of 1, 64 and 2,000 (both mirrors of the band, length
    ratios far beyond 40 %), reads 40 % longer and shorter than a 2,000-base template, D = 0, D = max(tl, rl), low complexity"""
    rng = np.random.default_rng(30)
    piles = []
    for k, tl in enumerate((1, 64, 2000)):
        t = A.random_seq(rng, tl)
        piles.append(pile(t, [A.random_seq(rng, n) for n in (0, 1, 63, 64, 65, 4095, 4096, 4097)], cid=k))
    t = A.random_seq(rng, 2000)
    reads = [t.copy(), A.mutate(rng, t, 0.1)[:1200], np.concatenate([A.mutate(rng, t, 0.1), A.random_seq(rng, 800)]),
             np.concatenate([A.random_seq(rng, 700), A.mutate(rng, t, 0.05)])[:2800], A.mutate(rng, t[400:1700], 0.12)]
    piles.append(pile(t, reads, cid=3))
    piles.append(pile("A" * 300, ["C" * 300, "C" * 200, "G" * 420, "A" * 300, "A" * 180, "A" * 420], cid=4))
    piles.append(pile("AC" * 200, ["CA" * 200, "CA" * 150, "AC" * 260, "ACC" * 130], cid=5))
    piles.append(pile("", ["", "ACGT"], cid=6))
    b = jb.pack(piles)
    d = check_batch(b, api.align_reads(b))
    assert 0 in d and 300 in d


def widenings(tl, rl, d):
    """how often the schedule of DESIGN section 5 doubles t before it reaches d: t starts at the length difference plus
    max(32, (tl + rl) / 12) and never passes max(tl, rl)"""
    t, n = min(max(tl, rl), abs(tl - rl) + max(32, (tl + rl) // 12)), 0
    while t < d:
        t, n = min(2 * t, max(tl, rl)), n + 1
    return n


def test_widenings_and_max_dist(lib):
    """300-base pairs whose distances need no, one, two and three widenings of the first band; max_dist just below / at / above
    the distance of one read fails that read alone"""
    rng = np.random.default_rng(31)
    x = A.random_seq(rng, 300)
    near, mid = A.mutate(rng, x, 0.05), A.mutate(rng, x, 0.3)
    b = jb.pack([pile(x, [near, mid, A.random_seq(rng, 300)], cid=0), pile("A" * 300, ["C" * 300], cid=1)])
    full = api.align_reads(b)
    dists = check_batch(b, full)
    tl = [300, 300, 300, 300]
    got = [widenings(t, len(b.read(r)), d) for r, (t, d) in enumerate(zip(tl, dists))]
    print("distances", dists, "widenings", got)
    assert got == [0, 1, 2, 3]
    for k in (1, 2):
        for md, ok in ((dists[k] - 1, False), (dists[k], True), (dists[k] + 1, True)):
            out = api.align_reads(b, max_dist=md, raise_on_read_failure=False)
            far = [r for r in range(b.n_reads) if dists[r] > md]
            assert (k in far) == (not ok) and 3 in far
            assert out["rc"] == CHUNK_FAILED
            for r in range(b.n_reads):
                if r in far:
                    assert out["status"][r] == UNSUPPORTED and int(out["dist"][r]) == NO_DIST and len(ops_of(out, r)) == 0
                else:
                    assert out["status"][r] == 0 and int(out["dist"][r]) == dists[r]
                    assert bytes(ops_of(out, r)) == bytes(ops_of(full, r))
    with pytest.raises(Exception):
        api.align_reads(b, max_dist=10)
    assert api.align_reads(b, max_dist=300)["rc"] == 0


def test_long_and_unrelated_pairs(lib):
    """8 kbp at ~12 % divergence (one band of a quarter of the summed length), unrelated 3 kbp pairs (D ~ 0.53 len: widened
    until the band is a quarter of the matrix on each side of the diagonal)"""
    rng = np.random.default_rng(32)
    x = A.random_seq(rng, 8000)
    piles = [pile(x, [A.mutate(rng, x, 0.12)], cid=0)]
    for k in range(2):
        piles.append(pile(A.random_seq(rng, 3000), [A.random_seq(rng, 3000 + 150 * k)], cid=1 + k))
    b = jb.pack(piles)
    d = check_batch(b, api.align_reads(b), dtype=np.uint16)
    assert d[1] > 1500 and d[2] > 1500


def test_same_bytes_twice_and_in_reverse_chunk_order(lib):
    b, cfg, p = helpers.small_batch(n_chunks=4, tmpl_len=300, reads_per_hap=6)
    a, a2 = api.align_reads(b), api.align_reads(b)
    rev = b.subset(list(range(b.n_chunks))[::-1])
    c = api.align_reads(rev)
    for ch in range(b.n_chunks):
        for q, r in enumerate(b.chunk_reads(ch)):
            r2 = rev.chunk_reads(b.n_chunks - 1 - ch)[q]
            assert bytes(ops_of(a, r)) == bytes(ops_of(a2, r)) == bytes(ops_of(c, r2))
            assert a["dist"][r] == a2["dist"][r] == c["dist"][r2]


def test_polish_composes_with_device_ops(lib):
    """api.polish_chunks on batch.with_ops(device ops): the consensus, rounds and re-threaded ops of tests/phmm_reference.py's
    polish handed align_reference's ops (computed on the CPU, tests/test_align_reference.py)"""
    names = TA.COMPOSITION
    assert 2 * len(names) >= len(P.MAIN)
    radii = sorted({P.CASES[n]["radius"] for n in names})
    for radius in radii:
        group = [n for n in names if P.CASES[n]["radius"] == radius]
        b0 = P.batch_of(group)
        al = api.align_reads(b0)
        assert al["rc"] == 0
        for c, name in enumerate(group):
            for r, ops in zip(b0.chunk_reads(c), TA.aligned_ops(name)):
                assert bytes(ops_of(al, r)) == bytes(ops), (name, r)
        b = b0.with_ops(al["ops"], al["ops_off"])
        fwd, rev = T.models()[P.CASES[group[0]]["model"]]
        assert all(P.CASES[n]["model"] == P.CASES[group[0]]["model"] for n in group)
        out = api.polish_chunks(device_params(fwd, rev, 100, 8), b, radius=radius, take_num=0, ignore_edge=0)
        assert out["rc"] == 0 and (out["result"]["status"] == 0).all()
        for c, name in enumerate(group):
            P.assert_same_outcome(TA.reference_on_aligned_ops(name), *P.outputs_of(b, out, c), where=(name, radius))


def test_realign_repairs_a_dataset_whose_cigars_do_not_fit(lib):
    ds = synthetic_dataset(2, 300, 6)
    for read in ds["encoded_reads"]:
        for node in read["nodes"]:
            node["cigar"] = "%dM" % (len(node["seq"]) + 7)              # consumes neither the chunk nor the node
    gains = jb.default_params(6.0).gains
    with pytest.raises(ffi.JtkError) as e:                              # pileup_nodes' sort key already refuses the cigars
        D.local_clustering_selected(copy.deepcopy(ds), [0, 1], gains=gains, failed=[], refit=False)
    assert e.value.status == -5
    D.realign_selected(ds, [0, 1])
    D.validate(ds)
    D.sanity_check(ds)
    chunk = {c["id"]: c["seq"] for c in ds["selected_chunks"]}
    for read in ds["encoded_reads"]:
        for node in read["nodes"]:
            ops = A.align(chunk[node["chunk"]], node["seq"])[0]
            assert node["cigar"] == D.ops_to_cigar(ops)
    failed = []
    D.local_clustering_selected(ds, [0, 1], gains=gains, failed=failed, refit=False)
    assert failed == []
