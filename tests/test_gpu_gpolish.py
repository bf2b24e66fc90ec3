"""jtk_lc_polish_guided on the device against tests/gpolish_reference.py, no tolerance: consensus bytes, every op, every
distance, rounds and status of the cases of tests/gpolish_cases.py, and through jtk_lc_debug_guided_table every entry of the
14-row table, dead ones included.  The CPU side (the reference against its own properties, the storage path of every read of the
ring cases, the 16-bit condition and the census of the applied edits) is tests/test_gpolish_reference.py.

Duration of `pytest tests -m gpu` on one MI355X: GPU_SUITE_SECONDS of tests/test_gpu_guided.py.  TEST_SECONDS is the call time
of each new test in a run of this module on its own; the new cases that are not listed take 0.01 to 0.04 s.

Seeded faults, each in an uncommitted copy of gpolish.hip, one build and one run of this module and tests/test_gpolish_abi.py
each: KERNEL_SEEDED_FAULTS below.  Neither fault fails any test of the two modules as they were before the ring and 16-bit cases
(20 passed, run once against the same libraries).

Not reached: gp_rethread_kernel's `overflow` arm.  Re-threaded ops consume the new template and the read, so they are at most
new_n + m <= tmpl_cap + m <= ops_cap long whenever gp_select_kernel let the round through; the arm is a second guard behind
`n + grow > tmpl_cap`, which test_pileups_beyond_the_limits_beside_pileups_that_are_answered takes."""
import numpy as np
import pytest

import gpolish_cases as K
import gpolish_reference as gp
from jtk_amd import api, batch as jb, ffi

pytestmark = pytest.mark.gpu

UNSUPPORTED, CHUNK_FAILED = -3, -6

TEST_SECONDS = {
    "test_table[f16_table]": 0.91, "test_table[ring_width4096]": 0.09, "test_table[ring_n12_wide]": 0.08, "test_polish_case[ring_rounds]": 0.28,
    "test_polish_case[f16_polish]": 0.18, "test_rounds_in_the_global_ring_in_three_slices_or_more": 0.29,
    "test_pileups_beyond_the_limits_beside_pileups_that_are_answered": 0.05,
}
KERNEL_SEEDED_FAULTS = {
    "gpolish.hip, gp_read: where the ring is in global memory, the backward fill reads the row below from ring row (i + 2) & 3":
        "test_table[ring_n1_wide, ring_n5_wide, ring_n12_wide, ring_n1_ins_run, ring_n5_ins_run, ring_n12_ins_run, ring_mixed_block, "
        "ring_width4096], test_polish_case[ring_rounds], test_rounds_in_the_global_ring_in_three_slices_or_more: table entries, then "
        "the consensus; the 26 other tests pass",
    "gpolish.hip, gp_sat: a cell saturates to the stored infinity from 32,767 on":
        "test_table[f16_table], test_polish_case[f16_polish]: the distance is lost and the call returns JTK_ERR_INTERNAL (a walk "
        "left the band); the 34 other tests pass",
}


@pytest.fixture(scope="module")
def lib(jtk_lib):
    assert jtk_lib.jtk_lc_device_ok(0) == 1, "needs a gfx950 device"
    return jtk_lib


@pytest.mark.parametrize("name", sorted(K.TABLE))
def test_table(lib, name):
    """dist and all (n + 1) x 14 entries of every read; positions n - 3 .. n are where copy and delete rows stop existing"""
    (tmpl, reads, guides, radius), want = K.table_expected(name)
    dist, table = api.guided_table(tmpl, reads, guides, radius)
    for r, (d, T, _ops) in enumerate(want):
        dead = int((T == gp.DEAD).sum())
        print(name, "read", r, "n", len(tmpl), "m", len(reads[r]), "radius", radius, "dist", d, int(dist[r]), "dead", dead)
        assert int(dist[r]) == d
        assert np.array_equal(table[r].astype(np.int64), T), (name, r, np.argwhere(table[r].astype(np.int64) != T)[:5])


def pack(names):
    cases = [K.case(n) for n in names]
    b = jb.pack([(i, 1, c["tmpl"], c["reads"], c["ops"], [1] * len(c["reads"]), None) for i, c in enumerate(cases)])
    return cases, b


def run_one(name, **kw):
    c = K.case(name)
    _, b = pack([name])
    return api.polish_guided(b, c["radius"], take_num=c["take_num"], ignore_edge=c["ignore_edge"], max_rounds=c["max_rounds"], **kw)


def check(out, c, b, want, label):
    """pile-up c of a call against the reference's (consensus, ops, dists, rounds)"""
    cons, opss, dists, rounds = want
    got = out["cons"][int(out["cons_off"][c]):int(out["cons_off"][c + 1])]
    res = out["result"][c]
    print(label, "n", len(cons), "reads", len(opss), "rounds", rounds, int(res["polish_rounds"]), "status", int(res["status"]))
    assert int(res["status"]) == 0, label
    assert bytes(got) == bytes(cons), label
    assert int(res["polish_rounds"]) == rounds, label
    for q, r in enumerate(b.chunk_reads(c)):
        ops = out["ops_out"][int(out["ops_out_off"][r]):int(out["ops_out_off"][r + 1])]
        assert ops.tolist() == opss[q].tolist(), (label, q)
        assert int(out["dist"][r]) == dists[q], (label, q)


@pytest.mark.parametrize("name", sorted(K.POLISH))
def test_polish_case(lib, name):
    out = run_one(name)
    assert out["rc"] == 0
    _, b = pack([name])
    check(out, 0, b, K.expected(name), name)
    c = K.case(name)
    if "truth" in c and name in K.PLANTED:
        assert bytes(out["cons"][:int(out["cons_off"][1])]) == bytes(c["truth"])


def mixed():
    """-> (cases, batch, radii, index of the refused pile-up)"""
    cases, b = pack(K.MIXED)
    return cases, b, np.array([c["radius"] for c in cases], dtype=np.uint32), K.MIXED.index("too_wide")


def check_mixed(out, cases, b, bad):
    assert out["rc"] == CHUNK_FAILED
    for c, name in enumerate(K.MIXED):
        if c == bad:
            assert int(out["result"][c]["status"]) == UNSUPPORTED
            assert int(out["cons_off"][c + 1]) == int(out["cons_off"][c])
            for r in b.chunk_reads(c):
                assert int(out["ops_out_off"][r + 1]) == int(out["ops_out_off"][r]) and int(out["dist"][r]) == 0xFFFFFFFF
        else:
            check(out, c, b, K.mixed_expected(name), name)


def test_mixed_batch_with_one_pileup_over_the_width_cap(lib):
    cases, b, radii, bad = mixed()
    with pytest.raises(ffi.JtkError):
        api.polish_guided(b, radii, max_rounds=K.MIXED_ROUNDS)
    out = api.polish_guided(b, radii, max_rounds=K.MIXED_ROUNDS, raise_on_chunk_failure=False)
    assert api.gpolish_timing()["slices"] == 1
    check_mixed(out, cases, b, bad)


def test_mixed_batch_in_three_slices_or_more(lib):
    """the same call with the work-area budget at a quarter of what the reads take together: four slices or more"""
    cases, b, radii, bad = mixed()
    api.polish_guided(b, radii, max_rounds=1, raise_on_chunk_failure=False)
    need = api.gpolish_timing()["work_bytes"]
    try:
        api.guided_scratch_cap(max(need // 4, 1))
        out = api.polish_guided(b, radii, max_rounds=K.MIXED_ROUNDS, raise_on_chunk_failure=False)
        slices = api.gpolish_timing()["slices"]
    finally:
        api.guided_scratch_cap(0)
    print("work bytes", need, "slices", slices)
    assert slices >= 3
    check_mixed(out, cases, b, bad)


def test_rounds_in_the_global_ring_in_three_slices_or_more(lib):
    """ring_rounds (every row of every read is wider than 512 cells, and the template changes between the rounds) beside two
    LDS-sized pile-ups, with the work-area budget at a quarter of what the reads take: the rings are carved per slice"""
    names = ["planted70", "ring_rounds", "many_reads"]
    cases, b = pack(names)
    radii = np.array([c["radius"] for c in cases], dtype=np.uint32)
    whole = api.polish_guided(b, radii, max_rounds=K.MIXED_ROUNDS)
    assert api.gpolish_timing()["slices"] == 1
    need = api.gpolish_timing()["work_bytes"]
    try:
        api.guided_scratch_cap(max(need // 4, 1))
        out = api.polish_guided(b, radii, max_rounds=K.MIXED_ROUNDS)
        slices = api.gpolish_timing()["slices"]
    finally:
        api.guided_scratch_cap(0)
    print("work bytes", need, "slices", slices)
    assert slices >= 3 and K.case("ring_rounds")["max_rounds"] == K.MIXED_ROUNDS
    for c, name in enumerate(names):
        check(out, c, b, K.mixed_expected(name), name)
    for key in ("cons", "cons_off", "ops_out", "ops_out_off", "dist"):
        assert bytes(out[key]) == bytes(whole[key]), key


def test_pileups_beyond_the_limits_beside_pileups_that_are_answered(lib):
    """a template of 32,001 bases and a read of 32,001 bases are refused on the host (JTK_ERR_UNSUPPORTED); a template of 40
    bases under reads of 300 outgrows tmpl_cap = 109 in some round and is refused there (JTK_ERR_CHUNK_FAILED).  The reference has
    no cap and polishes that pile-up on to more than 218 bases (tests/test_gpolish_reference.py): this is a refusal, not parity.
    The pile-ups between them are answered"""
    cases, b = pack(K.LIMITS)
    radii = np.array([c["radius"] for c in cases], dtype=np.uint32)
    with pytest.raises(ffi.JtkError):
        api.polish_guided(b, radii)
    out = api.polish_guided(b, radii, raise_on_chunk_failure=False)
    assert out["rc"] == CHUNK_FAILED
    for c, name in enumerate(K.LIMITS):
        if name in K.LIMITS_STATUS:
            print(name, "status", int(out["result"][c]["status"]), "rounds", int(out["result"][c]["polish_rounds"]))
            assert int(out["result"][c]["status"]) == K.LIMITS_STATUS[name], name
            assert int(out["cons_off"][c + 1]) == int(out["cons_off"][c]), name
            for r in b.chunk_reads(c):
                assert int(out["ops_out_off"][r + 1]) == int(out["ops_out_off"][r]) and int(out["dist"][r]) == 0xFFFFFFFF, name
        else:
            check(out, c, b, K.expected(name), name)


def test_take_consensus_of_two_chunks_with_two_clusters(lib):
    """api.take_consensus and dataset.take_consensus_sequence against the composition of the two references: the global ops of
    tests/align_reference.py, then the guided polish at radius = ceil(len x band_frac); cluster 0 is the chunk's own sequence"""
    import math

    import align_reference as ar
    from jtk_amd import dataset
    rng = np.random.RandomState(77)
    chunk_seqs = {10: K.random_seq(rng, 90), 20: K.random_seq(rng, 120)}
    variant = {cid: K.mutate(rng, s, 0.04) for cid, s in chunk_seqs.items()}      # what cluster 1 of each chunk really is
    nodes = []                                                                      # (chunk, cluster, seq), shuffled into "reads"
    for cid in (10, 20):
        nodes += [(cid, 0, K.mutate(rng, chunk_seqs[cid], 0.08)) for _ in range(3)]
        nodes += [(cid, 1, K.mutate(rng, variant[cid], 0.08)) for _ in range(7)]
    order = rng.permutation(len(nodes))
    nodes = [nodes[i] for i in order]
    frac = dataset.BAND_FRAC["CLR"]
    want = {}
    for cid, cl, _ in nodes:
        if (cid, cl) in want:
            continue
        if cl == 0:
            want[cid, cl] = chunk_seqs[cid]
            continue
        seqs = [s for c2, l2, s in nodes if (c2, l2) == (cid, cl)]
        ops = [ar.align(chunk_seqs[cid], s)[0] for s in seqs]
        want[cid, cl] = gp.polish(chunk_seqs[cid], seqs, ops, math.ceil(len(chunk_seqs[cid]) * frac))[0]
    got = api.take_consensus(chunk_seqs, [n[0] for n in nodes], [n[1] for n in nodes], [n[2] for n in nodes], frac)
    assert list(got) == list(want)                                                  # bucket order: that of the nodes
    for key in want:
        print(key, "chunk", len(chunk_seqs[key[0]]), "consensus", len(want[key]), "is the variant", bytes(want[key]) == bytes(variant[key[0]]))
        assert bytes(got[key]) == bytes(want[key]), key
    assert any(bytes(want[c, 1]) != bytes(chunk_seqs[c]) for c in (10, 20))
    # the same through the DataSet: three reads that hold the nodes in this order
    text = lambda s: bytes(s).decode()   # noqa: E731
    ds = {"read_type": "CLR", "selected_chunks": [{"id": cid, "seq": text(s)} for cid, s in chunk_seqs.items()],
          "encoded_reads": [{"nodes": [{"chunk": c, "cluster": cl, "seq": text(s).lower() if k % 2 else text(s)} for k, (c, cl, s) in enumerate(nodes[a::3])]}
                            for a in range(3)]}
    flat = [n for a in range(3) for n in nodes[a::3]]
    again = api.take_consensus(chunk_seqs, [n[0] for n in flat], [n[1] for n in flat], [n[2] for n in flat], frac)
    via_ds = dataset.take_consensus_sequence(ds)
    assert {k: bytes(v).decode() for k, v in again.items()} == via_ds and list(again) == list(via_ds)
