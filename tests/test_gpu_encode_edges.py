"""jtk_lc_encode_edges on the device against tests/edge_reference.py: status, score, the two stretches, first_chunk, head_ins and,
per chunk, the verdict, the counts, the query range, the position and every op of every trial of tests/edge_cases.py, no
tolerance.  That the trials are what they are named for is asserted on the CPU in tests/test_edge_reference.py.
api.edge_consensus against the same composition of tests/align_reference.py and tests/gpolish_reference.py.

TEST_SECONDS is the call time of each test in a run of this module on its own on one MI355X (the reference's share included;
the references of all named trials are computed once, in the first test's set-up: 14 s).

Seeded faults of edge_cut_kernel, each a single compared or counted value changed in an uncommitted copy of encode_edges.hip
(one build, one run of this module without the consensus tests): KERNEL_SEEDED_FAULTS below."""
import numpy as np
import pytest

import align_reference as A
import edge_cases as EC
import edge_reference as ER
import gpolish_reference as GP
from guided_cases import mutate_with_guide, random_seq
from jtk_amd import api, ffi

pytestmark = pytest.mark.gpu

TEST_SECONDS = {
    "test_named_trials": 0.77, "test_named_trial_alone": 0.01, "test_batch_of_70": 1.03, "test_batch_of_70_with_the_pass_in_three_slices_or_more": 0.04,
    "test_two_kbp_trial": 0.62, "test_a_radius_above_256_alone_and_in_a_batch": 0.63, "test_refused_trials_beside_answered_ones": 0.02,
    "test_windows_of_one_read_against_one_contig": 0.16, "test_edge_consensus_against_the_reference": 2.25, "test_edge_consensus_none_conditions": 1.30,
}
KERNEL_SEEDED_FAULTS = {
    "the Match ballot counts Mismatches too (op <= JTK_OP_MISMATCH for op == JTK_OP_MATCH)":
        "19 of 32 fail on mat_num: test_named_trials, test_batch_of_70 (both forms), test_two_kbp_trial, the radius-above-256, refused and "
        "shared-read tests, and 12 named trials alone; the 13 that pass hold no Mismatch (error-free, closing_op_*, leading_ins_*, ...)",
    "the prefix counts leave the lane's own op out (a count off by one: upto without bit `lane`)":
        "30 of 32 fail, on the counts or with JTK_ERR_INTERNAL from the host's check of a trial's share of the op area; nothing_aligns alone and the "
        "non-ACGT refusal, which never reach the walk, pass",
    "a chunk closed behind the pass's ops gets the index real + (bp - ctg_end) for real + (bp - ctg_end) - 1":
        "12 of 32 fail on ops_len and the ops: test_named_trials, both batches of 70, the radius-above-256, refused and shared-read tests, and "
        "closed_by_virtual_del, contig_longer_than_window, error_40_percent, lower_case, window_inside_contig (both strands) alone: every "
        "trial with a chunk that a tail Del closes",
}

RESULT_FIELDS = ("seq_start", "seq_end", "ctg_start", "ctg_end", "score", "first_chunk", "head_ins")
NODE_FIELDS = ("verdict", "mat_num", "ops_len", "query_off", "query_len", "position_from_start")


@pytest.fixture(scope="module")
def lib(jtk_lib):
    assert jtk_lib.jtk_lc_device_ok(0) == 1, "needs a gfx950 device"
    return jtk_lib


def run(trials, **kw):
    """every trial with buffers of its own, behind each other"""
    return api.encode_edges(*api.pack_edge_trials(trials), **kw)


def check_trial(out, k, t, where):
    want, got = EC.expected(t), out["result"][k]
    first = int(out["node_off"][k])
    print(where, "reference", [want[f] for f in RESULT_FIELDS], "device", [int(got[f]) for f in RESULT_FIELDS], "status", int(got["status"]))
    assert int(got["status"]) == 0, where
    assert [int(got[f]) for f in RESULT_FIELDS] == [int(want[f]) for f in RESULT_FIELDS], where
    assert int(out["node_off"][k + 1]) - first == len(want["nodes"]), where
    for q, nd in enumerate(want["nodes"]):
        dev = out["nodes"][first + q]
        assert [int(dev[f]) for f in NODE_FIELDS] == [int(nd[f]) for f in NODE_FIELDS], (where, q, [int(dev[f]) for f in NODE_FIELDS], [nd[f] for f in NODE_FIELDS])
        assert out["ops"][int(out["ops_off"][first + q]):int(out["ops_off"][first + q + 1])].tolist() == nd["ops"], (where, q)
    ref = ER.accepted_nodes(want, t["is_forward"])
    assert [(a["chunk"], a["position_from_start"], a["seq"], a["ops"].tolist()) for a in out["accepted"][k]] == \
        [(c, nd["position_from_start"], seq, nd["ops"]) for c, nd, seq in ref], where


def check(trials, out, names=None):
    assert out["rc"] == 0
    off = out["ops_off"].astype(np.int64)
    assert off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == len(out["ops"])
    for k, t in enumerate(trials):
        check_trial(out, k, t, names[k] if names else k)


def test_named_trials(lib):
    names = list(EC.CASES)
    trials = [EC.CASES[n] for n in names]
    out = run(trials)
    check(trials, out, names)
    assert {int(v) for v in out["nodes"]["verdict"]} == {ER.ACCEPTED, ER.REJECTED, ER.NOT_REACHED}


@pytest.mark.parametrize("name", sorted(EC.CASES))
def test_named_trial_alone(lib, name):
    t = EC.CASES[name]
    check([t], run([t]), [name])


def test_batch_of_70(lib):
    trials = EC.batch70()
    assert len(trials) == 70
    check(trials, run(trials))


def test_batch_of_70_with_the_pass_in_three_slices_or_more(lib):
    """with the work area's budget at a third of the pass's cells the guided pass takes three slices or more, and every byte of
    the results is that of the unsliced call"""
    trials = EC.batch70()
    whole = run(trials)
    cells = api.edges_timing()["pass_cells"]
    try:
        api.guided_scratch_cap(cells // 3)
        sliced = run(trials)
        timing = api.edges_timing()
    finally:
        api.guided_scratch_cap(0)
    print("pass cells", cells, "budget", cells // 3, "slices", timing["slices"])
    assert cells > 0 and timing["pass_cells"] == cells and timing["slices"] >= 3
    for key in ("result", "nodes", "ops", "ops_off"):
        assert bytes(sliced[key]) == bytes(whole[key]), key
    check(trials, sliced)


def test_two_kbp_trial(lib):
    t = EC.big_trial()
    check([t], run([t]))


def test_a_radius_above_256_alone_and_in_a_batch(lib):
    """rows of more than 512 cells: the pass runs its global-rows kernel, beside LDS-sized trials in the same slice"""
    t = EC.wide_band_trial()
    assert t["radius"] > 256
    check([t], run([t]))
    names = ["forward", "reverse", "window_inside_contig", "nothing_aligns", "leading_ins_64"]
    trials = [EC.CASES[n] for n in names[:2]] + [t] + [EC.CASES[n] for n in names[2:]] + [t]
    check(trials, run(trials))


def test_refused_trials_beside_answered_ones(lib):
    """a window of 32,001 bases and contig + window >= 32,768, first, in the middle and last: their status, every chunk not
    reached, an empty share of the ops, return code -6, and every other trial exact"""
    trials, refused = EC.refusal_batch()
    with pytest.raises(ffi.JtkError):
        run(trials)
    out = run(trials, raise_on_trial_failure=False)
    assert out["rc"] == -6
    off = out["ops_off"].astype(np.int64)
    assert (np.diff(off) >= 0).all() and off[0] == 0 and off[-1] == len(out["ops"])
    for k, t in enumerate(trials):
        if k in refused:
            a, b = int(out["node_off"][k]), int(out["node_off"][k + 1])
            print(k, "refused", int(out["result"][k]["status"]))
            assert int(out["result"][k]["status"]) == refused[k] and off[a] == off[b], k
            assert out["nodes"]["verdict"][a:b].tolist() == [ER.NOT_REACHED] * len(t["chunks"]) and out["accepted"][k] == [], k
            continue
        check_trial(out, k, t, k)


def test_non_acgt_window_is_refused(lib):
    t = dict(EC.CASES["forward"])
    read = bytearray(t["read"])
    read[t["start"] + 5] = ord("N")
    t["read"] = bytes(read)
    with pytest.raises(ffi.JtkError) as err:
        run([t])
    assert err.value.status == -1


def test_windows_of_one_read_against_one_contig(lib):
    """the layout of production: trials that share a read buffer, a contig and its break points give what trials with buffers of
    their own give"""
    t = EC.CASES["forward"]
    contig = EC.contig_of(t)
    shifts = [(0, 0, True), (10, -15, True), (-20, 5, True), (120, -130, True)]
    arr = np.zeros(len(shifts), dtype=ffi.EDGE_TRIAL_DT)
    trials = []
    for k, (a, b, forward) in enumerate(shifts):
        arr[k] = (0, t["start"] + a, t["end"] + b, int(forward), t["radius"], 0, len(contig), len(t["chunks"]), 0, t["sim_thr"])
        trials.append(dict(t, start=t["start"] + a, end=t["end"] + b))
    as_u8 = lambda s: np.frombuffer(s, dtype=np.uint8)   # noqa: E731
    shared = api.encode_edges(arr, as_u8(t["read"]), as_u8(contig), EC.break_points(t))
    check(trials, shared)
    own = run(trials)
    for key in ("result", "nodes", "ops", "ops_off"):
        assert bytes(shared[key]) == bytes(own[key]), key


# ---- api.edge_consensus

def pile_up(seed, n=6, length=450, err=0.06):
    rng = np.random.default_rng(seed)
    truth = random_seq(rng, length)
    return [mutate_with_guide(rng, truth, err)[0] for _ in range(n)]


def reference_consensus(seqs, cov_thr):
    """`consensus` (dense_encoding.rs:548-579) on tests/align_reference.py and tests/gpolish_reference.py"""
    plan = api.edge_consensus_plan(seqs, cov_thr)      # the host arithmetic, pinned in tests/test_edge_reference.py
    if plan is None:
        return None
    kept, band = plan
    cons = kept[0]
    opss = [A.align(GP.as_seq(cons), GP.as_seq(s))[0] for s in kept]
    for _ in range(2):
        cons, opss = GP.polish(cons, kept, opss, band)[:2]
    return bytes(cons) if len(cons) > 400 else None


@pytest.mark.parametrize("seed", [41, 42])
def test_edge_consensus_against_the_reference(lib, seed):
    seqs = pile_up(seed)
    want = reference_consensus(seqs, 3)
    got = api.edge_consensus(seqs, 3)
    assert want is not None and got is not None and bytes(got) == want


def test_edge_consensus_none_conditions(lib):
    seqs = pile_up(43)
    assert api.edge_consensus(seqs, 6) is None                                      # at most cov_thr sequences remain
    assert api.edge_consensus([s[:90] for s in seqs], 3) is None                    # 2 median <= max(median, 400) / 2
    assert api.edge_consensus([random_seq(np.random.default_rng(5), 10001)] * 3, 1) is None      # a median above 10,000
    short = pile_up(44, length=380)
    assert reference_consensus(short, 3) is None and api.edge_consensus(short, 3) is None        # the result is not longer than 400
