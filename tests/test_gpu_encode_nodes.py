"""jtk_lc_encode_nodes on the device against tests/encode_reference.py: status, verdict, trims, position, query length, band,
score, the six counts and every op of every trial of tests/encode_cases.py, no tolerance.  The conditions on the trials at
the edges of the counts and on the refused trials are asserted on the CPU in tests/test_guided_reference.py.

Duration of `pytest tests -m gpu` on one MI355X: GPU_SUITE_SECONDS of tests/test_gpu_guided.py.  TEST_SECONDS is the call time
of each new or grown test in a run of this module on its own.

Seeded fault, in an uncommitted copy of encode_nodes.hip (one build, one run of this module): KERNEL_SEEDED_FAULTS below."""
import numpy as np
import pytest

import encode_cases as EC
import encode_reference as E
from jtk_amd import api, ffi

pytestmark = pytest.mark.gpu

TEST_SECONDS = {
    "test_named_trials": 0.81,      # 0.50 before the trials at the edges of the counts
    "test_refused_trials_beside_answered_ones": 0.03, "test_batch_of_70_with_every_pass_in_three_slices_or_more": 0.03,
    "test_a_band_wider_than_256_alone_and_in_a_batch": 1.55, "test_windows_of_one_read_against_one_consensus_and_one_chunk": 0.14,
}
KERNEL_SEEDED_FAULTS = {
    "encode_nodes.hip, encode_fit_kernel: the head edge takes the ops with rpos <= head_end":
        "test_named_trials, test_batch_of_70, test_two_kbp_trial, test_refused_trials_beside_answered_ones, "
        "test_batch_of_70_with_every_pass_in_three_slices_or_more, test_a_band_wider_than_256_alone_and_in_a_batch, "
        "test_windows_of_one_read_against_one_consensus_and_one_chunk: head_len and head_match; the two tests without an answered "
        "trial past the filter pass",
}

FIELDS = ("verdict", "trim_head", "trim_tail", "position_from_start", "query_len", "band", "score", "mat_num", "ops_len", "head_match", "head_len",
          "tail_match", "tail_len")


@pytest.fixture(scope="module")
def lib(jtk_lib):
    assert jtk_lib.jtk_lc_device_ok(0) == 1, "needs a gfx950 device"
    return jtk_lib


def run(trials, **kw):
    """every trial with buffers of its own, behind each other"""
    reads, conses, chunks = (api._flat([t[k] for t in trials]) for k in ("read", "cons", "chunk_seq"))
    arr = np.zeros(len(trials), dtype=ffi.ENCODE_TRIAL_DT)
    for k, t in enumerate(trials):
        arr[k] = (reads[1][k], t["start"], t["end"], int(t["is_forward"]), len(t["cons"]), conses[1][k], chunks[1][k], len(t["chunk_seq"]), 0,
                  t["sim_thr"])
    return api.encode_nodes(arr, reads[0], conses[0], chunks[0], **kw)


def check(trials, out, names=None):
    assert out["rc"] == 0
    for k, t in enumerate(trials):
        want, got = EC.expected(t), out["result"][k]
        where = names[k] if names else k
        print(where, "reference", [want[f] for f in FIELDS], "device", [int(got[f]) for f in FIELDS], "status", int(got["status"]))
        assert int(got["status"]) == 0, where
        assert [int(got[f]) for f in FIELDS] == [int(want[f]) for f in FIELDS], where
        assert out["ops"][int(out["ops_off"][k]):int(out["ops_off"][k + 1])].tolist() == want["ops"], where


def test_named_trials(lib):
    names = list(EC.CASES)
    trials = [EC.CASES[n] for n in names]
    out = run(trials)
    check(trials, out, names)
    verdicts = {int(v) for v in out["result"]["verdict"]}
    assert verdicts == {E.ACCEPTED, E.LOWER_BOUND, E.REJECTED}


def test_batch_of_70(lib):
    trials = EC.batch70()
    assert len(trials) == 70
    check(trials, run(trials))


def test_two_kbp_trial(lib):
    t = EC.big_trial()
    check([t], run([t]))


def test_a_trial_that_only_the_filter_sees(lib):
    """nothing but lower-bound verdicts: no device work is queued, the ops are empty"""
    t = EC.CASES["lower_bound"]
    out = run([t, t])
    assert out["rc"] == 0 and out["result"]["verdict"].tolist() == [E.LOWER_BOUND] * 2 and len(out["ops"]) == 0


def test_non_acgt_window_is_refused(lib):
    t = dict(EC.CASES["forward"])
    read = bytearray(t["read"])
    read[t["start"] + 5] = ord("N")
    t["read"] = bytes(read)
    with pytest.raises(ffi.JtkError) as err:
        run([t])
    assert err.value.status == -1


def test_refused_trials_beside_answered_ones(lib):
    """trials that the infix alignment, the first guided pass and the length limit refuse, first, in the middle and last in a
    batch with trials that stop at the filter: their status, an empty share of the ops, and every other trial exact"""
    trials, refused = EC.refusal_batch()
    with pytest.raises(ffi.JtkError):
        run(trials)
    out = run(trials, raise_on_trial_failure=False)
    assert out["rc"] == -6
    off = out["ops_off"].astype(np.int64)
    assert (np.diff(off) >= 0).all() and off[0] == 0 and off[-1] == len(out["ops"])
    verdicts = set()
    for k, t in enumerate(trials):
        got = out["result"][k]
        if k in refused:
            print(k, "refused", int(got["status"]))
            assert int(got["status"]) == refused[k] and off[k + 1] == off[k], k
            continue
        want = EC.expected(t)
        verdicts.add(want["verdict"])
        assert int(got["status"]) == 0, k
        assert [int(got[f]) for f in FIELDS] == [int(want[f]) for f in FIELDS], k
        assert out["ops"][off[k]:off[k + 1]].tolist() == want["ops"], k
    assert verdicts == {E.ACCEPTED, E.LOWER_BOUND, E.REJECTED}


def test_batch_of_70_with_every_pass_in_three_slices_or_more(lib):
    """the three guided passes share one work area; with its budget at a third of the smallest pass's cells every pass takes
    three slices or more, and every byte of the results is that of the unsliced call"""
    trials = EC.batch70()
    whole = run(trials)
    cells = api.encode_timing()["pass_cells"]
    try:
        api.guided_scratch_cap(min(cells) // 3)
        sliced = run(trials)
    finally:
        api.guided_scratch_cap(0)
    print("pass cells", cells, "budget", min(cells) // 3)
    assert min(cells) > 0 and api.encode_timing()["pass_cells"] == cells
    for key in ("result", "ops", "ops_off"):
        assert bytes(sliced[key]) == bytes(whole[key]), key
    check(trials, sliced)


def test_a_band_wider_than_256_alone_and_in_a_batch(lib):
    """rows of more than 512 cells: all three passes run the global-rows kernel, beside LDS-sized trials in the same slice"""
    t = EC.wide_band_trial()
    assert EC.expected(t)["band"] > 256
    check([t], run([t]))
    names = ["forward", "reverse", "accepted", "identity_rejected", "cons_len1"]
    trials = [EC.CASES[n] for n in names[:2]] + [t] + [EC.CASES[n] for n in names[2:]] + [t]
    check(trials, run(trials))


def test_windows_of_one_read_against_one_consensus_and_one_chunk(lib):
    """the layout of production: overlapping windows of one read buffer, forward and reverse windows over the same bases, one
    consensus and one chunk sequence for every trial.  The same answers as with buffers of their own, and the reference's"""
    read, cons, chunk_seq, windows = EC.shared_layout()
    arr = np.zeros(len(windows), dtype=ffi.ENCODE_TRIAL_DT)
    for k, (start, end, forward, sim_thr) in enumerate(windows):
        arr[k] = (0, start, end, int(forward), len(cons), 0, 0, len(chunk_seq), 0, sim_thr)
    as_u8 = lambda s: np.frombuffer(s, dtype=np.uint8)   # noqa: E731
    shared = api.encode_nodes(arr, as_u8(read), as_u8(cons), as_u8(chunk_seq))
    trials = EC.shared_trials()
    own = run(trials)
    check(trials, shared)
    for key in ("result", "ops", "ops_off"):
        assert bytes(shared[key]) == bytes(own[key]), key
    assert {int(v) for v in shared["result"]["verdict"]} == {E.ACCEPTED, E.LOWER_BOUND, E.REJECTED}
