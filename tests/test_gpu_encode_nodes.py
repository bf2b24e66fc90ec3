"""jtk_lc_encode_nodes on the device against tests/encode_reference.py: status, verdict, trims, position, query length, band,
score, the six counts and every op of every trial of tests/encode_cases.py, no tolerance."""
import numpy as np
import pytest

import encode_cases as EC
import encode_reference as E
from jtk_amd import api, ffi

pytestmark = pytest.mark.gpu

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
