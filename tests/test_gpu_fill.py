"""jtk_lc_fill_candidates and jtk_lc_debug_fill_pairs (fill.hip) against tests/fill_reference.py on every case of
tests/fill_cases.py.  Every output is an integer: all comparisons are exact."""
import ctypes as C

import numpy as np
import pytest

import fill_cases as K
import test_fill_reference as T
from jtk_amd import api, ffi

pytestmark = pytest.mark.gpu

NAMES = sorted(K.CASES)


def device(name, **kw):
    node_off, nodes = T.arrays(name)
    return api.fill_candidates(node_off, nodes, target=K.CASES[name]["target"], **kw)


@pytest.mark.parametrize("name", NAMES)
def test_candidates_equal_the_reference(name):
    ref, out = T.reference(name), device(name)
    assert out["coverage"].tolist() == ref["coverage"]
    assert out["ins_thr"].tolist() == ref["ins_thr"]
    assert out["cand_off"].tolist() == ref["cand_off"]
    assert T.cand_tuples(out["cands"]) == ref["cands"]
    assert not out["cands"]["reserved"].any()


@pytest.mark.parametrize("name", NAMES)
def test_pairs_equal_the_reference(name):
    node_off, nodes = T.arrays(name)
    pairs = T.pair_list(name)
    out = api.fill_pairs(node_off, nodes, [t for t, _ in pairs], [q for _, q in pairs])
    for p, (t, q) in enumerate(pairs):
        want = T.pair_reference(name, t, q)
        got = dict(dir=int(out["dir"][p]), score=int(out["score"][p]), ops=out["ops"][p])
        got["pass"] = int(out["passed"][p])
        assert got == want, (t, q)


@pytest.mark.parametrize("name", ["middle_insertion_2", "random_family"])
def test_tight_capacity_returns_the_need_and_writes_nothing(name):
    ref = T.reference(name)
    need = len(ref["cands"])
    assert need > 0
    node_off, nodes = T.arrays(name)
    n_reads, n = len(node_off) - 1, len(nodes)
    coverage, ins_thr = np.full(n + n_reads, 77, dtype=np.uint32), np.full(n_reads, 77, dtype=np.uint32)
    cand_off, cands = np.full(n_reads + 1, 77, dtype=np.uint64), np.zeros(need, dtype=ffi.FILL_CAND_DT)
    cands["count"] = 77
    got = C.c_size_t(0)
    rc = ffi.lib().jtk_lc_fill_candidates(n_reads, ffi.u64p(node_off), nodes.ctypes.data, None, ffi.u32p(coverage), ffi.u32p(ins_thr),
                                          ffi.u64p(cand_off), cands.ctypes.data, need - 1, C.byref(got), 0)
    assert rc == -1 and got.value == need
    assert (coverage == 77).all() and (ins_thr == 77).all() and (cand_off == 77).all() and (cands["count"] == 77).all()
    # the binding grows the array once on that reply
    out = device(name, cand_cap=need - 1)
    assert T.cand_tuples(out["cands"]) == ref["cands"]


def test_two_runs_are_identical_byte_for_byte():
    a, b = device("random_family"), device("random_family")
    for key in ("coverage", "ins_thr", "cand_off", "cands"):
        assert a[key].tobytes() == b[key].tobytes(), key
