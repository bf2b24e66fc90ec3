"""jtk_lc_settle_nodes (settle.hip) through api.settle_nodes against tests/settle_reference.py on every problem of
tests/settle_cases.py, in all three modes: the statistics, keep, the per-read order, n_kept, the statuses and the return code are
equal.  No tolerance: everything is an integer but the two identities remove_overlapping_encoding compares, and those are one f64
subtraction of one f64 division of integers on either side."""
import numpy as np
import pytest

import settle_cases as K
import settle_reference as R
from jtk_amd import api, ffi

pytestmark = pytest.mark.gpu

MODES = {"stats_only": (R.STATS_ONLY, ffi.SETTLE_STATS_ONLY), "by_chunk_pos": (R.BY_CHUNK_POS, ffi.SETTLE_BY_CHUNK_POS),
         "by_chunk": (R.BY_CHUNK, ffi.SETTLE_BY_CHUNK)}


def flatten(reads):
    """the arrays of api.settle_nodes for a list of reads of tests/settle_reference.py's nodes"""
    node_off = np.zeros(len(reads) + 1, dtype=np.uint64)
    node_off[1:] = np.cumsum([len(r) for r in reads])
    flat = [n for r in reads for n in r]
    nodes = np.array([(n["chunk"], n["pos"], 1 if n["fwd"] else 0, n["qlen"]) for n in flat], dtype=ffi.SETTLE_NODE_DT)
    per_base = [R.per_base(n["cigar"]) for n in flat]
    ops_off = np.zeros(len(flat) + 1, dtype=np.uint64)
    ops_off[1:] = np.cumsum([len(o) for o in per_base])
    ops = np.array([o for node in per_base for o in node], dtype=np.uint8)
    return node_off, nodes, ops, ops_off


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", K.NAMES)
def test_settle_nodes_equals_the_reference(name, mode):
    ref_mode, dev_mode = MODES[mode]
    reads = K.CASES[name]
    want = R.settle(reads, ref_mode)
    got = api.settle_nodes(*flatten(reads), mode=dev_mode)
    stats = got["stats"]
    assert [tuple(int(x) for x in (s["score"], s["total"], s["indel"], s["del_size"])) for s in stats] == want["stats"]
    assert got["status"].tolist() == want["status"] and got["rc"] == want["rc"]
    assert got["n_kept"].tolist() == want["n_kept"]
    assert [o.tolist() for o in got["order"]] == want["order"]
    assert got["keep"].tolist() == want["keep"]
    n_global = sum(len(r) > K.LDS_NODES for r in reads)
    assert api.settle_timing()["n_global"] == n_global and api.settle_timing()["n_reads"] == len(reads)


def test_settle_nodes_refuses_what_it_cannot_read():
    node_off, nodes, ops, ops_off = flatten(K.CASES["random"])
    with pytest.raises(ffi.JtkError) as e:
        api.settle_nodes(node_off, nodes, ops, ops_off, mode=3)
    assert e.value.status == -1
    bad = ops.copy()
    bad[int(ops_off[1]) + 3] = 4   # an op above 3 in the second node of the first read
    out = api.settle_nodes(node_off, nodes, bad, ops_off)
    assert out["rc"] == -6 and out["status"].tolist() == [-1] + [0] * (len(node_off) - 2)
    assert out["order"][0].tolist() == list(range(len(K.CASES["random"][0])))
    empty = api.settle_nodes(np.zeros(3, np.uint64), np.zeros(0, ffi.SETTLE_NODE_DT), np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    assert empty["rc"] == 0 and empty["n_kept"].tolist() == [0, 0] and empty["status"].tolist() == [0, 0]
