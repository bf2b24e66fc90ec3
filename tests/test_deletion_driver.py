"""dataset._fill_round, the driver of one round of correct_deletion, on the CPU: the three device calls it makes are replaced by
the Python references of the same primitives, fed with PLANTED candidates, and its outcome is compared with
tests/deletion_reference.py's fill_round on the same candidates.  The case the data of tests/deletion_fixture.py does not show
by itself: one slot that carries the same (chunk, cluster, direction) as head and as tail candidate.  The reference tries the head
first, and a head candidate that fails is a failed trial (deletion_fill.rs:325) before the slot's tail candidates are filtered
(:328): the tail candidate is then never tried, however good its window."""
import copy

import numpy as np
import pytest

import deletion_reference as DR
import encode_reference as E
import fill_reference as F
import purge_reference as PR
import settle_reference as S
from deletion_fixture import fixture
from jtk_amd import api, dataset as D, ffi

READ, SLOT, KEY = 2, 2, (12, 0, 1)      # read 2 lacks its node of chunk 12 between its second and third node


def planted(ds, sides):
    """candidates for read 2, slot 2: `sides` maps side (0 head, 1 tail) to a position"""
    return [(READ, SLOT, side, KEY[0], KEY[1], KEY[2], 3, pos) for side, pos in sorted(sides.items())]


def stub_calls(monkeypatch, ds, cands):
    n_reads = len(ds["encoded_reads"])
    off = [0] * (READ + 1) + [len(cands)] * (n_reads - READ)
    monkeypatch.setattr(F, "fill_candidates", lambda reads, target=None: {"cands": cands, "cand_off": off})
    records = np.array([c[:3] + (c[5], c[3], c[4], c[6], 0, c[7]) for c in cands], dtype=ffi.FILL_CAND_DT)
    monkeypatch.setattr(api, "fill_candidates", lambda node_off, nodes, target=None, device=0: {"cands": records, "cand_off": np.array(off, dtype=np.uint64)})
    tried = []

    def encode_nodes(trials, read_bases, cons_bases, chunk_bases, device=0, raise_on_trial_failure=True):
        result, ops, ops_off = np.zeros(len(trials), dtype=ffi.ENCODE_RESULT_DT), [], [0]
        for t, tr in enumerate(trials):
            tried.append((int(tr["start"]), int(tr["end"])))
            res = E.encode_node(bytes(read_bases[int(tr["read_off"]):]), int(tr["start"]), int(tr["end"]), bool(tr["is_forward"]),
                                bytes(cons_bases[int(tr["cons_off"]):int(tr["cons_off"]) + int(tr["cons_len"])]),
                                bytes(chunk_bases[int(tr["chunk_off"]):int(tr["chunk_off"]) + int(tr["chunk_len"])]), float(tr["sim_thr"]))
            for key in ("status", "verdict", "trim_head", "trim_tail", "position_from_start", "score"):
                result[t][key] = res[key]
            ops += list(res["ops"])
            ops_off.append(len(ops))
        return dict(result=result, ops=np.array(ops, dtype=np.uint8), ops_off=np.array(ops_off, dtype=np.uint64), rc=0)

    def settle_nodes(node_off, nodes, ops, ops_off, mode=1, device=0):
        reads = []
        for r in range(len(node_off) - 1):
            reads.append([dict(chunk=int(n["chunk"]), pos=int(n["position_from_start"]), fwd=bool(n["is_forward"]), qlen=int(n["query_len"]),
                               cigar=DR.runs(D.ops_to_cigar(ops[int(ops_off[e]):int(ops_off[e + 1])])))
                          for e, n in enumerate(nodes) if int(node_off[r]) <= e < int(node_off[r + 1])])
        out = S.settle(reads, S.BY_CHUNK_POS)
        return dict(order=[np.array(o) for o in out["order"]], rc=out["rc"])

    monkeypatch.setattr(api, "encode_nodes", encode_nodes)
    monkeypatch.setattr(api, "settle_nodes", settle_nodes)
    return tried


def rates(ds):
    pds = DR.as_purge_ds(ds)
    num, length, _ = PR.node_errors(pds)
    fit = PR.estimate_error_rate(pds, num, length, PR.error_quantile(num, length, DR.TAKE_THR))
    read_err = {r["id"]: fit["read_err"][i] for i, r in enumerate(ds["encoded_reads"])}
    return read_err, fit["chunk_err"], fit["median"]


CASES = {"head_fails_then_tail_is_not_tried": ({0: "bad", 1: "good"}, False, 2), "tail_alone_is_taken": ({1: "good"}, True, 1),
         "head_is_taken_and_tail_too": ({0: "good", 1: "good"}, True, 2), "both_fail": ({0: "bad", 1: "bad"}, False, 2)}


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_round_on_planted_candidates(monkeypatch, name):
    sides, inserted, n_tried = CASES[name]
    ds = copy.deepcopy(fixture())
    nodes = ds["encoded_reads"][READ]["nodes"]
    assert [n["chunk"] for n in nodes] == [10, 11, 13, 14]
    gap = (nodes[1]["position_from_start"] + D.query_length(nodes[1]) + 50, nodes[2]["position_from_start"] - 50)   # where chunk 12 lies
    position = {(0, "good"): gap[0], (1, "good"): gap[1], (0, "bad"): 0, (1, "bad"): 230}        # bad: a window on chunk 10 instead
    cands = planted(ds, {side: position[side, kind] for side, kind in sides.items()})
    tried = stub_calls(monkeypatch, ds, cands)
    read_err, chunk_err, stddev = rates(ds)
    ref_ds, ref_state = copy.deepcopy(ds), [{"alive": True, "failed": set()} for _ in ds["encoded_reads"]]
    ref_new = DR.fill_round(ref_ds, ref_state, DR.take_consensus_sequence(ds), read_err, chunk_err, stddev)
    assert (12 in [n["chunk"] for n in ref_ds["encoded_reads"][READ]["nodes"]]) == inserted       # the reference by itself
    state = [{"alive": True, "failed": set()} for _ in ds["encoded_reads"]]
    consensi = {k: v.decode() for k, v in DR.take_consensus_sequence(ds).items()}
    flat_err = {(cid, cl): x for cid, xs in chunk_err.items() for cl, x in enumerate(xs)}
    new = D._fill_round(ds, state, consensi, read_err, flat_err, stddev, 0)
    assert len(tried) == n_tried           # one encode call makes every window; the pick then leaves out what the head has failed
    assert new == ref_new and ds == ref_ds
    for mine, theirs in zip(state, ref_state):
        assert mine["alive"] == theirs["alive"]
        assert {(s, (k[0], k[1], bool(k[2]))) for s, k in mine["failed"]} == {(s, (k[0], k[1], bool(k[2]))) for s, k in theirs["failed"]}
    if name == "head_fails_then_tail_is_not_tried":
        assert state[READ]["failed"] == {(SLOT, (12, 0, True))} and not state[READ]["alive"]
