"""tests/fill_reference.py against values worked by hand and against the expectations of the reference's own aln_test_gotoh
(deletion_fill.rs:1142-1176), the declarations of jtk_lc_fill_candidates in the header, the ctypes binding and the Rust source,
the argument checks that need no device, and the dataset.py stage.  The GPU tests (tests/test_gpu_fill.py) take the reference's
answers from here, computed once per case."""
import ctypes as C
import functools
import json
import os
import re

import numpy as np
import pytest

import fill_cases as K
import fill_reference as R
from fill_reference import DEL, INS, MATCH
from jtk_amd import api, dataset as D, ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def reference(name):
    c = K.CASES[name]
    return R.fill_candidates(c["reads"], c["target"])


@functools.lru_cache(maxsize=None)
def arrays(name):
    node_off, flat = K.flatten(K.CASES[name]["reads"])
    return node_off, (np.array(flat, dtype=ffi.FILL_NODE_DT) if flat else np.zeros(0, dtype=ffi.FILL_NODE_DT))


def cand_tuples(cands):
    return [(int(c["read"]), int(c["slot"]), int(c["side"]), int(c["chunk"]), int(c["cluster"]), int(c["is_forward"]), int(c["count"]),
             int(c["position"])) for c in cands]


def pair_list(name):
    """every ordered pair of a small case; the first 12 targets against every read of the random family"""
    n = len(K.CASES[name]["reads"])
    return [(t, q) for t in range(min(n, 12)) for q in range(n)]


@functools.lru_cache(maxsize=None)
def pair_reference(name, t, q):
    reads = K.CASES[name]["reads"]
    return R.pair(reads[t], reads[q])


# ---- the three named rules

def test_named_rules():
    assert R.last_max([(0, 5), (1, 7), (2, 7), (3, 1)], key=lambda x: x[1]) == (2, 7)
    assert R.first_equal([4, 9, 9], 9) == 1
    assert [R.div_trunc(a, b) for a, b in ((-7, 2), (7, 2), (-1, 3), (-6, 3), (0, 5))] == [-3, 3, 0, -2, 0]
    assert -7 // 2 == -4     # what the truncating division must not be
    assert R.as_isize((1 << 64) - 8) == -8


# ---- the reference's own unit test, as data: (read, query, score); aln_test_gotoh asserts the scores only

ALN_TEST_GOTOH = [
    ([69, 148, 318, 0], [69, 221, 286, 148, 318], 2),
    ([0], [0, 1, 2, 3, 4], 1),
    ([0, 4], [0, 1, 2, 3, 4], 1),
    ([0, 1, 2, 3, 4], [0, 4], 1),
    ([0, 1], [0, 1, 2, 3, 4], 2),
    ([0, 1, 2, 3, 4], [0, 1], 2),
]


@pytest.mark.parametrize("read,query,score", ALN_TEST_GOTOH)
def test_aln_test_gotoh(read, query, score):
    light = lambda ids: [(c, 0, True, None, None) for c in ids]
    got, ops = R.gotoh(light(read), light(query))
    assert got == score
    assert sum(l for c, l in ops if c != INS) == len(read) and sum(l for c, l in ops if c != DEL) == len(query)


# ---- values worked by hand.  Default nodes are 100 bases long and 10 apart: node i spans [110 i, 110 i + 100).

def test_identical_reads():
    ref = reference("identical")
    assert ref == dict(coverage=[2, 2, 2, 0, 2, 2, 2, 0], ins_thr=[0, 0], cand_off=[0, 0, 0], cands=[])   # mean_cov 6 / 4 = 1, / 5 = 0
    assert pair_reference("identical", 0, 1) == {"dir": 1, "score": 3, "pass": 1, "ops": [(MATCH, 3)]}


def test_middle_insertions():
    # target A B; query A X B: X starts 10 after A's end (head: 100 + 10)
    assert reference("middle_insertion_1")["cands"] == [(0, 1, 0, K.X, 0, 1, 1, 110)]
    # query A X Y B: Y ends 10 in front of B (tail: B's start 110 - 10); the longer query covers the target's two nodes too
    two = reference("middle_insertion_2")
    assert two["cands"] == [(0, 1, 0, K.X, 0, 1, 1, 110), (0, 1, 1, K.Y, 0, 1, 1, 100)]
    assert two["coverage"] == [2, 2, 0, 2, 1, 1, 2, 0] and two["cand_off"] == [0, 2, 2]
    # query A X Y P B: first to head, last to tail, the middle one nowhere
    assert reference("middle_insertion_3")["cands"] == [(0, 1, 0, K.X, 0, 1, 1, 110), (0, 1, 1, K.P, 0, 1, 1, 100)]
    assert pair_reference("middle_insertion_3", 0, 1)["ops"] == [(MATCH, 1), (INS, 3), (MATCH, 1)]
    # seen from the query, the target lacks nodes: deletions add nothing but skip their slots
    assert pair_reference("middle_insertion_3", 1, 0) == {"dir": 1, "score": 1, "pass": 1, "ops": [(MATCH, 1), (DEL, 3), (MATCH, 1)]}


def test_insertions_at_the_ends():
    # X Y A B on A B: only Y, in the tail list of slot 0; Y ends 10 in front of A, A starts at 0: max(0 - 10, 0)
    assert reference("leading_insertion")["cands"] == [(0, 0, 1, K.Y, 0, 1, 1, 0)]
    # A B X Y on A B: position == n, the subtraction wraps, the general arm runs: X to the head list of slot 2 (B ends at 210,
    # X starts 10 later); Y goes to the tail list of slot 2, which check_insertion_tail never opens
    assert reference("trailing_insertion")["cands"] == [(0, 2, 0, K.X, 0, 1, 1, 220)]


def test_the_shadowed_length():
    # Ins(2) at slot 1: n = 3 -> 2 * 1 + 1 == 3, head only; n = 4 -> head and tail
    assert reference("half_arm_n3")["cands"] == [(0, 1, 0, K.X, 0, 1, 1, 110)]
    assert reference("half_arm_n4")["cands"] == [(0, 1, 0, K.X, 0, 1, 1, 110), (0, 1, 1, K.Y, 0, 1, 1, 100)]


def test_reverse_query_and_tie():
    # the query is A X Y B C (gaps of 17) from the other strand: as aligned, X again follows A by 17; n = 3 keeps the head only
    assert pair_reference("reverse_query", 0, 1) == {"dir": 0, "score": 2, "pass": 1, "ops": [(MATCH, 1), (INS, 2), (MATCH, 2)]}
    assert reference("reverse_query")["cands"][0] == (0, 1, 0, K.X, 0, 1, 1, 117)
    assert pair_reference("direction_tie", 0, 1)["dir"] == 1


def test_verdicts():
    assert pair_reference("cluster_mismatch", 0, 1) == {"dir": 1, "score": 1, "pass": 1, "ops": [(MATCH, 2), (INS, 1), (MATCH, 2)]}
    score = pair_reference("reject_score", 0, 1)
    assert (score["dir"], score["score"], score["pass"]) == (1, 0, 0)
    matched = pair_reference("reject_matched", 0, 1)
    assert (matched["score"], matched["pass"]) == (1, 0) and sum(l for c, l in matched["ops"] if c == MATCH) == 1
    adjacent = pair_reference("reject_ins_del", 0, 1)
    assert adjacent["score"] >= 1 and sum(l for c, l in adjacent["ops"] if c == MATCH) >= 2 and adjacent["pass"] == 0
    assert not R.is_proper(adjacent["ops"])
    for name in ("reject_score", "reject_matched", "reject_ins_del"):    # only the self pairs count
        assert set(reference(name)["coverage"]) == {0, 1} and reference(name)["cands"] == []
    assert pair_reference("empty_query", 0, 1)["dir"] == -1 and pair_reference("empty_query", 1, 0)["dir"] == -1
    assert pair_reference("one_node_target", 0, 1) == {"dir": 1, "score": 1, "pass": 1, "ops": [(INS, 1), (MATCH, 1), (INS, 1)]}


def test_tandem_tie_breaks():
    # A A A (rows) against A A: the end-cell chain takes the LAST maximum, (3, 2) over (2, 2): the deletion leads
    assert pair_reference("tandem_short", 0, 1) == {"dir": 1, "score": 2, "pass": 1, "ops": [(DEL, 1), (MATCH, 2)]}
    assert pair_reference("tandem_short", 1, 0) == {"dir": 1, "score": 2, "pass": 1, "ops": [(INS, 1), (MATCH, 2)]}
    assert reference("tandem_short")["coverage"] == [1, 2, 2, 0, 2, 2, 0]


def test_offsets():
    # -3 and -4: (-7) / 2 = -3; the head lands at 100 - 3, the tail at 0 - (-3).  Floored, they would be 96 and 4.
    cands = reference("offset_truncates")["cands"]
    assert (0, 1, 0, K.X, 0, 1, 2, 97) in cands and (0, 0, 1, K.Y, 0, 1, 2, 3) in cands
    assert reference("negative_head")["cands"] == [(0, 1, 0, K.X, 0, 1, 1, -8)]
    assert reference("tail_clamped")["cands"] == [(0, 0, 1, K.X, 0, 1, 1, 0)]
    none = reference("offsets_all_none")     # X of read 1 and Y of read 2 end their reads: no after_offset, and slot n anyway
    assert none["cands"] == [(0, 2, 0, K.X, 0, 1, 2, 220), (1, 3, 0, K.Y, 0, 1, 1, 330)]


@pytest.mark.parametrize("mean,thr", [(4, 0), (5, 1), (9, 1), (10, 2)])
def test_mean_cov_and_threshold(mean, thr):
    ref = reference("mean_cov_%d" % mean)
    total = len(K.CASES["mean_cov_%d" % mean]["reads"])
    assert ref["coverage"][:4] == [total, total, total, 0] and 3 * total // 4 == mean and ref["ins_thr"][0] == thr
    want = [(0, 1, 0, K.X, 0, 1, 2, 110)] + ([(0, 1, 0, K.Y, 0, 1, 1, 110)] if thr <= 1 else [])    # X twice, Y once
    assert ref["cands"] == want
    assert not any(ref["coverage"][4:]) and not any(ref["ins_thr"][1:])      # the mask


def test_mask_and_empty_reads():
    ref = reference("target_mask")
    assert ref["cand_off"][1] == 0 and ref["cand_off"][2] == ref["cand_off"][3] and {c[0] for c in ref["cands"]} == {1, 3}
    assert ref["coverage"][:4] == [0, 0, 0, 0]
    empty = reference("empty_query")
    assert empty["coverage"] == [2, 2, 0, 0, 2, 1, 2, 0, 0] and empty["cand_off"] == [0, 1, 1, 1, 1]


def test_random_family_has_candidates_on_both_sides():
    reads = K.CASES["random_family"]["reads"]
    assert len(reads) == 200 and len({n[0] for r in reads for n in r}) <= 40
    assert {n[2] for r in reads for n in r} == {True, False}
    cands = reference("random_family")["cands"]
    assert any(c[2] == 0 for c in cands) and any(c[2] == 1 for c in cands)
    assert set(reference("random_family")["ins_thr"]) == {0, 1, 2}


def test_long_cases_align_and_cross_the_boundary():
    need = lambda n, m: 24 * (m + 1) + 4 * (n + m + 2) + n * ((m + 1) // 2)      # bytes of one pair
    for name in ("long_65", "long_130", "lds_boundary_99", "lds_boundary_100"):
        assert pair_reference(name, 0, 1)["pass"] == 1 and pair_reference(name, 1, 0)["pass"] == 1
    n99, n100 = (len(K.CASES["lds_boundary_%d" % n]["reads"][0]) for n in (99, 100))
    assert need(n99, n99) <= 8192 < need(n100, n100)


# ---- declarations

def test_declarations_agree(jtk_lib):
    header = open(os.path.join(ROOT, "include", "jtk_lc.h")).read()
    debug = open(os.path.join(ROOT, "include", "jtk_lc_debug.h")).read()
    rust = open(os.path.join(ROOT, "rust", "gpu_ffi.rs")).read()
    assert "jtk_lc_fill_candidates" in ffi.EXPORTED_SYMBOLS and "jtk_lc_debug_fill_pairs" in ffi.DEBUG_SYMBOLS
    for name, text in (("jtk_lc_fill_candidates", header), ("jtk_lc_debug_fill_pairs", debug)):
        f = getattr(ffi.lib(), name)
        decl = re.search(r"JTK_LC_API int %s\((.*?)\);" % name, text, flags=re.S).group(1)
        decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
        assert f.restype is C.c_int and len(f.argtypes) == len(decl.split(","))
    assert "pub fn jtk_lc_fill_candidates(" in rust and "fill_candidates_gpu" in open(os.path.join(ROOT, "rust", "gpu_shim.rs")).read()
    for c_name, r_name, dt in (("jtk_fill_node", "JtkFillNode", ffi.FILL_NODE_DT), ("jtk_fill_cand", "JtkFillCand", ffi.FILL_CAND_DT)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s_t;" % (c_name, c_name), header, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        c_fields = [(n.strip(), decl.split()[0]) for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
        r_body = re.search(r"pub struct %s \{(.*?)\}" % r_name, rust, flags=re.S).group(1)
        r_fields = re.findall(r"pub ([a-z_0-9]+)\s*:\s*([a-z0-9]+)", r_body)
        kinds = {"uint64_t": ("u64", "<u8"), "uint32_t": ("u32", "<u4"), "int64_t": ("i64", "<i8")}
        assert [n for n, _ in c_fields] == [n for n, _ in r_fields] == list(dt.names)
        for (n, ct), (_, rt) in zip(c_fields, r_fields):
            assert kinds[ct] == (rt, dt[n].str), n
    assert ffi.FILL_NODE_DT.itemsize == 32 and ffi.FILL_CAND_DT.itemsize == 48
    for needle in ("deletion_fill.rs:642-698", "deletion_fill.rs:1003-1030", "2 position + 1 == n"):
        assert needle in header, needle
    assert ffi.lib().jtk_lc_version() == 2
    assert "fill.hip" in __import__("jtk_amd.build", fromlist=["SOURCES"]).SOURCES


# ---- argument checks: decided before a device is looked for

def raw_call(node_off, nodes, cov=True):
    n_reads = len(node_off) - 1
    coverage, thr = np.full(len(nodes) + n_reads + 1, 7, dtype=np.uint32), np.full(n_reads + 1, 7, dtype=np.uint32)
    off, need = np.full(n_reads + 1, 7, dtype=np.uint64), C.c_size_t(7)
    rc = ffi.lib().jtk_lc_fill_candidates(n_reads, ffi.u64p(node_off), nodes.ctypes.data if len(nodes) else None, None,
                                          ffi.u32p(coverage) if cov else None, ffi.u32p(thr), ffi.u64p(off), None, 0, C.byref(need), 0)
    assert (coverage == 7).all() and (thr == 7).all() and (off == 7).all() and need.value == 7
    return rc


def test_argument_checks(jtk_lib):
    L = ffi.lib()
    assert L.jtk_lc_fill_candidates(0, None, None, None, None, None, None, None, 0, None, 0) == -1
    assert L.jtk_lc_debug_fill_pairs(0, None, None, 0, None, None, None, None, None, None, None, 0, None, 0) == -1
    node_off, nodes = arrays("identical")
    assert raw_call(node_off, nodes, cov=False) == -1
    assert raw_call(np.array([1, 3, 6], dtype=np.uint64), nodes) == -1          # does not start at 0
    assert raw_call(np.array([0, 4, 3, 6], dtype=np.uint64), nodes) == -1       # decreases
    # a read of 65,536 nodes: the status only; 65,535 pass this check
    big = np.zeros(65536, dtype=ffi.FILL_NODE_DT)
    assert raw_call(np.array([0, 65536], dtype=np.uint64), big) == -3
    assert "65,535" in L.jtk_lc_last_error().decode()
    with pytest.raises(ValueError):
        api.fill_candidates(np.array([0, 2], dtype=np.uint64), nodes)
    with pytest.raises(ValueError):
        api.fill_candidates(node_off, nodes, target=[1])
    with pytest.raises(ffi.JtkError) as e:     # a pair that names a read that is not there
        api.fill_pairs(node_off, nodes, [0], [2])
    assert e.value.status == -1


def test_no_cpu_path(jtk_lib):
    if ffi.lib().jtk_lc_device_ok(0) == 1:
        return   # a device is present: tests/test_gpu_fill.py runs the entry points
    node_off, nodes = arrays("identical")
    for call in (lambda: api.fill_candidates(node_off, nodes), lambda: api.fill_pairs(node_off, nodes, [0], [1])):
        with pytest.raises(ffi.JtkError) as e:      # an error, never a host computation
            call()
        assert e.value.status == -2
    assert raw_call(np.array([0, 65535], dtype=np.uint64), np.zeros(65535, dtype=ffi.FILL_NODE_DT)) == -2


# ---- the dataset.py stage, the device call stubbed by the reference

def tiny_dataset():
    def node(chunk, pos, cigar, cluster=0, fwd=True):
        return {"chunk": chunk, "cluster": cluster, "is_forward": fwd, "position_from_start": pos, "cigar": cigar, "seq": "", "posterior": []}
    # query_length counts M and I: 90M10I5D = 100 read bases
    return {"encoded_reads": [
        {"id": 5, "nodes": [node(K.A, 0, "100M"), node(K.B, 110, "90M10I5D")]},
        {"id": 9, "nodes": [node(K.A, 0, "95M5I"), node(K.X, 110, "100M3D"), node(K.Y, 220, "100M"), node(K.B, 330, "100M")]},
        {"id": 2, "nodes": []}]}


def test_dataset_stage(monkeypatch, tmp_path):
    seen = {}

    def fake(node_off, nodes, target=None, device=0):
        reads = [[tuple(int(x) for x in nodes[e]) for e in range(int(node_off[r]), int(node_off[r + 1]))] for r in range(len(node_off) - 1)]
        seen["reads"], seen["target"] = reads, None if target is None else list(target)
        ref = R.fill_candidates([[(c, k, bool(f), q, p) for (c, k, f, q, p) in r] for r in reads], target)
        cands = np.array([c[:3] + (c[5], c[3], c[4], c[6], 0, c[7]) for c in ref["cands"]], dtype=ffi.FILL_CAND_DT)
        return dict(coverage=np.array(ref["coverage"], dtype=np.uint32), ins_thr=np.array(ref["ins_thr"], dtype=np.uint32),
                    cand_off=np.array(ref["cand_off"], dtype=np.uint64), cands=cands)
    monkeypatch.setattr(api, "fill_candidates", fake)
    monkeypatch.setattr(api, "trim_cache", lambda device=0: None)
    ds = tiny_dataset()
    report = D.fill_candidates(ds)
    assert seen["reads"][0] == [(K.A, 0, 1, 100, 0), (K.B, 0, 1, 100, 110)] and seen["reads"][2] == [] and seen["target"] is None
    assert seen["reads"][1] == K.flatten([K.CASES["middle_insertion_2"]["reads"][1]])[1]
    assert [r["id"] for r in report] == [5, 9]
    assert report[0] == {"id": 5, "ins_thr": 0, "coverage": [2, 2, 0], "candidates": [
        {"slot": 1, "side": "head", "chunk": K.X, "cluster": 0, "is_forward": True, "count": 1, "position": 110},
        {"slot": 1, "side": "tail", "chunk": K.Y, "cluster": 0, "is_forward": True, "count": 1, "position": 100}]}
    assert report[1]["candidates"] == [] and ds == tiny_dataset()
    assert [r["id"] for r in D.fill_candidates(ds, alive=[9])] == [9] and seen["target"] == [0, 1, 0]
    src, dst = tmp_path / "in.json", tmp_path / "out.json"
    src.write_text(json.dumps(ds))
    assert D.main(["--stage", "fill_candidates", str(src), str(dst)]) == 0
    assert json.loads(dst.read_text()) == report
