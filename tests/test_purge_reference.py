"""The purge entry points without a device: the Python reference (tests/purge_reference.py) on the problems of
tests/purge_cases.py, a fit small enough to follow by hand, the rebuild of the reads, the declarations, the argument checks and the
dataset.py stage with the device call stubbed by the reference."""
import copy
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import purge_cases as K
import purge_reference as R
from jtk_amd import api, dataset as D, ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


def reference(name):
    """every reference answer on a case, computed once and shared by every test (GPU module included)"""
    if name not in _cache:
        ds = K.CASES[name]["ds"]
        num, length, status = R.node_errors(ds)
        res = dict(num=num, length=length, status=status, purge=R.purge(ds), quantile={}, fit=None)
        for q in (0.0, 0.5, 1.0):
            try:
                res["quantile"][q] = R.error_quantile(num, length, q)
            except R.ReferencePanic as p:
                res["quantile"][q] = p
        res["fallback"] = K.CASES[name].get("fallback", res["quantile"][0.5] if isinstance(res["quantile"][0.5], float) else 0.1)
        try:
            res["fit"] = R.estimate_error_rate(ds, num, length, res["fallback"])
            res["fit_status"] = 0
        except R.ReferencePanic as p:
            res["fit_status"] = p.status
        _cache[name] = res
    return _cache[name]


# ---- the cases

@pytest.mark.parametrize("name", K.NAMES)
def test_cases_go_where_they_were_built_to_go(name):
    case, ref = K.CASES[name], reference(name)
    assert {i: s for i, s in enumerate(ref["status"]) if s} == case.get("node_status", {})
    if "fit_status" in case:
        assert ref["fit_status"] == case["fit_status"]
    if "n_iter" in case:
        assert case["n_iter"][0] <= ref["fit"]["n_iter"] <= case["n_iter"][1]
    if "purge_status" in case:
        assert ref["purge"]["status"] == case["purge_status"]
    if "flags" in case:
        off, got = ref["purge"]["chunk_err_off"], ref["purge"]["diverged"]
        assert {c["id"]: got[off[i]:off[i + 1]] for i, c in enumerate(case["ds"]["chunks"])} == case["flags"]
        assert ref["purge"]["purged"] == sorted(cid for cid, xs in case["flags"].items() if any(xs))


def test_cases_cover_the_corners_they_name():
    # the column walk: every length around the 64-op steps, and more nodes than one pass of the grid
    lens = reference("columns")["length"]
    assert set(lens) >= {1, 63, 64, 65, 127, 128, 129, 301} and len(reference("beyond_one_pass")["num"]) > K.WAVES_PER_PASS
    by_len = dict(zip(lens, reference("columns")["num"]))
    assert by_len[200] == 4 and by_len[129] == 128                  # the four edge mismatches; 64 Ins + 64 Del + a match
    n = len(lens)
    assert (reference("columns")["num"][n - 3], lens[n - 3]) == (0, 70) and (reference("columns")["num"][n - 2], lens[n - 2]) == (70, 70)
    assert reference("columns_bad")["status"][11] == 0 and reference("columns_bad")["num"][11] == 64
    # the fit
    assert reference("fit_one_pass")["fit"]["n_iter"] == 1 and reference("fit_many_passes")["fit"]["n_iter"] >= 10
    neg = reference("fit_negative_slot")
    assert neg["fit"]["chunk_err"][5] == [0.0] and all(a / b < neg["fallback"] for a, b, nd in zip(
        neg["num"], neg["length"], (nd for r in K.CASES["fit_negative_slot"]["ds"]["reads"] for nd in r["nodes"])) if nd["chunk"] == 5)
    corners = reference("fit_empty_corners")["fit"]
    assert corners["chunk_err"][8] == [] and corners["chunk_err"][10] == [0.0, 0.0] and corners["chunk_err"][12][1] == 0.0
    assert corners["read_err"][1] != corners["read_err"][1] and [c["id"] for c in K.CASES["fit_empty_corners"]["ds"]["chunks"]] == [12, 8, 9, 10]
    assert K.order_shows(K.CASES["fit_real_valued"]["ds"]) and len(K.CASES["fit_real_valued"]["ds"]["reads"]) == 41
    # the purge
    p = reference("purge_all_flagged")["purge"]
    off = p["chunk_err_off"][1]
    assert all(x > R.THR for x in p["chunk_err"][off:off + 3]) and p["diverged"] == [0] * 6 and p["cluster_num"] == [2, 3, 1]
    p = reference("purge_middle_of_three")["purge"]
    assert p["cluster_num"] == [2, 2, 1] and 2 in [n["cluster"] for r in K.CASES["purge_middle_of_three"]["ds"]["reads"] for n in r["nodes"]]
    assert max(c for c, n in zip(p["cluster"], (n for r in K.CASES["purge_middle_of_three"]["ds"]["reads"] for n in r["nodes"]))
               if n["chunk"] == 31 and n["cluster"] != 1) == 1
    assert 0 in p["post_keep"] and 0 in p["keep"]
    case = K.CASES["purge_loses_first_middle_last"]["ds"]
    after = R.written_back(case, reference("purge_loses_first_middle_last")["purge"])
    assert len(after["reads"]) == len(case["reads"]) - 1 and after["reads"][0]["id"] == case["reads"][1]["id"]
    assert [n["chunk"] for n in after["reads"][0]["nodes"]] == [30, 33, 32, 30] and [e["offset"] for e in after["reads"][0]["edges"]] == [-7, -10, 20]
    assert len(after["reads"][0]["leading_gap"]) == 3 + 2 + 200 + 2 and len(after["reads"][0]["trailing_gap"]) == 200 + 2


def test_a_fit_small_enough_to_follow_by_hand():
    """two reads, two chunks of one cluster: read 0 = (chunk 1: 1 / 10, chunk 2: 3 / 10), read 1 = (chunk 1: 2 / 10), fallback 0.2.
    First pass: chunk 1 adds (0.1 - 0.2) + (0.2 - 0.2) < 0 and is clamped to 0; chunk 2 is (0.3 - 0.2) / 1.1; read 0 is
    ((0.1 - 0) + (0.3 - chunk 2)) / 2, read 1 is 0.2.  Chunk 1 stays 0 and read 1 stays 0.2 from then on; chunk 2 and read 0 move
    towards 1 / 6 and 7 / 60, and the twelfth pass changes the residual by less than 0.00001."""
    ds = dict(reads=[dict(id=0, nodes=[dict(chunk=1, cluster=0), dict(chunk=2, cluster=0)]), dict(id=1, nodes=[dict(chunk=1, cluster=0)])],
              chunks=[dict(id=1, cluster_num=1), dict(id=2, cluster_num=1)])
    c2_1 = (0.3 - 0.2) / 1.1
    assert c2_1 == 0.09090909090909088 and ((0.1 - 0.0) + (0.3 - c2_1)) / 2 == 0.15454545454545454
    c2, r0, passes = 0.0, 0.2, 0
    x, y = 0.1 - 0.2 - 0.0, 0.3 - 0.2 - 0.0
    current = (x * x + y * y) + 0.0
    assert current == 0.019999999999999997
    while True:
        passes += 1
        s2 = 0.3 - r0
        c2 = (s2 if s2 > 0.0 else 0.0) / 1.1
        r0 = (0.1 + (0.3 - c2)) / 2
        x, y = 0.1 - r0 - 0.0, 0.3 - r0 - c2
        resid = (x * x + y * y) + c2 * c2          # read 1's term and chunk 1's square are 0
        if abs(current - resid) < 0.00001:
            break
        current = resid
    assert (passes, c2, r0) == (12, 0.1666537015455033, 0.11667314922724835)
    fit = R.estimate_error_rate(ds, [1, 3, 2], [10, 10, 10], 0.2)
    assert fit["n_iter"] == 12 and fit["chunk_err"] == {1: [0.0], 2: [c2]} and fit["read_err"] == [r0, 0.2]
    x = 0.3 - (c2 + r0)      # the three squared residuals are (0.1 - r0)^2 = x^2 (to rounding) and 0: the middle one is the median
    sq = sorted([(0.1 - (0.0 + r0)) * (0.1 - (0.0 + r0)), x * x, 0.0])
    assert fit["median"] == math.sqrt(sq[1])


def test_quantile_cases():
    for name, (num, length) in K.QUANTILE.items():
        rates = sorted(a / b for a, b in zip(num, length))
        assert R.error_quantile(num, length, 0.0) == rates[0] and R.error_quantile(num, length, 1.0) == rates[-1]
        assert R.error_quantile(num, length, 0.5) == rates[len(rates) // 2]
    assert R.error_quantile(*K.QUANTILE["ties"], 0.5) == 0.1 and R.error_quantile(*K.QUANTILE["even"], 0.5) == 5 / 17
    for bad in ((([], []), 0.5), (([1], [0]), 0.5), (([1], [2]), 1.5), (([1], [2]), -0.1)):
        with pytest.raises(R.ReferencePanic):
            R.error_quantile(*bad[0], bad[1])


# ---- nodes_to_encoded_read

def dataset_json(ds):
    """a DataSet JSON (every field of the wire format) around a case that carries sequences"""
    reads, raw = [], []
    for read in ds["reads"]:
        nodes = [dict(position_from_start=n["position_from_start"], chunk=n["chunk"], cluster=n["cluster"], seq=n["seq"],
                      is_forward=bool(n["is_forward"]), cigar=n["cigar"], posterior=list(n["posterior"])) for n in read["nodes"]]
        built = R.nodes_to_encoded_read(read["id"], nodes, read["seq"]) or dict(leading_gap=read["seq"], trailing_gap="", edges=[])
        reads.append(dict(id=read["id"], original_length=len(read["seq"]), leading_gap=built["leading_gap"], trailing_gap=built["trailing_gap"],
                          edges=built["edges"], nodes=nodes))
        raw.append(dict(name="r%d" % read["id"], desc="", id=read["id"], seq=read["seq"]))
    hmm = {k: float(getattr(ffi.default_hmm(), k)) for k in D.SCHEMA["HMMParam"][:9]}
    hmm.update(mat_emit=list(ffi.default_hmm().mat_emit), ins_emit=list(ffi.default_hmm().ins_emit))
    return dict(input_file="x.fa", masked_kmers=dict(k=12, thr=10), coverage={"Protected": 10.0}, raw_reads=raw, hic_pairs=[],
                selected_chunks=[dict(id=c["id"], seq=c["seq"], cluster_num=c["cluster_num"], copy_num=c["copy_num"], score=c["score"])
                                 for c in ds["chunks"]],
                encoded_reads=reads, hic_edges=[], read_type="CCS", model_param=dict(forward=hmm, reverse=copy.deepcopy(hmm)),
                error_rate={k: 0.01 for k in D.SCHEMA["ErrorRate"]}, processed_stages=[dict(stage_name="local_clustering", arg=[])])


PURGE_OK = [n for n in K.NAMES if n.startswith("purge_") and K.CASES[n]["purge_status"] == 0]


@pytest.mark.parametrize("name", PURGE_OK + ["fit_many_passes"])
def test_rebuilt_reads_recover_their_raw_reads(name):
    ds = K.CASES[name]["ds"]
    before = dataset_json(ds)
    D.sanity_check(before)                       # the cases are laid out like real data
    for built, read in zip((r for r in before["encoded_reads"]), ds["reads"]):
        assert D.recover_raw_read(built) == read["seq"]
    after = R.written_back(ds, reference(name)["purge"])
    for read in after["reads"]:
        assert D.recover_raw_read(read) == read["seq"], read["id"]
    if name == "purge_loses_first_middle_last":
        assert any(e["offset"] < 0 for r in after["reads"] for e in r["edges"])


# ---- declarations

ENTRIES = (("jtk_lc_node_errors", 15), ("jtk_lc_error_quantile", 6), ("jtk_lc_estimate_error_rate", 15), ("jtk_lc_purge_diverged", 27))


def test_symbols_are_declared_exported_and_bound(jtk_lib):
    header = open(os.path.join(ROOT, "include", "jtk_lc.h")).read()
    rust = open(os.path.join(ROOT, "rust", "gpu_ffi.rs")).read()
    for name, n_args in ENTRIES:
        assert name in ffi.EXPORTED_SYMBOLS and hasattr(jtk_lib, name)
        f = getattr(ffi.lib(), name)
        assert f.restype is C.c_int and len(f.argtypes) == n_args
        decl = re.search(r"JTK_LC_API int %s\((.*?)\);" % name, header, flags=re.S).group(1)
        assert len(decl.split(",")) == n_args
        assert "pub fn %s(" % name in rust
    for needle in ("purge_diverged.rs:238-322", "estimate_error_rate.rs:37-133", "determine_chunks.rs:806-823", "definitions/src/lib.rs:773-813"):
        assert needle in header, needle
    assert ffi.lib().jtk_lc_version() == 2
    assert "jtk_lc_purge_diverged" in open(os.path.join(ROOT, "rust", "gpu_shim.rs")).read()
    assert "purge.hip" in __import__("jtk_amd.build", fromlist=["SOURCES"]).SOURCES


def test_entry_points_reject_null_arguments(jtk_lib):
    L = ffi.lib()
    assert L.jtk_lc_node_errors(0, None, None, 0, None, None, None, None, None, None, None, None, None, None, 0) == -1
    assert L.jtk_lc_error_quantile(1, None, None, 0.5, None, 0) == -1
    assert L.jtk_lc_estimate_error_rate(0, None, None, None, None, 0, None, 0.1, None, None, None, 0, None, None, 0) == -1
    assert L.jtk_lc_purge_diverged(0, None, None, 0, 0, None, None, None, None, None, None, None, 0.1, None, None, 0, None, None, None, None,
                                   None, 0, None, None, None, None, 0) == -1
    # arguments that no device would accept either, refused before a device is looked for
    one = np.ones(1, dtype=np.uint32)
    out = C.c_double(7.0)
    for n, q, length in ((0, 0.5, one), (1, 1.5, one), (1, float("nan"), one), (1, 0.5, np.zeros(1, dtype=np.uint32))):
        assert L.jtk_lc_error_quantile(n, ffi.u32p(one), ffi.u32p(length), q, C.byref(out), 0) == -1 and out.value == 7.0
    prob = R.flatten(K.CASES["purge_middle_of_three"]["ds"])
    twice = prob["chunks"].copy()
    twice["id"][1] = twice["id"][0]
    with pytest.raises(ffi.JtkError) as e:
        api.purge_diverged(prob["node_off"], prob["nodes"], prob["n_post"], twice, prob["seqs"])
    assert e.value.status == -1 and "repeat" in str(e.value)
    with pytest.raises(ffi.JtkError) as e:     # a posterior that lies outside the array it indexes
        api.purge_diverged(prob["node_off"], prob["nodes"], prob["n_post"] - 1, prob["chunks"].copy(), prob["seqs"])
    assert e.value.status == -1


def test_entry_points_have_no_cpu_path(jtk_lib):
    if ffi.lib().jtk_lc_device_ok(0) == 1:
        return   # a device is present: tests/test_gpu_purge.py runs the entry points
    prob = R.flatten(K.CASES["purge_middle_of_three"]["ds"])
    ref = reference("purge_middle_of_three")
    chunks = prob["chunks"].copy()
    calls = (lambda: api.node_errors(prob["node_off"], prob["nodes"], chunks, prob["seqs"]),
             lambda: api.error_quantile(ref["num"], ref["length"], 0.5),
             lambda: api.estimate_error_rate(prob["node_off"], prob["nodes"], ref["num"], ref["length"], chunks, 0.1),
             lambda: api.purge_diverged(prob["node_off"], prob["nodes"], prob["n_post"], chunks, prob["seqs"]))
    for call in calls:
        with pytest.raises(ffi.JtkError) as e:      # an error, never a host computation
            call()
        assert e.value.status == -2
    assert np.array_equal(chunks, prob["chunks"])


# ---- the dataset.py stage, the device call stubbed by the reference

def stub_purge(monkeypatch, calls):
    def fake(node_off, nodes, n_post, chunks, seqs, thr=0.1, device=0):
        ds = R.unflatten(node_off, nodes, n_post, chunks, seqs)
        res = R.purge(ds, thr)
        assert res["status"] == 0
        chunks["cluster_num"] = res["cluster_num"]
        calls.append("purge")
        return {k: np.array(res[k]) for k in ("keep", "cluster", "touched", "post_keep", "purged")}
    monkeypatch.setattr(api, "purge_diverged", fake)


def same_reads(got, want):
    assert [r["id"] for r in got] == [r["id"] for r in want]
    for a, b in zip(got, want):
        for key in ("original_length", "leading_gap", "trailing_gap", "edges"):
            assert a[key] == b[key], (a["id"], key)
        assert len(a["nodes"]) == len(b["nodes"])
        for na, nb in zip(a["nodes"], b["nodes"]):
            for key in ("position_from_start", "chunk", "cluster", "seq", "is_forward", "cigar", "posterior"):
                assert na[key] == nb[key], (a["id"], key)


def test_dataset_stage(monkeypatch, tmp_path, capsys):
    name = "purge_loses_first_middle_last"
    ds = K.CASES[name]["ds"]
    want = R.written_back(ds, reference(name)["purge"])
    calls = []
    stub_purge(monkeypatch, calls)
    monkeypatch.setattr(api, "trim_cache", lambda device=0: None)
    src, dst = tmp_path / "in.json", tmp_path / "out.json"
    before = dataset_json(ds)
    src.write_text(json.dumps(before))
    assert D.main(["--stage", "purge_diverged_nodes", str(src), str(dst)]) == 0
    assert "PD\tPurged\t31\n" in capsys.readouterr().err
    after = json.loads(dst.read_text())
    D.sanity_check(after)
    same_reads(after["encoded_reads"], want["reads"])
    assert [c["cluster_num"] for c in after["selected_chunks"]] == [c["cluster_num"] for c in want["chunks"]] == [2, 2, 1, 1]
    for key in before:
        if key not in ("selected_chunks", "encoded_reads"):
            assert after[key] == before[key]
    # --recluster: local_clustering_selected on the purged chunks, on the purged data set, copy numbers as they stand
    seen = []

    def fake_lc(ds_, selection, **kw):
        seen.append((copy.deepcopy(ds_), list(selection)))
        calls.append("recluster")
    monkeypatch.setattr(D, "local_clustering_selected", fake_lc)
    assert D.main(["--stage", "purge_diverged_nodes", "--recluster", str(src), str(dst)]) == 0
    assert calls == ["purge", "purge", "recluster"] and seen[0] == (after, [31])
    # nothing purged: nothing to recluster
    src.write_text(json.dumps(dataset_json(K.CASES["purge_no_flag"]["ds"])))
    assert D.main(["--stage", "purge_diverged_nodes", "--recluster", str(src), str(dst)]) == 0 and calls[3:] == ["purge"]
    assert "PD\tPurged\t\n" in capsys.readouterr().err
