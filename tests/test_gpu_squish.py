"""jtk_lc_squish_clusters (squish.hip) against tests/squish_reference.py under ProjectMath on every problem of
tests/squish_cases.py: status, the pair list (ids and observation counts equal, the index BIT-equal), classes, cluster_num, the
nodes' clusters and rewritten flags.  No tolerance: every float of the path is one division of integers or a sum in a fixed order.
Then `--stage corrected` against reference-squish followed by the correction entry, and the same call twice (the path has
atomics)."""
import copy
import json

import numpy as np
import pytest

import correction_reference as CRF
import squish_cases as K
import squish_reference as R
import test_squish_reference as T
from helpers import bits, correction_dataset
from jtk_amd import api, dataset as D, ffi

pytestmark = pytest.mark.gpu


def device_run(ds, cfg):
    prob = CRF.flatten(ds)
    chunks = prob["chunks"].copy()
    try:
        out = api.squish_clusters(prob["node_off"], prob["nodes"], prob["posteriors"], chunks, config=cfg)
        out["status"] = 0
    except ffi.JtkError as e:
        out = dict(status=e.status)
    out["chunks"] = chunks
    return out, prob


def assert_same(dev, ref, prob):
    assert dev["status"] == ref["status"]
    if ref["status"] != 0:
        assert np.array_equal(dev["chunks"], prob["chunks"])   # nothing written
        return
    assert list(zip(dev["pair_u1"].tolist(), dev["pair_u2"].tolist())) == [p[:2] for p in ref["pairs"]]
    assert dev["pair_count"].tolist() == [p[3] for p in ref["pairs"]]
    assert np.array_equal(bits(dev["pair_ari"]), bits(np.array([p[2] for p in ref["pairs"]], dtype=np.float64)))
    assert dev["classes"].tolist() == ref["classes"]
    assert dev["chunks"]["cluster_num"].tolist() == ref["cluster_num"]
    assert dev["cluster"].tolist() == ref["cluster"] and dev["touched"].tolist() == ref["touched"]


@pytest.mark.parametrize("name", K.NAMES)
def test_every_case_against_the_reference(name):
    dev, prob = device_run(K.CASES[name]["ds"], T.config_of(name))
    assert_same(dev, T.reference(name), prob)


def test_pair_list_is_optional_and_its_capacity_checked():
    import ctypes as C
    name = "suspicious_smaller_isolated_larger"
    prob, ref = CRF.flatten(K.CASES[name]["ds"]), T.reference(name)
    n, m = len(prob["nodes"]), len(prob["chunks"])
    L, cfg = ffi.lib(), T.config_of(name)

    def call(with_pairs, cap):
        chunks = prob["chunks"].copy()
        classes, cluster, touched = np.full(m, 9, np.uint8), np.zeros(n, np.uint64), np.full(n, 9, np.uint8)
        u1, u2, ari, cnt = np.zeros(16, np.uint64), np.zeros(16, np.uint64), np.zeros(16), np.zeros(16, np.uint64)
        n_pairs = C.c_size_t(99)
        rc = L.jtk_lc_squish_clusters(len(prob["node_off"]) - 1, ffi.u64p(prob["node_off"]), prob["nodes"].ctypes.data,
                                      ffi.f64p(prob["posteriors"]), m, chunks.ctypes.data, C.byref(cfg), ffi.u8p(classes),
                                      ffi.u64p(cluster), ffi.u8p(touched), ffi.u64p(u1) if with_pairs else None, ffi.u64p(u2),
                                      ffi.f64p(ari), ffi.u64p(cnt), cap, C.byref(n_pairs), 0)
        return rc, n_pairs.value, classes, chunks
    rc, got, classes, chunks = call(False, 0)            # one NULL skips all four
    assert rc == 0 and got == len(ref["pairs"]) and classes.tolist() == ref["classes"]
    rc, got, classes, chunks = call(True, len(ref["pairs"]) - 1)
    assert rc == -1 and got == len(ref["pairs"]) and classes.tolist() == [9] * m and np.array_equal(chunks, prob["chunks"])


def test_same_call_twice_gives_identical_output():
    for name in ("beyond_every_grid", "graph_fractional_scores"):
        a, _ = device_run(K.CASES[name]["ds"], T.config_of(name))
        b, _ = device_run(K.CASES[name]["ds"], T.config_of(name))
        assert a["status"] == b["status"] == 0
        for key in ("pair_u1", "pair_u2", "pair_count", "classes", "cluster", "touched", "chunks"):
            assert np.array_equal(a[key], b[key]), key
        assert np.array_equal(bits(a["pair_ari"]), bits(b["pair_ari"]))


def test_stage_corrected_is_squish_then_correction(monkeypatch, tmp_path):
    """`--stage corrected` on a two-haplotype data set whose chunk 1 (the smallest id) is labelled at random: squish collapses
    it, the correction then runs on what is left -- equal to the reference's squish followed by jtk_lc_correct_clustering"""
    ds = correction_dataset(110, [1, 2, 3, 4, 5, 6], 44, hard=True, coverage=20.0)
    rng = np.random.default_rng(2)
    for read in ds["reads"]:
        for n in read["nodes"]:
            if n["chunk"] == 1:
                n["cluster"] = int(rng.integers(0, 2))
                n["posterior"] = [0.0, -10000.0] if n["cluster"] == 0 else [-10000.0, 0.0]
    squished = R.squish(ds, exp=T.CR.ProjectMath().exp)
    assert squished["status"] == 0 and squished["classes"][0] == R.SUSPICIOUS and sum(squished["touched"]) > 0
    mid = R.written_back(ds, squished)
    min_gain = 1.0
    monkeypatch.setattr(api, "estimate_minimum_gain", lambda *a, **k: min_gain)   # (a device simulation of its own: not this test's)
    src, dst = tmp_path / "in.json", tmp_path / "out.json"
    src.write_text(json.dumps(T.dataset_json(ds)))
    assert D.main(["--stage", "corrected", str(src), str(dst)]) == 0
    after = json.loads(dst.read_text())
    prob = CRF.flatten(mid)
    chunks = prob["chunks"].copy()
    sel = sorted(int(c["id"]) for c in chunks if c["cluster_num"] > 1)
    cluster, touched = api.correct_clustering(prob["read_id"], prob["node_off"], prob["nodes"], prob["posteriors"], chunks, sel,
                                              ds["coverage"], min_gain)
    assert [c["cluster_num"] for c in after["selected_chunks"]] == chunks["cluster_num"].tolist()
    k_of = {int(c["id"]): int(c["cluster_num"]) for c in chunks}
    e = 0
    for ra, rm in zip(after["encoded_reads"], mid["reads"]):
        for na, nm in zip(ra["nodes"], rm["nodes"]):
            if touched[e]:
                want = [-10000.0] * k_of[nm["chunk"]]
                want[int(cluster[e])] = 0.0
                assert (na["cluster"], na["posterior"]) == (int(cluster[e]), want)
            else:
                assert (na["cluster"], na["posterior"]) == (nm["cluster"], nm["posterior"])
            e += 1
    assert touched.sum() > 0
