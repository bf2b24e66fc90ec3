"""jtk_lc_node_errors / jtk_lc_error_quantile / jtk_lc_estimate_error_rate / jtk_lc_purge_diverged (purge.hip) against
tests/purge_reference.py on every problem of tests/purge_cases.py: counts, statuses, flags and lists equal, every float BIT-equal,
the pass count of the fit equal.  No tolerance: every float of the path is a division of integers, a sum in a fixed order, a product,
a max or a host square root."""
import ctypes as C
import json

import numpy as np
import pytest

import purge_cases as K
import purge_reference as R
import test_purge_reference as T
from helpers import bits
from jtk_amd import api, dataset as D, ffi

pytestmark = pytest.mark.gpu


def same_floats(got, want):
    return np.array_equal(bits(np.asarray(got, dtype=np.float64)), bits(np.asarray(want, dtype=np.float64)))


@pytest.mark.parametrize("name", K.NAMES)
def test_node_errors(name):
    prob, ref = R.flatten(K.CASES[name]["ds"]), T.reference(name)
    out = api.node_errors(prob["node_off"], prob["nodes"], prob["chunks"], prob["seqs"], raise_on_node_failure=False)
    assert out["rc"] == (-6 if any(ref["status"]) else 0)
    assert out["err_num"].tolist() == ref["num"] and out["err_len"].tolist() == ref["length"] and out["status"].tolist() == ref["status"]


@pytest.mark.parametrize("name", K.NAMES)
def test_error_quantile_on_the_cases(name):
    ref = T.reference(name)
    for q, want in ref["quantile"].items():
        if isinstance(want, float):
            assert same_floats([api.error_quantile(ref["num"], ref["length"], q)], [want]), q
        else:
            with pytest.raises(ffi.JtkError) as e:
                api.error_quantile(ref["num"], ref["length"], q)
            assert e.value.status == want.status


@pytest.mark.parametrize("name", sorted(K.QUANTILE))
def test_error_quantile(name):
    num, length = K.QUANTILE[name]
    for q in (0.0, 0.5, 1.0, 0.25, 0.999):
        assert same_floats([api.error_quantile(num, length, q)], [R.error_quantile(num, length, q)]), q


@pytest.mark.parametrize("name", K.NAMES)
def test_estimate_error_rate(name):
    ds = K.CASES[name]["ds"]
    prob, ref = R.flatten(ds), T.reference(name)
    if ref["fit_status"] != 0:
        with pytest.raises(ffi.JtkError) as e:
            api.estimate_error_rate(prob["node_off"], prob["nodes"], ref["num"], ref["length"], prob["chunks"], ref["fallback"])
        assert e.value.status == ref["fit_status"]
        return
    out = api.estimate_error_rate(prob["node_off"], prob["nodes"], ref["num"], ref["length"], prob["chunks"], ref["fallback"])
    flat, off = R.flat_chunk_err(ds, ref["fit"]["chunk_err"])
    assert out["n_iter"] == ref["fit"]["n_iter"] and out["chunk_err_off"].tolist() == off
    assert same_floats(out["read_err"], ref["fit"]["read_err"]) and same_floats(out["chunk_err"], flat)
    assert same_floats([out["median_of_sqrt_err"]], [ref["fit"]["median"]])


def device_purge(prob):
    chunks = prob["chunks"].copy()
    try:
        out = api.purge_diverged(prob["node_off"], prob["nodes"], prob["n_post"], chunks, prob["seqs"])
        out["status"] = 0
    except ffi.JtkError as e:
        out = dict(status=e.status)
    out["chunks"] = chunks
    return out


def assert_same_purge(dev, ref, prob):
    assert dev["status"] == ref["status"]
    if ref["status"] != 0:
        assert np.array_equal(dev["chunks"], prob["chunks"])      # nothing written
        return
    for key in ("diverged", "chunk_err_off", "keep", "cluster", "touched", "post_keep", "purged"):
        assert dev[key].tolist() == ref[key], key
    assert dev["chunks"]["cluster_num"].tolist() == ref["cluster_num"]
    assert same_floats(dev["read_err"], ref["read_err"]) and same_floats(dev["chunk_err"], ref["chunk_err"])
    assert same_floats([dev["median_of_sqrt_err"]], [ref["median"]])


@pytest.mark.parametrize("name", K.NAMES)
def test_purge_diverged(name):
    prob = R.flatten(K.CASES[name]["ds"])
    assert_same_purge(device_purge(prob), T.reference(name)["purge"], prob)
    if T.reference(name)["purge"]["status"] == 0:
        assert api.purge_timing()["n_iter"] == T.reference(name)["purge"]["n_iter"]


def test_same_call_twice_gives_identical_bytes():
    for name in ("fit_real_valued", "beyond_one_pass"):
        prob = R.flatten(K.CASES[name]["ds"])
        a, b = device_purge(prob), device_purge(prob)
        assert a["status"] == b["status"] == 0
        for key in a:
            if key != "status":
                assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), key


def raw_purge(prob, slot_cap, purged_cap, with_fit=True):
    """the entry point on arrays filled with 9s, so that a write shows"""
    n, m, n_reads = len(prob["nodes"]), len(prob["chunks"]), len(prob["node_off"]) - 1
    sb, so, ob, oo, tb, to = prob["seqs"]
    o = dict(chunks=prob["chunks"].copy(), diverged=np.full(64, 9, np.uint8), off=np.full(m + 1, 9, np.uint64), keep=np.full(n, 9, np.uint8),
             cluster=np.full(n, 9, np.uint64), touched=np.full(n, 9, np.uint8), post_keep=np.full(prob["n_post"], 9, np.uint8),
             purged=np.full(m, 9, np.uint64), read_err=np.full(n_reads, 9.0), chunk_err=np.full(64, 9.0))
    n_purged, median = C.c_size_t(99), C.c_double(9.0)
    o["rc"] = ffi.lib().jtk_lc_purge_diverged(
        n_reads, ffi.u64p(prob["node_off"]), prob["nodes"].ctypes.data, prob["n_post"], m, o["chunks"].ctypes.data, ffi.u8p(sb), ffi.u64p(so),
        ffi.u8p(ob), ffi.u64p(oo), ffi.u8p(tb), ffi.u64p(to), 0.1, ffi.u8p(o["diverged"]), ffi.u64p(o["off"]), slot_cap, ffi.u8p(o["keep"]),
        ffi.u64p(o["cluster"]), ffi.u8p(o["touched"]), ffi.u8p(o["post_keep"]), ffi.u64p(o["purged"]), purged_cap, C.byref(n_purged),
        ffi.f64p(o["read_err"]) if with_fit else None, ffi.f64p(o["chunk_err"]) if with_fit else None, C.byref(median) if with_fit else None, 0)
    o["n_purged"], o["median"] = n_purged.value, median.value
    return o


def untouched(o, prob):
    return (np.array_equal(o["chunks"], prob["chunks"]) and o["n_purged"] == 99 and o["median"] == 9.0
            and all((o[k] == 9).all() for k in ("diverged", "off", "keep", "cluster", "touched", "post_keep", "purged", "read_err", "chunk_err")))


def test_capacities_are_checked_and_the_fit_is_optional():
    name = "purge_middle_of_three"
    prob, ref = R.flatten(K.CASES[name]["ds"]), T.reference(name)["purge"]
    n_slots, n_purged = len(ref["diverged"]), len(ref["purged"])
    assert n_purged == 1
    o = raw_purge(prob, n_slots, n_purged)
    assert o["rc"] == 0 and o["n_purged"] == 1 and o["purged"][0] == 31 and o["diverged"][:n_slots].tolist() == ref["diverged"]
    assert (o["diverged"][n_slots:] == 9).all() and (o["chunk_err"][n_slots:] == 9).all() and (o["purged"][1:] == 9).all()
    o = raw_purge(prob, n_slots, n_purged, with_fit=False)
    assert o["rc"] == 0 and o["keep"].tolist() == ref["keep"] and (o["read_err"] == 9).all() and o["median"] == 9.0
    for caps in ((n_slots - 1, n_purged), (n_slots, n_purged - 1)):
        o = raw_purge(prob, *caps)
        assert o["rc"] == -1 and untouched(o, prob), caps
    # jtk_lc_estimate_error_rate: one double too few
    num, length = T.reference(name)["num"], T.reference(name)["length"]
    read_err, chunk_err, off = np.full(len(prob["node_off"]) - 1, 9.0), np.full(64, 9.0), np.full(len(prob["chunks"]) + 1, 9, np.uint64)
    median, n_iter = C.c_double(9.0), C.c_uint32(99)
    args = (len(read_err), ffi.u64p(prob["node_off"]), prob["nodes"].ctypes.data, ffi.u32p(np.array(num, np.uint32)),
            ffi.u32p(np.array(length, np.uint32)), len(prob["chunks"]), prob["chunks"].ctypes.data, 0.02, ffi.f64p(read_err), ffi.f64p(chunk_err),
            ffi.u64p(off))
    assert ffi.lib().jtk_lc_estimate_error_rate(*args, n_slots - 1, C.byref(median), C.byref(n_iter), 0) == -1
    assert (read_err == 9).all() and (chunk_err == 9).all() and (off == 9).all() and median.value == 9.0 and n_iter.value == 99
    assert ffi.lib().jtk_lc_estimate_error_rate(*args, n_slots, C.byref(median), C.byref(n_iter), 0) == 0 and (chunk_err[n_slots:] == 9).all()


def test_stage_end_to_end(tmp_path, capsys):
    """`--stage purge_diverged_nodes` on the read that loses its first, a middle and its last node, against the reference's
    written-back data set"""
    name = "purge_loses_first_middle_last"
    ds = K.CASES[name]["ds"]
    want = R.written_back(ds, T.reference(name)["purge"])
    src, dst = tmp_path / "in.json", tmp_path / "out.json"
    src.write_text(json.dumps(T.dataset_json(ds)))
    assert D.main(["--stage", "purge_diverged_nodes", str(src), str(dst)]) == 0
    assert "PD\tPurged\t31\n" in capsys.readouterr().err
    after = json.loads(dst.read_text())
    D.sanity_check(after)
    T.same_reads(after["encoded_reads"], want["reads"])
    assert [c["cluster_num"] for c in after["selected_chunks"]] == [c["cluster_num"] for c in want["chunks"]]
