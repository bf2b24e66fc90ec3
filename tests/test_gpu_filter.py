"""The variant filter and the pick on the device, through jtk_lc_debug_filter (include/jtk_lc_debug.h), against the record of
tests/clustering_reference.py in tests/golden/filter_reference.json (tests/test_filter_reference.py keeps that record live and
shows that every case reaches its branch).  The input is tests/filter_cases.py's; the golden is keyed by its SHA-256.

Every table case runs in mode 0 (homop_kernel, chunk_tables_kernel, column_filter_kernel, pick_kernel<true>,
pick_trace_kernel<true>), every row-sum case in mode 1 (column_filter_fused_kernel, pick_kernel<false>, pick_trace_kernel<false>)
and in mode 2 (finalize_kernel, then the table kernels).  The comparison is exact: the whole cand array (-1 where the reference has
no candidate, the score's bits where it has one), dim, the picked columns, their variant types, the feature bits and the pick order;
modes 1 and 2 agree byte for byte.  No case needed a tolerance: the sums run left to right over the reads in the reference and in
both kernels and the logarithm is the project's own.

Duration of `pytest tests -m gpu` on one MI355X: GPU_SUITE_SECONDS; TEST_SECONDS is the call time of the tests of this module.
Seeded faults, each in an uncommitted copy of filter_kernels.hip / finalize_common.h, one run each: KERNEL_SEEDED_FAULTS.
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import filter_cases as F
from jtk_amd import api, ffi

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "filter_reference.json")
GPU_SUITE_SECONDS = dict(parent=(945.0, "derived: this less the 2.0 s of this module's calls; no run of the parent was made"), this=(947.0, "542 passed, 1 skipped"))
TEST_SECONDS = dict(rows_deep=1.4, planted_60=0.24, every_other=0.1)   # call times; rows_deep uploads 0.7 GB twice
# each: the library built from an uncommitted copy with the one change, then this module and the five
# test_pileup_against_the_reference cases of tests/test_gpu_clustering_reference.py in one run; "the rest" = the other tests of the two
KERNEL_SEEDED_FAULTS = {
    "finalize_common.h: FIN_ROWS = FIN_TILE + 3 (a tile stages one row less)":
        "NOT caught, and not catchable through the filter: the row that is missing is p0 + 131, which only the 3-bp deletion (row 13) of "
        "the tile's last position reads, and filter_profiles reads rows 0-7 and 11 (pseudo_mcmc.rs:447-449).  21 passed",
    "finalize_common.h: FIN_ROWS = FIN_TILE + 1 (three rows less: row p0 + 129 is missing, the 1-bp deletion of position 127 reads it)":
        "test_row_sum_case_fused_and_materialised[rows_tile_edges]; the rest passes",
    "column_filter_fused_kernel takes hmm2[1] for a forward read and hmm2[0] for a reverse one":
        "test_row_sum_case_fused_and_materialised[rows_tile_edges], [rows_deep]; the rest passes",
    "pick_body: `ov == bv && oi > bi` turned to `oi < bi` (the first of equal maxima across lanes)":
        "test_table_case[planted_60], [short_templates], [thresholds], [thresholds_pos_thr], [homopolymers_h1], [homopolymers_h3], "
        "[homopolymers_h8], [copy_numbers], [pick_many]; the rest passes",
    "pick_body: `diff < JTK_MASK_LENGTH` turned to `<=`":
        "test_table_case[tile_edges], [pick_many], [pick_cap], test_row_sum_case_fused_and_materialised[rows_tile_edges], "
        "test_table_of_the_row_sums_through_the_table_filter; the rest passes",
    "pick_body: `0.8 < sok` turned to `0.8 <= sok`":
        "test_table_case[pick_many]; the rest passes",
    "column_filter_fused_kernel: `pos[j] += strand ? 1u << 16 : 1u` turned to `1u << 15`":
        "test_row_sum_case_fused_and_materialised[rows_deep] -- and test_pileup_against_the_reference[ont_diploid], [ont_4copy], "
        "[ont_diploid_80_reads]: this one the pile-ups caught before (a forward read with a gain is enough); the rest passes",
}


def _hex(x):
    return ["%016x" % int(b) for b in np.ascontiguousarray(x, dtype=np.float64).ravel().view(np.uint64)]


def run_case(name, mode):
    cs = F.CASES[name]()
    gold = json.load(open(GOLDEN))[name]
    assert gold["input_sha256"] == F.input_sha256(cs), "the golden file was written for other input: tests/golden/make_filter_reference.py"
    return cs, gold, api.filter_stage(F.params_of(cs), cs["chunks"], mode)


def compare(name, cs, gold, out):
    assert len(out) == len(cs["chunks"]) == len(gold["chunks"])
    for c, (ch, ref, got) in enumerate(zip(cs["chunks"], gold["chunks"], out)):
        where = (name, c)
        want = np.full(14 * (len(ch["tmpl"]) + 1), -1.0)
        for pos, score, _ in ref["cands"]:
            want[pos] = np.array([int(score, 16)], dtype=np.uint64).view(np.float64)[0]
        assert hashlib.sha256(want.tobytes()).hexdigest() == ref["cand_sha256"], where
        cand = got["cand"]
        assert np.flatnonzero(cand != -1.0).tolist() == [pos for pos, _, _ in ref["cands"]], where
        assert np.array_equal(cand.view(np.uint64), want.view(np.uint64)), where
        assert got["dim"] == len(ref["probes"]) and got["pos"].tolist() == ref["probes"], where
        assert got["vtype"].tolist() == ref["vtype"], where
        assert list(got["feat"].shape) == ref["feat_shape"], where
        assert hashlib.sha256(np.ascontiguousarray(got["feat"]).tobytes()).hexdigest() == ref["feat_sha256"], where
        if ref["feat"] is not None:
            assert _hex(got["feat"]) == ref["feat"], where
        if ch["copy_num"] >= 2:
            assert got["n_cand"] == len(ref["cands"]) and got["order"].tolist() == ref["order"], where
        else:
            assert got["n_cand"] == 0 and got["order"].tolist() == [] == ref["order"], where


@pytest.mark.parametrize("name", list(F.TABLE_CASES))
def test_table_case(jtk_lib, name):
    cs, gold, out = run_case(name, ffi.DEBUG_FILTER_TABLE)
    compare(name, cs, gold, out)


@pytest.mark.parametrize("name", list(F.ROW_CASES))
def test_row_sum_case_fused_and_materialised(jtk_lib, name):
    cs, gold, fused = run_case(name, ffi.DEBUG_FILTER_ROWS_FUSED)
    compare(name + ", fused", cs, gold, fused)
    _, _, tabled = run_case(name, ffi.DEBUG_FILTER_ROWS_TABLE)
    compare(name + ", materialised", cs, gold, tabled)
    for a, b in zip(fused, tabled):
        assert sorted(a) == sorted(b)
        for key in a:
            assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), (name, key)


def test_table_of_the_row_sums_through_the_table_filter(jtk_lib):
    """the row-sum case's own reference table handed over as a table (mode 0): finalize_kernel out of the way, the same record"""
    import clustering_reference as R   # (the logarithm only: the oracle's library, which the GPU suite has built)
    cs = F.rows_tile_edges()
    gold = json.load(open(GOLDEN))["rows_tile_edges"]
    tables = F.tables_of(cs, R.ProjectMath().log)
    chunks = [dict(tmpl=ch["tmpl"], strands=ch["strands"], copy_num=ch["copy_num"], table=t) for ch, t in zip(cs["chunks"], tables)]
    compare("rows_tile_edges as tables", dict(cs, chunks=chunks), gold, api.filter_stage(F.params_of(cs), chunks, ffi.DEBUG_FILTER_TABLE))


def _call(params, chunks, tmpl, strand, mode, values, exps, lk, n_reads, cols):
    """the entry point on one chunk (`chunks` holds a spare record behind it)"""
    L = ffi.lib()
    out = [np.zeros(cols + 1), np.zeros(2, np.uint32), np.zeros(21 + 1, np.uint32), np.zeros(42 + 1, np.uint32),
           np.zeros(21 * n_reads + 1), np.zeros(66 + 1, np.uint32)]
    i32p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))   # noqa: E731
    f64 = lambda a: None if a is None else ffi.f64p(a)   # noqa: E731
    return L.jtk_lc_debug_filter(C.byref(params) if params is not None else None, 1, chunks.ctypes.data,
                                 ffi.u8p(tmpl) if tmpl is not None else None, ffi.u8p(strand) if strand is not None else None, mode, f64(values),
                                 i32p(exps), f64(lk), ffi.f64p(out[0]), ffi.u32p(out[1]), ffi.u32p(out[2]), ffi.u32p(out[3]), ffi.f64p(out[4]),
                                 ffi.u32p(out[5]), 0)


def test_refusals_are_the_hosts(jtk_lib):
    """null pointers, a mode that does not exist, a template with a base that is none of ACGT, a copy number beyond one
    clustering() call's, and the fused filter with 65,536 reads (the session's own rule, session_plan.h: batch_needs_tables):
    JTK_ERR_INVALID_ARG with a message, decided before a device is looked for"""
    p = F.params_of(F.planted_60())
    L, n = 14, 3
    rec = np.zeros(2, dtype=ffi.CHUNK_DT)
    rec[0] = (0, 2, n, 0, L, 0)
    tmpl, strand = np.frombuffer(b"ACGTACGTACGTAC\0", dtype=np.uint8).copy(), np.ones(n + 1, np.uint8)
    table, rows = np.full(n * 14 * (L + 1) + 1, -2.0), np.full(n * 16 * (L + 1) + 1, 1.0)
    exps, lk = np.zeros(n * (L + 1) + 1, np.int32), np.full(n + 1, -10.0)
    cols = 14 * (L + 1)
    err = lambda: ffi.lib().jtk_lc_last_error().decode()   # noqa: E731
    assert _call(p, rec, tmpl, strand, 0, table, None, None, n, cols) == 0          # the call itself is sound
    assert _call(p, rec, tmpl, strand, 1, rows, exps, lk, n, cols) == 0
    assert _call(None, rec, tmpl, strand, 0, table, None, None, n, cols) == -1 and err() == "null argument"
    assert _call(p, rec, tmpl, None, 0, table, None, None, n, cols) == -1 and err() == "null argument"
    assert _call(p, rec, tmpl, strand, 0, None, None, None, n, cols) == -1 and err() == "null argument"
    assert _call(p, rec, tmpl, strand, 1, rows, None, lk, n, cols) == -1 and err() == "null argument"
    assert _call(p, rec, tmpl, strand, 2, rows, exps, None, n, cols) == -1 and err() == "null argument"
    assert _call(p, rec, tmpl, strand, 3, rows, exps, lk, n, cols) == -1 and "mode" in err()
    bad = tmpl.copy()
    bad[5] = ord("N")
    assert _call(p, rec, bad, strand, 0, table, None, None, n, cols) == -1 and err() == "non-ACGT base in a template"
    eight = rec.copy()
    eight[0]["copy_num"] = 8
    assert _call(p, eight, tmpl, strand, 0, table, None, None, n, cols) == -1 and "copy number" in err()
    # 65,536 reads: refused for the fused filter before anything is read (the buffers hold three reads)
    deep = rec.copy()
    deep[0]["n_reads"] = 65536
    big_strand = np.ones(65537, np.uint8)
    assert _call(p, deep, tmpl, big_strand, 1, rows, exps, lk, n, cols) == -1 and "65,535" in err()
