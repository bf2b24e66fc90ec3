"""jtk_lc_sketch and jtk_lc_map_reads on the device against tests/map_reference.py on every case of tests/map_cases.py: the
minimizers and the placements are EQUAL, record for record -- everything is an integer, so there is no tolerance.  The hit buffer
is sized from the scan of the counts, so there is no first, smaller buffer of hits to outgrow; what can be too small is the
caller's `cap`, and that is asked here one below the need, at the need, and through api.map_reads' own second call."""
import ctypes as C

import numpy as np
import pytest

import map_cases as K
import map_reference as R
from jtk_amd import api, ffi

pytestmark = pytest.mark.gpu
FIELDS = ffi.MAP_PLACEMENT_DT.names


def records(placements):
    return [{f: int(p[f]) for f in FIELDS} for p in placements]


@pytest.mark.parametrize("case", K.SKETCH_CASES, ids=[c["name"] for c in K.SKETCH_CASES])
def test_sketch_equals_the_reference(case, jtk_lib):
    got = api.sketch(case["seqs"], case["k"], case["w"], cap=8)     # too small wherever there is more to return: the second call
    want = [(s, p, h, st) for s, seq in enumerate(case["seqs"]) for p, h, st in R.sketch(seq, case["k"], case["w"])]
    assert got["hash"].dtype == np.uint64 and len(got["hash"]) == len(want)
    assert list(zip(got["seq"].tolist(), got["pos"].tolist(), got["hash"].tolist(), got["strand"].tolist())) == want


@pytest.fixture(scope="module")
def reference():
    return {c["name"]: R.map_reads(c["targets"], c["queries"], **c["params"]) for c in K.MAP_CASES}


@pytest.mark.parametrize("case", K.MAP_CASES, ids=[c["name"] for c in K.MAP_CASES])
def test_map_reads_equals_the_reference(case, reference, jtk_lib):
    want = reference[case["name"]]
    got = records(api.map_reads(case["targets"], case["queries"], cap=2, **case["params"]))
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, i


def test_what_the_cases_hold(reference):
    """the shapes the cases are there for, read off the reference"""
    assert len(reference["tandem"]) == 4 and [p["is_forward"] for p in reference["tandem"]] == [1, 1, 0, 0]
    assert len(reference["diagonals_100_apart"]) == 2 and len(reference["diagonals_101_apart"]) == 4
    one, two = reference["diagonals_100_apart"][0], reference["diagonals_101_apart"][0]
    assert one["diag_hi"] - one["diag_lo"] == 100 and one["n_seeds"] == two["n_seeds"]     # the copies share their target positions
    assert [p["n_seeds"] for p in reference["homopolymer_kept"]] == [286, 286, 286] and reference["homopolymer_dropped"] == []
    assert reference["one_seed_short"] == [] and len(reference["just_enough_seeds"]) == 1
    assert reference["no_hit_at_all"] == [] and {p["query"] for p in reference["no_hit_queries"]} == {1, 3}
    assert all(p["query"] != p["target"] for p in reference["skip_self"]) and reference["skip_self"]
    assert len(reference["not_skip_self"]) > len(reference["skip_self"])


def test_a_capacity_that_is_too_small_returns_the_need(jtk_lib, reference):
    case = next(c for c in K.MAP_CASES if c["name"] == "planted_5")
    want = reference[case["name"]]
    _, tb, toff = api._flat_seqs(case["targets"])
    _, qb, qoff = api._flat_seqs(case["queries"])
    p = case["params"]
    params = np.array([(p["k"], p["w"], p["max_occ"], p["max_gap"], p["min_seeds"], 0)], dtype=ffi.MAP_PARAMS_DT)
    n = C.c_uint64(0)
    for cap, rc in ((len(want) - 1, -1), (len(want), 0)):
        out = np.zeros(len(want) + 1, dtype=ffi.MAP_PLACEMENT_DT)
        out.view(np.uint8)[:] = 7
        before = out.copy()
        got = jtk_lib.jtk_lc_map_reads(len(toff) - 1, ffi.u8p(tb), ffi.u64p(toff), len(qoff) - 1, ffi.u8p(qb), ffi.u64p(qoff), params.ctypes.data,
                                       out.ctypes.data, cap, C.byref(n), 0)
        assert got == rc and n.value == len(want)
        if rc:
            assert (out == before).all()                                   # nothing else is written
        else:
            assert records(out[:len(want)]) == want and out[len(want)] == before[len(want)]
    timing = api.map_timing()
    assert timing["n_hits"] > 0 and timing["n_minimizers"] > 0
    assert all(timing[f] > 0 for f in ("sketch_ms", "index_ms", "hits_ms", "order_ms", "chain_ms", "compact_ms"))


@pytest.mark.parametrize("rate", sorted(K.PLANTED_SEEDS))
def test_the_planted_set_on_the_device(rate, jtk_lib):
    p = K.planted_at(rate)
    reads = p["reads"] + [p["unrelated"]]
    got = api.map_reads(p["chunks"], reads)
    by_pair = {}
    for i, g in enumerate(got):
        by_pair.setdefault((int(g["query"]), int(g["target"])), []).append(i)
    trials = {t[0]: t for t in api.map_trials(got, [len(r) for r in reads], [len(c) for c in p["chunks"]], 0.3)}
    for r, spans in enumerate(p["truth"]):
        for c, (lo, hi, forward) in spans.items():
            hits = [i for i in by_pair.get((r, c), []) if int(got[i]["is_forward"]) == forward and i in trials]
            assert hits, (r, c)
            assert any(trials[i][1] <= lo and hi <= trials[i][2] for i in hits), (r, c)
    assert not any(int(g["query"]) == len(reads) - 1 for g in got)
