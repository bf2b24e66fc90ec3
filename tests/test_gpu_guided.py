"""jtk_lc_align_guided on the device against tests/guided_reference.py: score, start, end, status and every op of every
pair of tests/guided_cases.py, no tolerance.  The CPU side (the reference against its own properties, the conditions on the
cases at the limits and the census of the events on the optimal paths) is tests/test_guided_reference.py.

Duration of `pytest tests -m gpu` on one MI355X: GPU_SUITE_SECONDS below; TEST_SECONDS is the call time of each test that is new
or grew, in a run of this module on its own (the reference's share included).

Seeded faults, each in an uncommitted copy of the kernels, one build and one run of tests/test_gpu_guided.py, test_guided_abi.py
and test_gpu_encode_nodes.py each: KERNEL_SEEDED_FAULTS below.  "the parent's tests" are these modules as they were before the
cases at the limits were added, run once against the same libraries."""
import numpy as np
import pytest

import guided_cases as K
from jtk_amd import api, ffi

pytestmark = pytest.mark.gpu

UNSUPPORTED, CHUNK_FAILED = -3, -6

# `this`: the one full run with these tests in place, in two processes (643.6 s + 265.9 s).  The parent's whole suite was not run
# again: its versions of the three touched modules took 11.9 s in one process (32 tests), these take 18.9 s in three processes
# (60 tests), so the growth is about 7 s and the parent's total about 902 s.
GPU_SUITE_SECONDS = dict(parent=(902.5, "derived: this less the 7 s by which the three touched modules grew"), this=(909.5, "474 passed, 1 skipped"))
TEST_SECONDS = {
    "test_named_cases": 0.91,      # 0.70 before the cases at the limits
    "test_one_pair_one_cell_over_the_width_cap[False]": 0.01, "test_one_pair_one_cell_over_the_width_cap[True]": 0.01,
    "test_more_global_row_pairs_than_waves_in_one_slice_and_in_three": 0.64,
    "test_32000_by_32000[scores0-2]": 0.35, "test_32000_by_32000[scores1-2]": 0.31, "test_32000_by_32000[scores2-1]": 0.21,
    "test_32000_by_32000[scores3-2]": 0.33, "test_pairs_over_the_length_limit": 0.02,
}
KERNEL_SEEDED_FAULTS = {
    "guided.hip, gd_pair: lane 0 of a 64-column piece takes GD_NEG for the M state of its left neighbour, not the carried left_m":
        "test_named_cases[ins_opens_behind_column_127: score and ops], test_more_global_row_pairs_than_waves_in_one_slice_and_in_three, "
        "test_gpu_encode_nodes.py::test_a_band_wider_than_256_alone_and_in_a_batch; the 21 other tests pass.  The parent's tests: "
        "all 12 pass -- no case of theirs has an I cell in the first column of a later piece whose gap opens from M on the optimal "
        "path, which the census now asks for",
    "guided.hip, gd_pair: the running maximum of the I scan is not carried on, `run = __shfl(incl, 63, 64)`":
        "test_named_cases (the walk leaves the band, JTK_ERR_INTERNAL), test_one_pair_one_cell_over_the_width_cap[False, True], "
        "test_more_global_row_pairs_than_waves_in_one_slice_and_in_three; the 20 other tests pass.  The parent's tests: "
        "test_named_cases fails too",
    "guided.hip, gd_pair: where the rows are in global memory, prev is read from the half that cur is written to":
        "test_named_cases (the walk leaves the band, JTK_ERR_INTERNAL), test_one_pair_one_cell_over_the_width_cap[False, True], "
        "test_more_global_row_pairs_than_waves_in_one_slice_and_in_three, "
        "test_gpu_encode_nodes.py::test_a_band_wider_than_256_alone_and_in_a_batch; the 19 other tests pass.  The parent's tests: "
        "test_named_cases fails too, by width513 and width571 -- a swapped row breaks every pair of the global-rows launch, so this "
        "fault was never the suite's gap; the gap was the wave that takes a second pair, the widths above 571 and the cap",
    "wave_util.h, jtk_band_rows: a Match that does not fit steps j where j < m, instead of being skipped":
        "no test fails, and none can: a Match does not fit where i == n or j == m.  With j == m the changed walk does nothing; "
        "with i == n every later op can only step j, the tail takes the path to (n, m) along row n either way, and row n spans "
        "lo[n] to m in both.  The band is the same band, so this fault changes no value (60 tests of the five guided and polish "
        "modules pass).  The cases guide_of_*_ends_in_skipped_* and skipped_match_then_dels hold the skipped ops at the ends of the "
        "64-op loads all the same",
}


@pytest.fixture(scope="module")
def lib(jtk_lib):
    assert jtk_lib.jtk_lc_device_ok(0) == 1, "needs a gfx950 device"
    return jtk_lib


def run(cases, **kw):
    """cases of one mode and one set of scores, in one call"""
    assert len({(c["infix"], c["scores"]) for c in cases}) == 1
    items = [(c["x"], c["y"], np.array(c["guide"], dtype=np.uint8), c["radius"]) for c in cases]
    return api.align_guided_seqs(items, mode="infix" if cases[0]["infix"] else "global", scores=cases[0]["scores"], **kw)


def ops_of(out, p):
    return out["ops"][int(out["ops_off"][p]):int(out["ops_off"][p + 1])].tolist()


def check(cases, out, names=None, skip=()):
    for p, cs in enumerate(cases):
        if p in skip:
            continue
        want = K.expected(cs)
        got = (int(out["score"][p]), int(out["start"][p]), int(out["end"][p]), int(out["status"][p]))
        print(names[p] if names else p, "n", len(cs["x"]), "m", len(cs["y"]), "radius", cs["radius"], "reference", want["score"], want["start"],
              want["end"], "device", got)
        assert got == (want["score"], want["start"], want["end"], 0), names[p] if names else p
        assert ops_of(out, p) == want["ops"], names[p] if names else p


def test_named_cases(lib):
    """every named case; the cases of one mode and one set of scores share a call"""
    groups = {}
    for name, cs in K.CASES.items():
        groups.setdefault((cs["infix"], cs["scores"]), []).append(name)
    assert len(groups) >= 4
    for names in groups.values():
        cases = [K.CASES[n] for n in names]
        out = run(cases)
        assert out["rc"] == 0
        check(cases, out, names)


@pytest.mark.parametrize("infix", (False, True))
def test_batch_of_70_in_one_slice_and_in_three(lib, infix):
    """70 mixed pairs in one call, and again with the work-area budget cut so that the batch runs in three slices: the same
    answers, and the reference's"""
    cases = [dict(c, infix=infix) for c in K.mixed_batch()]
    whole = run(cases)
    assert whole["rc"] == 0 and api.guided_timing()["slices"] == 1
    check(cases, whole)
    cells = api.guided_timing()["cells"]
    try:
        # the budget is compared with the bound of the cells (at least the cells) plus the row tables
        api.guided_scratch_cap(max(cells // 2, 1))
        sliced = run(cases)
        slices = api.guided_timing()["slices"]
    finally:
        api.guided_scratch_cap(0)
    print("cells", cells, "slices", slices)
    assert slices >= 3
    for key in ("score", "start", "end", "status", "ops", "ops_off"):
        assert bytes(sliced[key]) == bytes(whole[key]), key


def test_one_pair_over_the_width_cap(lib):
    """a 5,000-op Ins run makes one row wider than JTK_GUIDED_MAX_WIDTH: that pair is refused, the others are answered"""
    cases = K.mixed_batch(count=9)
    cases.insert(4, K.over_wide_pair())
    with pytest.raises(ffi.JtkError):
        run(cases)
    out = run(cases, raise_on_pair_failure=False)
    assert out["rc"] == CHUNK_FAILED and out["status"].tolist() == [0] * 4 + [UNSUPPORTED] + [0] * 5
    assert ops_of(out, 4) == [] and int(out["score"][4]) == 0
    check(cases, out, skip=(4,))


@pytest.mark.parametrize("infix", (False, True))
def test_one_pair_one_cell_over_the_width_cap(lib, infix):
    """four rows of 4,097 cells are refused beside four rows of 4,096, which are answered (rows_of_4096 also runs with the named
    cases): the cap from both sides, in both modes"""
    tag = "infix" if infix else "global"
    cases = [K.CASES["rows_of_4096_" + tag], K.CASES["one_match_" + tag], K.over_cap_pair(infix), K.CASES["rows_of_2049_" + tag],
             K.CASES["rows_of_4096_" + tag]]
    out = run(cases, raise_on_pair_failure=False)
    assert out["rc"] == CHUNK_FAILED and out["status"].tolist() == [0, 0, UNSUPPORTED, 0, 0]
    assert ops_of(out, 2) == [] and (int(out["score"][2]), int(out["start"][2]), int(out["end"][2])) == (0, 0, 0)
    check(cases, out, skip=(2,))


def test_more_global_row_pairs_than_waves_in_one_slice_and_in_three(lib):
    """520 pairs with rows of 513 ..= 700 cells and 129 LDS-sized ones in one call: the global-rows launch has 512 waves, so
    waves take a second pair on the rows their first one left, and both launches have work in the slice.  Then the same call in
    three slices or more: the same bytes"""
    cases = K.large_batch()
    whole = run(cases)
    assert whole["rc"] == 0 and api.guided_timing()["slices"] == 1
    check(cases, whole)
    cells = api.guided_timing()["cells"]
    try:
        api.guided_scratch_cap(max(cells // 2, 1))
        sliced = run(cases)
        slices = api.guided_timing()["slices"]
    finally:
        api.guided_scratch_cap(0)
    print("cells", cells, "slices", slices)
    assert slices >= 3
    for key in ("score", "start", "end", "status", "ops", "ops_off"):
        assert bytes(sliced[key]) == bytes(whole[key]), key


@pytest.mark.parametrize("scores,radius", K.LIMIT_RUNS)
def test_32000_by_32000(lib, scores, radius):
    """the longest pair the call takes, mostly mismatching, at the default scores and at +- JTK_GUIDED_MAX_SCORE, where the
    score is below -3e7 (tests/test_guided_reference.py): finite scores that far down are still told from minus infinity"""
    cs = K.limit_pair(scores, radius)
    out = run([cs])
    assert out["rc"] == 0
    check([cs], out)


def test_pairs_over_the_length_limit(lib):
    """32,001 x bases in pair 1 and 32,001 y bases in pair 3 are refused on the host; pairs 0, 2 and 4 are answered"""
    cases = K.over_length_batch()
    with pytest.raises(ffi.JtkError):
        run(cases)
    out = run(cases, raise_on_pair_failure=False)
    assert out["rc"] == CHUNK_FAILED and out["status"].tolist() == [0, UNSUPPORTED, 0, UNSUPPORTED, 0]
    for p in (1, 3):
        assert ops_of(out, p) == [] and (int(out["score"][p]), int(out["start"][p]), int(out["end"][p])) == (0, 0, 0)
    check(cases, out, skip=(1, 3))


@pytest.mark.parametrize("radius,infix", ((10, False), (200, False), (10, True)))
def test_2000_by_2100_at_ten_percent(lib, radius, infix):
    """radius 10: rows of 21 cells in LDS; radius 200: 401 cells and more"""
    cs = K.big_pair(radius, infix)
    out = run([cs])
    assert out["rc"] == 0
    check([cs], out)
