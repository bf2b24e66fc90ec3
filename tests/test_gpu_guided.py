"""jtk_lc_align_guided on the device against tests/guided_reference.py: score, start, end, status and every op of every
pair of tests/guided_cases.py, no tolerance.  The CPU side (the reference against its own properties) is
tests/test_guided_reference.py."""
import numpy as np
import pytest

import guided_cases as K
from jtk_amd import api, ffi

pytestmark = pytest.mark.gpu

UNSUPPORTED, CHUNK_FAILED = -3, -6


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


@pytest.mark.parametrize("radius,infix", ((10, False), (200, False), (10, True)))
def test_2000_by_2100_at_ten_percent(lib, radius, infix):
    """radius 10: rows of 21 cells in LDS; radius 200: 401 cells and more"""
    cs = K.big_pair(radius, infix)
    out = run([cs])
    assert out["rc"] == 0
    check([cs], out)
