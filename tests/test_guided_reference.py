"""The guided aligner's specification as tests/guided_reference.py states it, checked against itself on
the CPU: the three hand values of the specification, the three properties a correct banded three-state aligner has, on
seeded random pairs, and tests/encode_reference.py on hand-worked trials, one per verdict.  The device side is
tests/test_gpu_guided.py and tests/test_gpu_encode_nodes.py."""
import numpy as np
import pytest

import encode_cases as EC
import encode_reference as E
import guided_cases as K
import guided_reference as G
from jtk_amd import api

M, X, I, D = G.MATCH, G.MISMATCH, G.INS, G.DEL


def test_hand_values():
    out = G.align_guided(b"ACGTACGT", b"ACGACGT", [M] * 7, 1)
    assert (out["score"], out["start"], out["end"], out["ops"]) == (9, 0, 8, [M, M, M, D, M, M, M, M])
    out = G.align_guided(b"ACGTACGT", b"ACGACGT", [M] * 7, 0)
    assert (out["score"], out["ops"]) == (-23, [M, M, M, X, X, X, X, D])
    out = G.align_guided(b"TTTTACGTACGTGGGG", b"ACGTACGT", [D] * 4 + [M] * 8 + [D] * 4, 2, infix=True)
    assert (out["score"], out["start"], out["end"]) == (16, 4, 12) and out["ops"] == [D] * 4 + [M] * 8 + [D] * 4
    out = G.align_guided(b"AACCAACC", b"AACC", [M] * 4, 8, infix=True)
    assert (out["score"], out["start"], out["end"]) == (8, 0, 4)      # the smallest end wins


def test_degenerate_inputs():
    assert G.align_guided(b"", b"", [], 3) == dict(score=0, start=0, end=0, ops=[])
    assert G.align_guided(b"", b"ACG", [], 0) == dict(score=-7, start=0, end=0, ops=[I] * 3)
    assert G.align_guided(b"ACG", b"", [], 0) == dict(score=-7, start=0, end=3, ops=[D] * 3)
    assert G.align_guided(b"ACG", b"", [], 0, infix=True) == dict(score=0, start=0, end=0, ops=[D] * 3)
    with pytest.raises(ValueError):
        G.align_guided(b"A", b"A", [M], 1, scores=(2, -6, -1, -5))
    with pytest.raises(ValueError):
        G.align_guided(b"A", b"A", [4], 1)


def test_guide_path_skips_and_extends():
    assert G.guide_path(2, 1, [M, M, M, I, D]) == [(0, 0), (1, 1), (2, 1)]          # the second M, the third and the I do not fit
    assert G.guide_path(3, 2, []) == [(0, 0), (1, 1), (2, 2), (3, 2)]                # diagonally, then by Del
    assert G.guide_path(1, 3, [D]) == [(0, 0), (1, 0), (1, 1), (1, 2), (1, 3)]       # ... then by Ins
    assert G.band_cells(2, 4, [M, I, I, M], 1) == {0: (0, 1), 1: (0, 4), 2: (3, 4)}


def random_pairs(count, seed):
    rng = np.random.default_rng(seed)
    for k in range(count):
        x = K.random_seq(rng, int(rng.integers(0, 60)), alphabet=(4, 2)[k % 2])
        y, guide = K.mutate_with_guide(rng, x, (0.1, 0.3, 0.5)[k % 3], alphabet=(4, 2)[k % 2])
        if k % 4 == 0:
            guide = [int(v) for v in rng.integers(0, 4, int(rng.integers(0, 90)))]
        yield x, y, guide, bool(k % 2)


def test_score_of_ops_monotone_in_radius_and_unbanded_limit():
    """on 120 seeded random pairs, global and infix: the ops spell the score, the score does not fall as the radius grows, and
    at a radius beyond both lengths it is the unbanded optimum"""
    for x, y, guide, infix in random_pairs(120, 7305):
        last = None
        for radius in (0, 1, 3, 8, 70):
            out = G.align_guided(x, y, guide, radius, infix=infix)
            assert G.score_of_ops(x, y, out["ops"], out["start"], out["end"]) == out["score"]
            assert last is None or out["score"] >= last
            last = out["score"]
        assert last == G.unbanded(x, y, infix=infix)


def test_named_cases_spell_their_scores_and_have_the_widths_they_are_named_for():
    for name, cs in K.CASES.items():
        out = K.expected(cs)
        assert G.score_of_ops(cs["x"], cs["y"], out["ops"], out["start"], out["end"], cs["scores"]) == out["score"], name
    for name, width in (("width63", 63), ("width64", 64), ("width65", 65), ("width128", 128), ("width129", 129)):
        assert K.row_widths(K.CASES[name]).count(width) >= 5, name      # (the last row, which runs on to the end of y, is wider)
    for name, width in (("width512", 512), ("width513", 513), ("width513_infix", 513), ("width571", 571)):
        assert max(K.row_widths(K.CASES[name])) == width, name
    assert max(K.row_widths(K.CASES["ins_run70"])) == 71 + 2 * 3
    assert max(K.row_widths(K.over_wide_pair())) > api.ffi.GUIDED_MAX_WIDTH
    # the L-shaped band keeps the answer off the main diagonal: every x base is deleted or matched in column <= radius
    cs = K.CASES["l_shaped"]
    assert K.expected(cs)["score"] < G.align_guided(cs["x"], cs["y"], [], 2)["score"]
    # a mismatch (-6) beats two opened gaps (-10); with a mismatch at -20 an Ins and a Del stand side by side
    assert X in K.expected(K.CASES["mismatch_or_two_opens"])["ops"]
    ops = K.expected(K.CASES["ins_after_del"])["ops"]
    assert X not in ops and any({a, b} == {D, I} for a, b in zip(ops, ops[1:]))
    # only the M, D, I order decides between equal scores
    assert K.expected(K.CASES["all_tie"])["ops"] == [D] * 3 + [M] * 9      # M first at every step back: the gap ends up in front
    assert K.expected(K.CASES["all_tie_infix"])["ops"] == [M] * 9 + [D] * 3 and K.expected(K.CASES["all_tie_infix"])["end"] == 9
    # without leading Dels at radius 2 only rows 0 ..= 2 are free starts: the wider band finds the copy, the narrow one cannot
    narrow, wide = K.expected(K.CASES["infix_no_leading_dels_radius2"]), K.expected(K.CASES["infix_no_leading_dels_radius12"])
    assert narrow["start"] <= 2 and 9 <= wide["start"] <= 11 and wide["score"] > narrow["score"]


def test_encode_reference_hand_worked_trials():
    cons = b"ACGTTGCAAGCT"
    # lower bound: (12 - 4) / 12 > 0.5
    out = E.encode_node(b"GG" + cons + b"TT", 2, 6, True, cons, cons, 0.5)
    assert out["verdict"] == E.LOWER_BOUND and out["ops"] == [] and out["band"] == 10
    # accepted: an exact copy between flanks of two bases.  head: the ops with rpos < min(100, 12) are the first 11; tail: all 12
    out = E.encode_node(b"GG" + cons + b"TT", 0, 16, True, cons, cons, 0.25)
    assert (out["verdict"], out["trim_head"], out["trim_tail"], out["position_from_start"], out["query_len"]) == (E.ACCEPTED, 2, 2, 2, 12)
    assert (out["mat_num"], out["ops_len"], out["head_match"], out["head_len"], out["tail_match"], out["tail_len"]) == (12, 12, 11, 11, 12, 12)
    assert out["score"] == 24 and out["ops"] == [M] * 12 and out["query"] == cons
    # the same on the reverse strand, lower-case, with uneven flanks: position_from_start counts the tail trim
    read = b"cc" + E.window_of(b"G" + cons + b"TTT", 0, 16, False).lower() + b"a"
    out = E.encode_node(read, 2, 18, False, cons, cons, 0.25)
    assert (out["verdict"], out["trim_head"], out["trim_tail"], out["position_from_start"]) == (E.ACCEPTED, 1, 3, 5)
    # rejected: every third base substituted, at most 13 of 20 columns can match: 0.75 < identity fails
    cons = b"ACGTTGCAAGCTGGATCCAT"
    bad = bytearray(cons)
    for q in range(0, 20, 3):
        bad[q] = EC.other_base(bad[q])
    out = E.encode_node(bytes(bad), 0, 20, True, cons, cons, 0.25)
    assert out["verdict"] == E.REJECTED and out["mat_num"] / out["ops_len"] <= 0.75 and len(out["ops"]) >= 20
    # 0 / 0: a trial whose fitted ops are empty is rejected, not an error
    assert E._div(0, 0) != E._div(0, 0) and E._rust_min(float("nan"), 0.9) == 0.9
    assert E.edge_counts(80, [M] * 80) == (79, 79, 80, 80)      # EDGE_LEN clips to the consensus
    assert E.edge_counts(250, [M] * 250) == (99, 99, 101, 101)
    assert E.trim_head_tail_insertion([I, I, I]) == ([], 0, 3)   # the tail is popped first


def test_named_trials_have_the_verdicts_they_are_named_for():
    want = dict(accepted=E.ACCEPTED, lower_bound=E.LOWER_BOUND, lower_bound_equal=None, identity_rejected=E.REJECTED,
                head_edge_rejected=E.REJECTED, tail_edge_rejected=E.REJECTED, forward=E.ACCEPTED, reverse=E.ACCEPTED)
    for name, verdict in want.items():
        out = EC.expected(EC.CASES[name])
        assert verdict is None or out["verdict"] == verdict, name
    assert EC.expected(EC.CASES["lower_bound_equal"])["verdict"] != E.LOWER_BOUND
    for name in ("head_edge_rejected", "tail_edge_rejected"):      # rejected by the edge, not by the identity
        out, t = EC.expected(EC.CASES[name]), EC.CASES[name]
        assert 1.0 - t["sim_thr"] < out["mat_num"] / out["ops_len"], name
    out = EC.expected(EC.CASES["trims_reverse"])
    assert out["trim_head"] > 0 and out["trim_tail"] > 0 and out["trim_head"] != out["trim_tail"]
    assert out["position_from_start"] == EC.CASES["trims_reverse"]["start"] + out["trim_tail"]
    t = EC.CASES["band_is_wider"]
    assert EC.expected(EC.CASES["band_is_10"])["band"] == 10 and EC.expected(t)["band"] == E.band_of(t["end"] - t["start"], 0.5) > 30
    assert EC.expected(EC.CASES["cons_shorter_than_edge"])["head_len"] < 100


def test_fill_trials_is_try_encoding_heads_arithmetic():
    lens = {(7, 0): 200, (8, 1): 95}
    look = lambda chunk, cluster: lens.get((chunk, cluster))
    cands = [(7, 0, True, 500), (7, 0, False, -3), (8, 1, True, 5), (9, 0, True, 50), (7, 0, True, 1000), (8, 1, True, 990)]
    for fn in (E.fill_trials, api.fill_trials):
        # head: offset = ceil(0.1 * len); the negative and the past-the-end position and the unknown consensus drop out
        assert fn(0, cands, 1000, None, look) == [(0, 480, 720), (2, 0, 110), (5, 980, 1000)]
        # is_the_same_encode: the next node is of chunk 7 and starts within a consensus length of the window
        assert fn(0, cands, 1000, (7, 600), look) == [(2, 0, 110), (5, 980, 1000)]
        assert fn(0, cands, 1000, (7, 680), look) == [(0, 480, 720), (2, 0, 110), (5, 980, 1000)]
        # tail: the position is the end
        assert fn(1, [(7, 0, True, 500), (8, 1, True, 40), (7, 0, True, 1200)], 1000, None, look) == [(0, 280, 520), (1, 0, 50), (2, 780, 1000)]
        # a negative tail position is the reference's wrapped usize, on which its assert fails: refused, not turned into a window
        with pytest.raises(ValueError):
            fn(1, [(8, 1, True, -3)], 1000, None, look)
