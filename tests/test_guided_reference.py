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


SIZE_LIMIT = sum(K.row_widths(K.big_pair(200)))      # no newer case costs the reference more band cells than this one


def test_cases_at_the_limits_are_what_they_are_named_for():
    """the widths, lengths, row counts, op counts and scores that the cases at the kernel's limits are built for, and the size
    condition: none of them costs the reference more band cells than big_pair(200)"""
    assert SIZE_LIMIT == 777541
    for name, cs in K.CASES.items():
        assert sum(K.row_widths(cs)) <= SIZE_LIMIT, name
    # ---- global rows up to the cap, and one cell over it
    for width in (1024, 1025, 2047, 2048, 2049, 4096):
        for tag in ("global", "infix"):
            assert set(K.row_widths(K.CASES["rows_of_%d_%s" % (width, tag)])) == {width}
    assert api.ffi.GUIDED_MAX_WIDTH == 4096
    for infix in (False, True):
        assert set(K.row_widths(K.over_cap_pair(infix))) == {4097} and K.over_cap_pair(infix)["infix"] == infix
    # ---- more global-row pairs than the 512 waves that run them, no two alike, LDS-sized pairs in between
    batch = K.large_batch()
    wide = [cs for cs in batch if max(K.row_widths(cs)) > 512]
    assert len(wide) == K.LARGE_BATCH_WIDE >= 520 and len(batch) - len(wide) >= 100
    assert all(513 <= w <= 700 for cs in wide for w in K.row_widths(cs)) and all(1 <= len(K.row_widths(cs)) <= 3 for cs in wide)
    assert all(max(K.row_widths(cs)) <= 512 for cs in batch if cs not in wide)
    assert len({(cs["x"], cs["y"]) for cs in wide}) == len(wide)
    assert {len(K.row_widths(cs)) for cs in wide} == {1, 2, 3}
    # the pairs a wave takes second, on the rows that a wide pair of other content left
    second = [(batch[at - 512], batch[at]) for at in range(512, len(batch)) if batch[at] in wide and batch[at - 512] in wide]
    assert len(second) >= 64 and all(len(a["y"]) != len(b["y"]) or a["y"] != b["y"] for a, b in second)
    assert sum(sum(K.row_widths(cs)) for cs in batch) <= SIZE_LIMIT
    # ---- the length limit and the score range
    for scores, radius in K.LIMIT_RUNS:
        cs = K.limit_pair(scores, radius)
        assert len(cs["x"]) == len(cs["y"]) == K.MAX_LEN == 32000 and sum(K.row_widths(cs)) <= SIZE_LIMIT
        out = K.expected(cs)
        assert G.score_of_ops(cs["x"], cs["y"], out["ops"], out["start"], out["end"], scores) == out["score"]
        if (scores, radius) in ((K.MAX_SCORES[0], 2), (K.MAX_SCORES[1], 1)):
            assert out["score"] < -3e7, (scores, radius, out["score"])
    assert max(abs(s) for scores in K.MAX_SCORES for s in scores) == 1024      # JTK_GUIDED_MAX_SCORE (include/jtk_lc.h)
    over = K.over_length_batch()
    assert (len(over[1]["x"]), len(over[3]["y"])) == (32001, 32001) and all(len(over[p]["x"]) <= 120 for p in (0, 2, 4))
    # ---- the 64-op loads of the walk, the 64-row steps of the prefix sum, the 64-op stores of the walk back
    for length in (63, 64, 65, 128):
        for last in "MDI":
            cs = K.CASES["guide_of_%d_ends_in_skipped_%s" % (length, last)]
            assert len(cs["guide"]) == length
            path = G.guide_path(len(cs["x"]), len(cs["y"]), cs["guide"][:40])
            assert path[-1] == (len(cs["x"]), len(cs["y"]))      # the table's corner after 40 ops: every later op is skipped
            assert cs["guide"][length - 1] == dict(M=M, D=D, I=I)[last] and (length <= 64 or cs["guide"][63] == cs["guide"][length - 1])
    cs = K.CASES["skipped_match_then_dels"]
    path = G.guide_path(50, 20, cs["guide"])      # 63 ops that fit, the M that does not, seven Dels that do
    assert cs["guide"][63] == M and path[63] == (43, 20) and path[64] == (44, 20) and path[-1] == (50, 20) and len(path) == 71
    for rows in (63, 64, 65, 128, 129):
        assert len(K.row_widths(K.CASES["rows%d" % rows])) == rows
    for name, nops in (("nops64", 64), ("nops128", 128), ("nops128_infix", 128)):
        assert len(K.expected(K.CASES[name])["ops"]) == nops, name
    for run in (63, 64, 65):
        out = K.expected(K.CASES["free_runs_of_%d" % run])
        assert (out["start"], out["end"]) == (run, run + 30) and out["ops"] == [D] * run + [M] * 30 + [D] * run


def test_census_of_the_named_cases():
    """every event on the optimal path that the kernel's structure tells apart is provided by a named case: the nine (state,
    predecessor) steps, each of them in the first and in the last column of a 64-column piece behind the first (an I step in the
    first column takes the carried left neighbour), an I gap over two piece boundaries (the carried running maximum, twice), M
    and D steps from the first and the last cell of the row above, and ties between end rows and between end states"""
    found = {}
    for name, cs in K.CASES.items():
        for event in K.events(cs):
            found.setdefault(event, name)
    for event in K.ALL_EVENTS:
        print(event, "<-", found.get(event))
    assert len(K.ALL_EVENTS) == 9 + 18 + 4 + 3
    assert [event for event in K.ALL_EVENTS if event not in found] == []
    # the carried left neighbour of both kinds, by the cases made for it
    assert "I from M at band column 0 mod 64" in K.events(K.CASES["ins_opens_behind_column_127"])
    assert "I from D at band column 0 mod 64" in K.events(K.CASES["ins_run_behind_del_in_column_63"])


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


def test_trials_at_the_edges_of_the_counts_are_what_they_are_named_for():
    out = EC.expected(EC.CASES["cons_len1"])      # 0 / 0 in the head: the verdict is min(NaN, tail) = the tail's
    assert (out["head_len"], out["head_match"], out["tail_len"], out["ops_len"], out["verdict"]) == (0, 0, 1, 1, E.ACCEPTED)
    for n in (99, 100, 101):
        t = EC.CASES["cons_len%d" % n]
        assert len(t["cons"]) == n and EC.expected(t)["verdict"] == E.ACCEPTED
    for lead, trail in ((63, 65), (64, 64), (65, 63)):
        for tag, forward in (("", True), ("_reverse", False)):
            t = EC.CASES["trims_%d_%d%s" % (lead, trail, tag)]
            out = EC.expected(t)
            assert (out["trim_head"], out["trim_tail"]) == (lead, trail) and t["is_forward"] == forward
            assert out["position_from_start"] == t["start"] + (lead if forward else trail)
    assert EC.expected(EC.CASES["ops_len64"])["ops_len"] == 64 and EC.expected(EC.CASES["ops_len128"])["ops_len"] == 128
    assert len(EC.expected(EC.CASES["ops_len64"])["ops"]) == 64
    # the trial with a band of more than 256, under the size condition in each of its passes
    t = EC.wide_band_trial()
    wl = t["end"] - t["start"]
    assert E.band_of(wl, t["sim_thr"]) > 256 and len(t["cons"]) + 1 > 512 and (wl + 1) * (2 * E.band_of(wl, t["sim_thr"]) + 1) <= SIZE_LIMIT
    # the refused trials pass the filter, and the one for the guided pass gets a guide with one Ins run of 4,200
    for t in (EC.refused_by_infix(), EC.refused_by_guided_pass(), EC.refused_by_guided_pass(False), EC.refused_by_length()):
        assert not t["sim_thr"] < max(len(t["cons"]) - (t["end"] - t["start"]), 0) / len(t["cons"])
    assert len(EC.refused_by_infix()["cons"]) == 32001 and len(EC.refused_by_length()["chunk_seq"]) == 32001
    for forward in (True, False):
        t = EC.refused_by_guided_pass(forward)
        window = E.window_of(t["read"], t["start"], t["end"], forward)
        guide = E.first_guide(t["cons"], window)
        assert guide == [M] * 100 + [I] * 4200 + [M] * 100 and len(window) <= 32000 and len(t["cons"]) <= 32000
        assert max(K.row_widths(K.case(window, t["cons"], guide, E.band_of(len(window), t["sim_thr"]), True))) > api.ffi.GUIDED_MAX_WIDTH
    trials, refused = EC.refusal_batch()
    assert sorted(refused) == [0, 4, 6, len(trials) - 1] and [t["sim_thr"] for k, t in enumerate(trials) if k in refused] == [0.97, 0.25, 0.999, 0.97]
    verdicts = [EC.expected(t)["verdict"] for t in EC.shared_trials()]
    assert set(verdicts) == {E.ACCEPTED, E.LOWER_BOUND, E.REJECTED}


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
