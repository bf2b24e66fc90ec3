"""tests/edge_reference.py (`tune_position`, `encode_edge`, `fill_edges_by_new_chunks` of dense_encoding.rs) against answers
worked out by hand, the named trials of tests/edge_cases.py against what they are named for (a census of events, as
tests/test_guided_reference.py keeps one for the guided aligner), and the host arithmetic of jtk_amd.api.  No GPU."""
import pytest

import edge_cases as EC
import edge_reference as ER
import guided_reference as G
from jtk_amd import api

M, X, I, D = G.MATCH, G.MISMATCH, G.INS, G.DEL


def all_trials():
    return dict(EC.CASES, wide_band=EC.wide_band_trial(), two_kbp=EC.big_trial())


# ---- hand-checked answers

@pytest.mark.parametrize("name", ["error_free", "error_free_reverse"])
def test_error_free_trial_by_hand(name):
    """a 600-base contig in 3 chunks, copied without an error into a 650-base window (25 bases of flank at each end) that
    starts at base 37 of the read: three all-Match nodes of 200 ops.  Forward, chunk k sits at 37 + 25 + 200 k; reverse, the
    window is the reverse complement, so chunk k sits at 687 - 25 - 200 (k + 1)"""
    t = EC.CASES[name]
    out = EC.expected(t)
    assert (t["start"], t["end"]) == (37, 687)
    assert (out["seq_start"], out["seq_end"], out["ctg_start"], out["ctg_end"], out["first_chunk"], out["head_ins"]) == (25, 625, 0, 600, 0, 0)
    assert out["score"] == 2 * 600
    for k, nd in enumerate(out["nodes"]):
        position = 62 + 200 * k if t["is_forward"] else 662 - 200 * (k + 1)
        assert nd == dict(verdict=ER.ACCEPTED, mat_num=200, ops_len=200, query_off=25 + 200 * k, query_len=200, position_from_start=position, ops=[M] * 200)
    got = ER.accepted_nodes(out, t["is_forward"])
    assert [k for k, _, _ in got] == ([0, 1, 2] if t["is_forward"] else [2, 1, 0])
    for k, _, seq in got:
        assert seq == t["chunks"][k]


def test_the_cut_by_hand():
    """the contig AACCGGTT in chunks of 3, 2 and 3 bases against the window CCAGGTAA.  The first alignment keeps CCAGGT: the
    contig's two A are lost in front of it, its last T behind it (a Del there and a Mismatch with the window's A cost the same;
    the smaller end wins).  The second lays CCAGGT on contig[2 .. 7) = CCGGT with the A as an Ins.  The stream is
    2 lead Dels, M | M, I, M | M, M, 1 tail Del"""
    contig, breaks = b"AACCGGTT", [3, 5, 8]
    read = b"GGG" + b"CCAGGTAA"
    out = ER.encode_edge(read, 3, len(read), True, contig, breaks, 5, 0.5)
    assert (out["seq_start"], out["seq_end"], out["ctg_start"], out["ctg_end"]) == (0, 6, 2, 7)
    assert out["first_chunk"] == 0 and out["head_ins"] == 0 and out["score"] == 2 * 5 - 5
    n0, n1, n2 = out["nodes"]
    assert n0["ops"] == [D, D, M] and (n0["mat_num"], n0["query_off"], n0["query_len"], n0["position_from_start"]) == (1, 0, 1, 3)
    assert n1["ops"] == [M, I, M] and (n1["mat_num"], n1["query_off"], n1["query_len"], n1["position_from_start"]) == (2, 1, 3, 4)
    assert n2["ops"] == [M, M, D] and (n2["mat_num"], n2["query_off"], n2["query_len"], n2["position_from_start"]) == (2, 4, 2, 7)
    assert [nd["verdict"] for nd in out["nodes"]] == [ER.REJECTED, ER.ACCEPTED, ER.ACCEPTED]     # 1/3, 2/3, 2/3 against 1 - 0.5
    assert out["closed_by"] == ["op", "op", "tail"]
    # the same window on the other strand: positions count from the window's end, 11 - ypos with ypos = 1, 4, 6
    rev = ER.window_of(read, 3, len(read), False)
    out_r = ER.encode_edge(b"GGG" + rev, 3, len(read), False, contig, breaks, 5, 0.5)
    assert [nd["ops"] for nd in out_r["nodes"]] == [nd["ops"] for nd in out["nodes"]]
    assert [nd["position_from_start"] for nd in out_r["nodes"]] == [10, 7, 5]
    assert [k for k, _, _ in ER.accepted_nodes(out_r, False)] == [2, 1]
    assert [seq for _, _, seq in ER.accepted_nodes(out, True)] == [b"CAG", b"GT"]


# ---- every named trial is what it is named for

def closing_index(out, k):
    """the index in the stream (the pass's ops behind their leading Ins, then the tail Dels) of the op that closes chunk k"""
    lead = out["ctg_start"] - ([0] + out["_breaks"])[out["first_chunk"]]
    return sum(nd["ops_len"] for nd in out["nodes"][out["first_chunk"]:k + 1]) - lead - 1


def census(t):
    out = dict(EC.expected(t), _breaks=EC.break_points(t))
    nodes, first = out["nodes"], out["first_chunk"]
    ev = set()
    ev |= {"verdict %d" % nd["verdict"] for nd in nodes}
    if 0 < first < len(nodes):
        ev.add("first_chunk > 0")
    if out["head_ins"]:
        ev.add("head_ins > 0")
    if "tail" in out["closed_by"]:
        ev.add("closed by a tail Del")
    if first < len(nodes) and nodes[first]["ops"][:1] == [D] and out["ctg_start"] > ([0] + out["_breaks"])[first]:
        ev.add("lead Dels")
    if any(nd["ops"][:1] == [I] for nd in nodes[first + 1:]):
        ev.add("Ins behind a closing op")
    if len(nodes) > 64:
        ev.add("more than 64 slots")
    return out, ev


def test_every_named_trial_is_what_it_is_named_for():
    seen = set()
    facts = {}
    for name, t in all_trials().items():
        out, ev = census(t)
        facts[name] = (out, ev)
        seen |= ev
        wl = t["end"] - t["start"]
        assert out["seq_end"] - out["seq_start"] <= wl and len(EC.contig_of(t)) == out["_breaks"][-1], name
    verdicts = lambda name: [nd["verdict"] for nd in facts[name][0]["nodes"]]      # noqa: E731
    for name in ("lower_case", "lower_case_reverse"):
        assert all_trials()[name]["read"].islower(), name
    for name in ("reverse", "lower_case_reverse", "window_inside_contig_reverse", "error_free_reverse", "chunks_of_3_reverse", "closing_op_64", "leading_ins_64"):
        assert not all_trials()[name]["is_forward"], name
    for name in ("window_inside_contig", "window_inside_contig_reverse"):
        out, ev = facts[name]
        assert verdicts(name) == [ER.REJECTED, ER.ACCEPTED, ER.REJECTED] and {"lead Dels", "closed by a tail Del"} <= ev, name
        assert 0 < out["ctg_start"] < out["_breaks"][0] and out["_breaks"][1] < out["ctg_end"] < out["_breaks"][2], name
    assert facts["begins_behind_chunk0"][0]["first_chunk"] == 1 and verdicts("begins_behind_chunk0")[0] == ER.NOT_REACHED
    assert set(verdicts("error_free")) == {ER.ACCEPTED} and set(verdicts("error_40_percent")) == {ER.REJECTED}
    assert facts["closed_by_virtual_del"][0]["closed_by"] == ["op", "tail", "tail"]
    assert "Ins behind a closing op" in facts["ins_behind_closing_op"][1]
    for name in ("chunks_of_3", "chunks_of_3_reverse"):
        out, ev = facts[name]
        assert "more than 64 slots" in ev and len(out["nodes"]) == 70, name
        closers = [closing_index(out, k) for k in range(70)]
        assert min(sum(64 * b <= c < 64 * (b + 1) for c in closers) for b in range(3)) >= 18, name      # about twenty per block of 64 ops
    assert len(facts["one_chunk"][0]["nodes"]) == 1
    t = all_trials()["contig_longer_than_window"]
    assert len(EC.contig_of(t)) > t["end"] - t["start"]
    t = all_trials()["window_much_longer"]
    assert t["end"] - t["start"] > 5 * len(EC.contig_of(t))
    out = facts["nothing_aligns"][0]
    assert out["seq_start"] == out["seq_end"] and out["first_chunk"] == 2 and set(verdicts("nothing_aligns")) == {ER.NOT_REACHED}
    for n in (63, 64, 65):
        out = facts["closing_op_%d" % n][0]
        assert out["head_ins"] == 0 and closing_index(out, 0) == n, n
        assert facts["leading_ins_%d" % n][0]["head_ins"] == n, n
    assert all_trials()["wide_band"]["radius"] > 256 and len(EC.contig_of(all_trials()["wide_band"])) + 60 == 860
    t = all_trials()["two_kbp"]
    assert len(EC.contig_of(t)) == 2000 and len(t["chunks"]) == 2
    assert seen >= {"verdict 0", "verdict 2", "verdict 3", "first_chunk > 0", "head_ins > 0", "closed by a tail Del", "lead Dels", "Ins behind a closing op",
                    "more than 64 slots"}, seen


def test_batch_of_70_holds_the_named_trials():
    trials = EC.batch70()
    assert len(trials) == 70 and all(a is b for a, b in zip(trials, EC.CASES.values()))
    refused, where = EC.refusal_batch()
    assert len(refused[0]["read"]) == 32001 and all(len(EC.contig_of(refused[k])) + refused[k]["end"] - refused[k]["start"] >= 32768 for k in (4, len(refused) - 1))
    assert sorted(where) == [0, 4, len(refused) - 1]


# ---- fill_edges_by_new_chunks

def hand_read():
    """four nodes (chunk, cluster, is_forward, position, seq length) on a read of 1,000 bases"""
    nodes = [(7, 0, True, 100, 200), (8, 1, True, 400, 200), (9, 0, False, 560, 150), (3, 2, True, 800, 150)]
    edges = {
        ((7, 0, True), (8, 1, True)): ["e78a", "e78b"],          # the forward key of gap 0
        ((9, 0, True), (8, 1, False)): ["e98"],                  # the reverse key of gap 1, whose window is empty: 600 - 25 >= 560 + 25 is false ...
        ((3, 2, False), (9, 0, True)): ["e39"],                  # the reverse key of gap 2
    }
    tips = {
        (7, 0, True, False): [["h1"], ["h2a", "h2b"]],           # head tip, the first key
        (7, 0, False, True): [["hbug"]],                         # head tip, the key marked "Here is a bug"
        (3, 2, True, True): [["t1"]],                            # tail tip, the first key
        (3, 2, False, False): [["t2"]],                          # tail tip, the second key
        (8, 1, True, True): [["never"]],                         # a tip of a node that is neither first nor last
    }
    return nodes, edges, tips


def test_edge_trials_by_hand():
    nodes, edges, tips = hand_read()
    # gap 1: start = 400 + 200 - 25 = 575, end = 560 + 25 = 585: a window; move node 2 forward so that end <= start
    nodes[2] = (9, 0, False, 545, 150)                           # end = 570 <= start = 575: skipped ("TooNear")
    want = [(0, 0, 125, True, ["h1"]), (0, 0, 125, True, ["h2a", "h2b"]), (0, 0, 125, False, ["hbug"]),
            (1, 275, 425, True, ["e78a", "e78b"]),
            (3, 670, 825, False, ["e39"]),                       # 545 + 150 - 25, 800 + 25
            (5, 925, 1000, True, ["t1"]), (5, 925, 1000, False, ["t2"])]
    assert ER.fill_edges_by_new_chunks(nodes, 1000, edges, tips) == want
    got = api.edge_trials(nodes, 1000, edges, tips, band_width_of=lambda n: 7 + n, sim_thr=0.3)
    assert [(g["insert_at"], g["start"], g["end"], g["is_forward"], g["chunks"]) for g in got] == want
    assert [g["radius"] for g in got] == [7 + sum(len(c) for c in w[4]) for w in want] and {g["sim_thr"] for g in got} == {0.3}
    # with the gap open again the reverse key of gap 1 is used
    nodes[2] = (9, 0, False, 560, 150)
    got = api.edge_trials(nodes, 1000, edges, tips, band_width_of=lambda n: 10, sim_thr=0.3)
    assert (2, 575, 585, False, ["e98"]) in [(g["insert_at"], g["start"], g["end"], g["is_forward"], g["chunks"]) for g in got]
    # the forward key goes before the reverse key
    edges[((8, 1, True), (9, 0, False))] = ["e89"]
    got = ER.fill_edges_by_new_chunks(nodes, 1000, edges, tips)
    assert (2, 575, 585, True, ["e89"]) in got and all(g[4] != ["e98"] for g in got)
    # the ends of the read clamp the windows; a read without nodes has no trial
    short = [(7, 0, True, 5, 10)]
    assert ER.fill_edges_by_new_chunks(short, 12, {}, tips) == [(0, 0, 12, True, ["h1"]), (0, 0, 12, True, ["h2a", "h2b"]), (0, 0, 12, False, ["hbug"])]
    assert api.edge_trials([], 1000, edges, tips, lambda n: 10, 0.3) == [] and ER.fill_edges_by_new_chunks([], 1000, edges, tips) == []


# ---- consensus: the host part

def test_edge_consensus_plan():
    seq = lambda n, fill=b"A": fill * n      # noqa: E731
    # lengths 450, 500, 430, 460, 2000, 100: ascending 100 430 450 460 500 2000, the median is index 3 = 460
    seqs = [seq(450), seq(500), seq(430), seq(460, b"C"), seq(2000), seq(100)]
    kept, band = api.edge_consensus_plan(seqs, 3)
    assert kept[0] == seq(460, b"C")                                       # the draft first
    assert [len(s) for s in kept] == [460, 500, 430, 450]                  # [230, 920): the swap, then 2,000 and 100 dropped
    assert band == (460 + 500 + 430 + 450) // 4 // 20 == 23
    assert api.edge_consensus_plan(seqs, 4) is None                        # at most cov_thr sequences remain
    assert api.edge_consensus_plan([seq(450), seq(450, b"C"), seq(450, b"G")], 0)[0][0] == seq(450)      # the first of the median's length
    assert api.edge_consensus_plan([seq(10001)] * 3, 1) is None            # a median above 10,000
    assert api.edge_consensus_plan([seq(10000)] * 3, 1)[1] == 50
    assert api.edge_consensus_plan([seq(100)] * 3, 0) is None              # 200 <= 400 / 2
    assert api.edge_consensus_plan([seq(101)] * 3, 0) is None              # 202 > 200, but no sequence lies in [200, 202)
    assert api.edge_consensus_plan([seq(150), seq(210), seq(205)], 0)[1] == 10      # [200, 410): 210 and 205 stay, 207 // 20 = 10
