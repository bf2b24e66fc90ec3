"""tests/settle_reference.py by itself (no device): the chain cases of tests/settle_cases.py against outcomes written by hand,
the statistics against hand-computed numbers, and the identity include/jtk_lc.h states between del_size on the run-length cigar
(what the reference computes) and on per-base ops (what the kernel sees), on 200 random cigars."""
import os
import random
import re

import pytest

import settle_cases as K
import settle_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(K.EXPECTED))
def test_chain_cases_by_hand(name):
    out = R.settle(K.CASES[name], R.BY_CHUNK_POS)
    assert out["order"] == K.EXPECTED[name] and out["rc"] == 0
    want_keep = [1 if i in kept else 0 for read, kept in zip(K.CASES[name], K.EXPECTED[name]) for i in range(len(read))]
    assert out["keep"] == want_keep and out["n_kept"] == [len(k) for k in K.EXPECTED[name]]
    by_chunk = R.settle(K.CASES[name], R.BY_CHUNK)
    assert by_chunk["order"] == K.EXPECTED_BY_CHUNK.get(name, K.EXPECTED[name])


def test_statistics_by_hand():
    stats = R.settle(K.CASES["match_only"], R.STATS_ONLY)["stats"]
    assert [s[3] for s in stats] == [0, -1, -1, -50, -50, -64]          # -(total) / 2 toward zero: the reference keeps it negative
    assert [s[:3] for s in stats] == [(n, n, 0) for n in (1, 2, 3, 100, 101, 129)]
    stats = R.settle(K.CASES["largest_run"], R.STATS_ONLY)["stats"]
    assert [s[3] for s in stats[:5]] == [10, 10, 10, 12, 9]             # 2 * 5 - 1 + 2 * 5 = 19, halved toward zero
    assert stats[0][:3] == (90, 110, 10) and stats[4][:3] == (91, 111, 10)
    assert R.max_region([]) == -(1 << 63) and R.max_region([-3]) == -3 and R.max_region([-3, 4, -1, 4, -9]) == 7


def test_stats_only_and_bad_reads_leave_the_nodes_as_they_came():
    for name in ("bad_empty_ops", "bad_query_len"):
        for mode in (R.STATS_ONLY, R.BY_CHUNK_POS, R.BY_CHUNK):
            out = R.settle(K.CASES[name], mode)
            assert out["status"] == [0, R.UNSUPPORTED, 0] and out["rc"] == -6
            assert out["order"][1] == [0, 1, 2]
            if mode != R.STATS_ONLY:
                assert out["order"][0] == [1, 2] and out["order"][2] == [1, 0]   # the good reads are settled
    out = R.settle(K.CASES["random"], R.STATS_ONLY)
    assert out["order"] == [list(range(len(r))) for r in K.CASES["random"]] and all(out["keep"])


def test_settling_removes_something_somewhere():
    for name in ("nodes_64_65", "lds_limit", "random"):
        out = R.settle(K.CASES[name], R.BY_CHUNK_POS)
        assert all(0 < k < len(r) for k, r in zip(out["n_kept"], K.CASES[name]) if len(r) >= 9), name
        assert out["order"] != R.settle(K.CASES[name], R.BY_CHUNK)["order"], name   # the two modes are told apart
    sizes = sorted(len(r) for r in K.CASES["lds_limit"])
    assert K.LDS_NODES in sizes and K.LDS_NODES + 1 in sizes and K.LDS_NODES - 1 in sizes
    text = open(os.path.join(ROOT, "jtk_amd", "csrc", "settle.hip")).read()
    assert int(re.search(r"ST_LDS_NODES = (\d+);", text).group(1)) == K.LDS_NODES


def test_run_length_and_per_base_del_size_agree():
    rng = random.Random(77)
    seen_negative = seen_multi_run = 0
    for trial in range(200):
        cigar = []
        for _ in range(rng.randint(1, 7)):
            kind = "M" if trial % 10 == 0 else rng.choice("MMID")
            if cigar and cigar[-1][0] == kind:
                continue   # a run-length cigar has no two adjacent runs of a kind
            cigar.append((kind, rng.randint(1, 30)))
        ops = R.per_base(cigar)
        want = R.del_size(cigar)
        assert R.per_base_del_size(ops) == want, cigar
        seen_negative += want < 0
        seen_multi_run += want > max([l for op, l in cigar if op != "M"] or [0])
    assert seen_negative >= 10 and seen_multi_run >= 10
