"""The reference of the guided polish (tests/gpolish_reference.py) against its own specification, DESIGN.md section 4, "Guided
polishing": no GPU.  The device is compared with it in tests/test_gpu_gpolish.py."""
import numpy as np
import pytest

import gpolish_cases as K
import gpolish_reference as gp
from phmm_reference import edited


def test_wide_table_is_the_unbanded_distance_to_the_edited_template():
    """at a radius beyond both lengths every existing entry is the edit distance of the read to edited(); random pairs, n <= 14"""
    rng = np.random.RandomState(1)
    entries = 0
    for _ in range(30):
        x, y = K.random_seq(rng, rng.randint(1, 15)), K.random_seq(rng, rng.randint(0, 18))
        dist, T, ops = gp.table(x, y, gp.global_ops(x, y), 40)
        assert dist == gp.edit_distance(x, y) == gp.consumes(ops, x, y)
        for p in range(len(x) + 1):
            for row in range(gp.NUM_ROW):
                e = edited(x, p, row)
                if e is not None:
                    assert T[p, row] == gp.edit_distance(e, y), (x, y, p, row)
                    entries += 1
    assert entries > 2000


def test_hand_value():
    """template ACGACGT, read ACGTACGT: one base apart, and inserting T before position 3 makes them equal"""
    x, y = gp.as_seq(b"ACGACGT"), gp.as_seq(b"ACGTACGT")
    dist, T, ops = gp.table(x, y, gp.global_ops(x, y), 20)
    assert dist == 1 and ops.tolist().count(gp.INS) == 1
    assert dist - T[3, 4 + 3] == 1
    assert int((dist - T[T != gp.DEAD]).max()) == 1
    # the other way round the read lacks the base: deleting one of the template's does it
    dist, T, _ = gp.table(y, x, gp.global_ops(y, x), 20)
    assert dist == 1 and dist - T[3, 11] == 1


def test_dead_entries_are_the_edits_that_do_not_exist_when_the_radius_is_wide():
    rng = np.random.RandomState(2)
    for n in (1, 2, 3, 4, 9):
        x, y = K.random_seq(rng, n), K.random_seq(rng, n + 1)
        _, T, _ = gp.table(x, y, gp.global_ops(x, y), 50)
        for p in range(n + 1):
            for row in range(gp.NUM_ROW):
                assert (T[p, row] == gp.DEAD) == (edited(x, p, row) is None), (n, p, row)
        # substitutions stop at p = n, copies of c at p + c > n, deletions of d at p + d >= n; an insertion always exists
        assert (T[n, :4] == gp.DEAD).all() and (T[n, 4:8] != gp.DEAD).all() and (T[n, 8:] == gp.DEAD).all()


def test_a_narrow_band_kills_entries_and_never_undercuts_the_wide_table():
    (tmpl, reads, guides, _), _ = K.table_expected("n12_r40")
    for rd, g in zip(reads, guides):
        _, wide, _ = gp.table(tmpl, rd, g, 40)
        d0, narrow, _ = gp.table(tmpl, rd, g, 0)
        assert d0 == gp.consumes(g, tmpl, rd)                  # radius 0: the band is the guide's path
        alive = narrow != gp.DEAD
        assert (narrow[alive] >= wide[alive]).all() and (wide[alive] != gp.DEAD).all()
        assert (~alive).sum() > (wide == gp.DEAD).sum()


@pytest.mark.parametrize("name", sorted(K.POLISH))
def test_polish_returns_ops_that_consume_both_sequences(name):
    c = K.case(name)
    cons, opss, dists, rounds = K.expected(name)
    assert len(opss) == len(dists) == len(c["reads"]) and 1 <= rounds <= gp.MAX_ROUNDS
    for ops, rd, d in zip(opss, c["reads"], dists):
        assert gp.consumes(ops, cons, rd) == d
    if not c["reads"] or 2 * c["ignore_edge"] >= len(c["tmpl"]):
        assert bytes(cons) == bytes(c["tmpl"]) and rounds == 1


@pytest.mark.parametrize("name", sorted(K.PLANTED))
def test_planted_cases_return_the_truth(name):
    """the reference alone recovers the truth and stays under the round limit, before any kernel is compared"""
    c = K.case(name)
    cons, _, _, rounds = K.expected(name)
    assert bytes(c["tmpl"]) != bytes(c["truth"])
    assert bytes(cons) == bytes(c["truth"]) and 2 <= rounds < gp.MAX_ROUNDS


def test_round_limit_leaves_ops_of_the_returned_consensus():
    """one_round stops after a round that applied edits: the consensus differs from the template, and the extra fill made the ops
    and distances belong to it"""
    c = K.case("one_round")
    cons, opss, dists, rounds = K.expected("one_round")
    assert rounds == 1 and bytes(cons) != bytes(c["tmpl"]) and bytes(cons) != bytes(c["truth"])
    for ops, rd, d in zip(opss, c["reads"], dists):
        assert gp.consumes(ops, cons, rd) == d == gp.fill(cons, rd, ops, c["radius"])[0]


def test_take_num_and_ignore_edge_change_the_vote_not_the_reads():
    all_votes, three = K.expected("planted70"), K.expected("take3of8")
    assert len(three[1]) == 8 and len(three[2]) == 8            # every read is re-threaded and measured
    c = K.case("ignore_edge3")
    x, gain, dead = c["tmpl"], *gp.gains(c["tmpl"], c["reads"], c["ops"], c["radius"], 0)[:2]
    edits = gp.select(gain, dead, 3, 0, len(x))
    assert all(3 <= pos < len(x) - 3 for pos, _ in edits)
    assert all(b - a >= 6 for (a, _), (b, _) in zip(edits, edits[1:]))
    assert all_votes[3] >= 2


def test_first_best_row_on_a_homopolymer():
    """inserting the run's base and copying one base give the same template: the insert row comes first"""
    (tmpl, reads, guides, radius), want = K.table_expected("homopolymer")
    gain, dead, _, _ = gp.gains(tmpl, reads[:1], guides[:1], radius, 0)       # the read with one A more
    assert gain[2, 4] == gain[2, 8] == 1
    assert gp.select(gain, dead, 0, 0, len(tmpl))[0] == (0, 4)
