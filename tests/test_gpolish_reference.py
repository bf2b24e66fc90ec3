"""The reference of the guided polish (tests/gpolish_reference.py) against its own specification, DESIGN.md section 4, "Guided
polishing": no GPU.  The device is compared with it in tests/test_gpu_gpolish.py."""
import numpy as np
import pytest

import gpolish_cases as K
import gpolish_reference as gp
from guided_reference import band_cells
from phmm_reference import edited, inactive


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


def band_widths(tmpl, read, guide, radius):
    band = band_cells(len(tmpl), len(read), np.asarray(guide).tolist(), radius)
    return [hi - lo + 1 for lo, hi in band.values()]


SIZE_LIMIT = 777541      # the band cells of guided_cases.big_pair(200): no case here costs the reference more for one read


def test_ring_cases_have_the_widths_they_are_named_for():
    """the storage path of every read of the cases made for the global ring: m + 1 <= 512 reserves no ring, a widest row of at
    most 512 cells is kept in LDS, a wider one in the ring, up to 4,096"""
    def widest(name):
        tmpl, reads, guides, radius = K.TABLE[name]()
        return len(tmpl), [(len(r), max(band_widths(tmpl, r, g, radius)), sum(band_widths(tmpl, r, g, radius))) for r, g in zip(reads, guides)]
    for n in (1, 5, 12):
        got_n, reads = widest("ring_n%d_wide" % n)
        assert got_n == n and [m for m, _, _ in reads] == [513, 600, 700] and all(w == m + 1 for m, w, _ in reads)
        got_n, reads = widest("ring_n%d_ins_run" % n)
        assert got_n == n and all(m == n + 520 and 521 <= w <= 525 and cells <= 525 + 5 * n for m, w, cells in reads)
    _, reads = widest("ring_mixed_block")
    kinds = ["none" if m + 1 <= 512 else "lds" if w <= 512 else "ring" for m, w, _ in reads]
    assert kinds == ["none", "lds", "ring", "ring", "ring", "none", "lds", "ring"]      # two blocks of four waves, each with all three
    _, reads = widest("ring_width4096")
    assert reads[0][:2] == (4095, 4096) and reads[1][1] <= 512
    for name in K.TABLE:
        assert all(cells <= SIZE_LIMIT for _, _, cells in widest(name)[1]), name
    # the polish case stays in the ring over its rounds: the radius is beyond every read, and every read is longer than 512
    c = K.case("ring_rounds")
    log = K.rounds_log("ring_rounds")
    assert len(log) == 2 and log[0][1] != log[1][1] and len(K.expected("ring_rounds")[0]) != log[1][1]      # n differs from round to round
    assert all(len(r) + 1 > 512 and c["radius"] > len(r) for r in c["reads"])


def test_sixteen_bit_cells_above_32767():
    """the distance and the largest stored F of the two f16 cases lie above 32,767 and below 65,535, the stored infinity; the
    band admits so little that the banded distance is far above the edit distance (n substitutions)"""
    for name, (tmpl, reads, guides, radius) in (("table", K.TABLE["f16_table"]()), ("polish", K.f16_case(K.MAX_LEN, 1))):
        dist, _ops, F, _band = gp.fill(tmpl, reads[0], guides[0], radius)
        top = max(F.values())
        print(name, "n", len(tmpl), "dist", dist, "largest F", top, "cells", len(F))
        assert 32767 < dist <= top < 65535 and len(tmpl) < dist and len(F) <= SIZE_LIMIT
    assert len(K.case("f16_polish")["tmpl"]) == len(K.case("f16_polish")["reads"][0]) == 32000
    assert K.table_expected("f16_table")[1][0][0] > 32767 and K.expected("f16_polish")[2][0] > 32767


def test_refused_pileups_and_what_the_reference_does_with_them():
    assert len(K.case("too_long_template")["tmpl"]) == 32001 and len(K.case("too_long_read")["reads"][1]) == 32001
    # the reference has no buffers to outgrow: it goes on to a consensus far longer than the device's tmpl_cap = n + 64 + n / 8
    c = K.case("outgrows")
    cons = K.expected("outgrows")[0]
    assert len(c["tmpl"]) == 40 and K.OUTGROWS_CAP == 109 and len(cons) > 2 * K.OUTGROWS_CAP
    assert any(n > K.OUTGROWS_CAP for _t, n, _g, _d, _e in K.rounds_log("outgrows"))


def census():
    """event -> the polish case that provides it, from the rounds of every named polish case"""
    found = {}
    for name in sorted(K.POLISH):
        e = K.case(name)["ignore_edge"]
        for t, n, gain, dead, edits in K.rounds_log(name):
            grow = 0
            for pos, row in edits:
                found.setdefault("row %d applied" % row, name)
                grow += 1 if 4 <= row < 8 else row - 7 if 8 <= row < 11 else 10 - row if row >= 11 else 0
                if 4 <= row <= 10 and pos == 0:
                    found.setdefault("an insertion edit at position 0", name)
                if row >= 11 and pos + (row - 10) == n - 1:
                    found.setdefault("a delete edit that ends at n - 2, the last that exists", name)
            for (a, row), (b, _) in zip(edits, edits[1:]):
                if b - a == (row - 10 if row >= 11 else 1) + inactive(t):
                    found.setdefault("two edits as close as inactive lets them be", name)
                if row < 11 and b - a == 1 + inactive(t):
                    found.setdefault("two edits 1 + inactive apart", name)
            if grow >= 3:
                found.setdefault("a round that adds three bases or more", name)
            if grow <= -3:
                found.setdefault("a round that removes three bases or more", name)
            for pos in [p for p in range(n) if p < e or p + e >= n]:
                alive = [int(gain[pos, q]) for q in range(gp.NUM_ROW) if not dead[pos, q]]
                if alive and max(alive) >= 1:
                    found.setdefault("ignore_edge cuts off an edit that would apply", name)
    return found


# Copying one base (row 8) makes the template that inserting that base (rows 4-7) makes, and the first best row wins: where the
# band holds both entries row 8 is never applied.  It is compared entry by entry in the tables, not as an edit.
CENSUS = ["row %d applied" % row for row in range(gp.NUM_ROW) if row != 8] + [
    "an insertion edit at position 0", "a delete edit that ends at n - 2, the last that exists", "two edits 1 + inactive apart",
    "two edits as close as inactive lets them be", "a round that adds three bases or more", "a round that removes three bases or more",
    "ignore_edge cuts off an edit that would apply"]


def test_census_of_the_polish_cases():
    """which case makes the scan and the surgery take which turn: every row but 8 as the applied edit, and the edits at the edges.
    A delete edit never reaches n - 1 (edited() has none with p + d >= n), so the last one that exists stands for it"""
    found = census()
    for event in CENSUS:
        print(event, "<-", found.get(event))
    assert [event for event in CENSUS if event not in found] == []
    assert all(edited(np.zeros(9, dtype=np.uint8) + 65, 9 - d, 10 + d) is None for d in (1, 2, 3))
