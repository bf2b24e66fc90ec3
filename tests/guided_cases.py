"""Named pairs for the guided aligner (tests/guided_reference.py, jtk_lc_align_guided): the smallest shapes at which the
kernel can still go wrong.  A case is dict(x, y, guide, radius, infix, scores); sequences are bytes, the guide a list of op
codes.  The reference's answers are computed once per process (expected / expected_items)."""
import functools

import numpy as np

import guided_reference as G

ACGT = b"ACGT"
M, X, I, D = G.MATCH, G.MISMATCH, G.INS, G.DEL
SCORES = G.ALN_PARAMETER


def random_seq(rng, n, alphabet=4):
    return bytes(ACGT[k] for k in rng.integers(0, alphabet, n))


def mutate_with_guide(rng, x, rate, alphabet=4):
    """-> (y, guide): y is x with substitutions, insertions and deletions at `rate` per base (a third each), the guide is
    the alignment that made it"""
    y, guide = bytearray(), []
    for b in x:
        r = rng.random()
        if r < rate / 3:
            y.append([c for c in ACGT[:alphabet] if c != b][int(rng.integers(0, alphabet - 1))])
            guide.append(X)
        elif r < 2 * rate / 3:
            guide.append(D)
        elif r < rate:
            y.append(ACGT[int(rng.integers(0, alphabet))])
            y.append(b)
            guide += [I, M]
        else:
            y.append(b)
            guide.append(M)
    return bytes(y), guide


def case(x, y, guide, radius, infix=False, scores=SCORES):
    return dict(x=bytes(x), y=bytes(y), guide=list(guide), radius=int(radius), infix=bool(infix), scores=tuple(scores))


def _cases():
    rng = np.random.default_rng(7301)
    c = {}
    # ---- degenerate inputs, in both modes
    for infix in (False, True):
        tag = "infix" if infix else "global"
        c["n0_" + tag] = case(b"", b"ACGT", [I] * 4, 2, infix)
        c["m0_" + tag] = case(b"ACGTA", b"", [D] * 5, 2, infix)
        c["both_empty_" + tag] = case(b"", b"", [], 3, infix)
        c["one_match_" + tag] = case(b"A", b"A", [M], 0, infix)
        c["one_mismatch_" + tag] = case(b"A", b"C", [M], 1, infix)
        x = random_seq(rng, 30)
        c["empty_guide_" + tag] = case(x, mutate_with_guide(rng, x, 0.1)[0], [], 4, infix)
    # ---- radius 0
    x = random_seq(rng, 40)
    y = bytearray(x)
    for q in (3, 17, 18, 39):
        y[q] = ACGT[(ACGT.index(y[q]) + 1) % 4]
    c["radius0_diagonal"] = case(x, y, [M] * 40, 0)
    c["radius0_ins_del"] = case(x, y, [M] * 20 + [I, D] + [M] * 19, 0)   # the corner admits the diagonal
    c["radius0_del_ins"] = case(x, y, [M] * 20 + [D, I] + [M] * 19, 0)
    c["hand_radius1"] = case(b"ACGTACGT", b"ACGACGT", [M] * 7, 1)
    c["hand_radius0"] = case(b"ACGTACGT", b"ACGACGT", [M] * 7, 0)
    c["hand_infix"] = case(b"TTTTACGTACGTGGGG", b"ACGTACGT", [D] * 4 + [M] * 8 + [D] * 4, 2, True)
    c["hand_two_placements"] = case(b"AACCAACC", b"AACC", [M] * 4, 8, True)
    # ---- row widths 63, 64, 65, 128, 129: the carry between the 64-column pieces
    x = random_seq(rng, 40)
    y = mutate_with_guide(rng, x, 0.1)[0] + random_seq(rng, 160)
    c["width63"] = case(x, y, [M] * 40, 31)
    c["width64"] = case(x, y, [M] * 31 + [I, M] * 5 + [M] * 4, 31)      # rows 31 ..= 35 span two columns
    c["width65"] = case(x, y, [M] * 40, 32)
    x = random_seq(rng, 150)
    y = mutate_with_guide(rng, x, 0.1)[0] + random_seq(rng, 60)
    c["width128"] = case(x, y, [M] * 100 + [I, M] * 5 + [M] * 45, 63)
    c["width129"] = case(x, y, [M] * 150, 64)
    c["width129_infix"] = case(x, y[:140], [M] * 150, 64, True)
    # ---- rows of 512 cells and of more: the widest row decides where a wave keeps its two rows of states
    x = random_seq(rng, 300)
    y = mutate_with_guide(rng, x, 0.1)[0]
    y = y + random_seq(rng, 900 - len(y))
    c["width512"] = case(x, y[:511], [M] * 300, 256)          # every row from 255 on is columns i - 256 ..= 511
    c["width513"] = case(x, y[:512], [M] * 300, 256)
    c["width513_infix"] = case(x, y[:512], [M] * 300, 256, True)
    c["width571"] = case(x[:120], y[:570], [M] * 120, 450)
    # ---- one row's span alone crosses a piece: a 70-op Ins run
    x = random_seq(rng, 60)
    y = x[:30] + random_seq(rng, 70) + x[30:]
    c["ins_run70"] = case(x, y, [M] * 30 + [I] * 70 + [M] * 30, 3)
    c["ins_run70_infix"] = case(random_seq(rng, 5) + x + random_seq(rng, 4), y, [D] * 5 + [M] * 30 + [I] * 70 + [M] * 30 + [D] * 4, 3, True)
    # ---- all Del, then all Ins: the band is L-shaped and the answer follows it, not the diagonal
    x = random_seq(rng, 30)
    c["l_shaped"] = case(x, mutate_with_guide(rng, x, 0.05)[0], [D] * 30 + [I] * 40, 2)
    c["l_shaped_infix"] = case(x, x[5:25], [D] * 30 + [I] * 20, 2, True)
    # ---- guides that do not fit: skip and extend
    x = random_seq(rng, 50)
    y, guide = mutate_with_guide(rng, x, 0.15)
    c["guide_longer"] = case(x[:35], y[:30], guide + [M, D, I] * 10, 3)
    c["guide_shorter"] = case(x, y, guide[:20], 3)
    c["guide_other_lengths"] = case(x + b"ACGTA", y[:-5], guide, 5, True)   # fine_mapping's last call: a guide made for other sequences
    # ---- gap and tie choices
    c["one_long_gap"] = case(b"ACGTACGGGGGGTTACGT", b"ACGTACTTACGT", [M] * 12, 8)
    c["two_short_gaps"] = case(b"ACGTAGGCGTACCGTTAG", b"ACGTACGTACGTTAG", [M] * 15, 8)
    c["mismatch_or_two_opens"] = case(b"ACGTACGT", b"ACGAACGT", [M] * 8, 4)
    c["ins_after_del"] = case(b"ACGTACGT", b"ACGAACGT", [M] * 8, 4, scores=(1, -20, -3, -1))
    c["ins_after_del_infix"] = case(b"TTACGTACGTCC", b"ACGAACGT", [M] * 8, 6, True, scores=(1, -20, -3, -1))
    c["all_tie"] = case(b"A" * 12, b"A" * 9, [M] * 9, 20)
    c["all_tie_longer_y"] = case(b"A" * 9, b"A" * 14, [M] * 9, 20)
    c["all_tie_infix"] = case(b"A" * 12, b"A" * 9, [M] * 9, 20, True)
    c["zero_scores"] = case(b"ACGTTGCA", b"ACTTGGCA", [M] * 8, 3, scores=(0, 0, 0, 0))
    for k in range(4):
        x = random_seq(rng, 35, alphabet=2)
        y, guide = mutate_with_guide(rng, x, 0.2, alphabet=2)
        c["low_complexity%d" % k] = case(x, y, guide, (1, 4, 9, 40)[k], k % 2 == 1)
    # ---- infix
    core = random_seq(rng, 60)
    y, guide = mutate_with_guide(rng, core, 0.1)
    c["infix_free_ends"] = case(random_seq(rng, 25) + core + random_seq(rng, 17), y, [D] * 25 + guide + [D] * 17, 6, True)
    c["infix_no_leading_dels_radius2"] = case(random_seq(rng, 10) + core, y, guide, 2, True)   # only rows 0 ..= 2 are free starts
    c["infix_no_leading_dels_radius12"] = case(random_seq(rng, 10) + core, y, guide, 12, True)
    # ---- global rows at their piece and stride boundaries, up to the cap: three bases against m at a radius beyond the matrix,
    # so that each of the four rows is m + 1 cells wide (the 4,097-cell pair that is refused is over_cap_pair)
    rng = np.random.default_rng(7306)
    for width in (1024, 1025, 2047, 2048, 2049, 4096):
        for infix in (False, True):
            x = random_seq(rng, 3)
            y = random_seq(rng, width - 1, alphabet=2)
            c["rows_of_%d_%s" % (width, "infix" if infix else "global")] = case(x, y, [M] * 3, width + 5, infix)
    # ---- the 64-op loads of the band walk: the op that ends a load (index 63, 127) and the last op do not fit and are skipped.
    # x is used up after five ops, so every later M and D is skipped, and after 35 more every I
    x = random_seq(rng, 5)
    y = random_seq(rng, 40)
    filler = [M, D, I, D, M, I, I, D] * 16
    for length in (63, 64, 65, 128):
        for last in (M, D, I):
            guide = [M] * 5 + [I] * 35 + filler[:length - 40]
            guide[length - 1] = last
            if length > 64:
                guide[63] = last
            c["guide_of_%d_ends_in_skipped_%s" % (length, "MDI"[(M, D, I).index(last)])] = case(x, y, guide, 2)
    # the skipped op in the middle of a guide that goes on: y is used up by a 20-op Ins run in row 0, the M at index 63 of the
    # load does not fit, and the Dels behind it do
    x = random_seq(rng, 50)
    c["skipped_match_then_dels"] = case(x, x[:20], [I] * 20 + [D] * 43 + [M] + [D] * 7, 1)
    c["skipped_match_then_dels_infix"] = case(x, x[:20], [I] * 20 + [D] * 43 + [M] + [D] * 7, 1, True)
    # ---- n + 1 = 63, 64, 65, 128, 129 rows: the carry of the prefix sum over the rows' widths
    for rows in (63, 64, 65, 128, 129):
        x = random_seq(rng, rows - 1)
        y, guide = mutate_with_guide(rng, x, 0.1)
        c["rows%d" % rows] = case(x, y, guide, 3, rows % 2 == 0)
    # ---- exactly 64 and 128 ops: the walk back flushes its last 64 ops in the loop and nothing behind it
    x = random_seq(rng, 64)
    c["nops64"] = case(x, x, [M] * 64, 2)
    x = random_seq(rng, 120)
    c["nops128"] = case(x, x[:60] + random_seq(rng, 8) + x[60:], [M] * 60 + [I] * 8 + [M] * 60, 2)
    x = random_seq(rng, 100)
    c["nops128_infix"] = case(random_seq(rng, 17) + x + random_seq(rng, 11), x, [D] * 17 + [M] * 100 + [D] * 11, 3, True)
    # ---- free runs of 63, 64 and 65 Dels in front of and behind an infix placement
    core = random_seq(rng, 30)
    for run in (63, 64, 65):
        c["free_runs_of_%d" % run] = case(random_seq(rng, run) + core + random_seq(rng, run), core, [D] * run + [M] * 30 + [D] * run, 2, True)
    # ---- gaps that open and close on a piece boundary of the band (band column 63 | 64 and 127 | 128): y has no T, a T in x is
    # deleted; x is a few bases of y around the boundary, behind an Ins run that row 0 pays for; the radius is beyond the matrix,
    # so that the band column is the column.  Which event each provides: the census of tests/test_guided_reference.py
    y = random_seq(rng, 140, alphabet=3)
    for col in (63, 127):
        c["ins_opens_behind_column_%d" % col] = case(y[col - 4:col] + y[col + 7:col + 12], y, [], 300)              # an Ins run opens behind a match in column col
        c["match_behind_del_in_column_%d" % col] = case(y[col - 4:col] + b"T" + y[col:col + 6], y, [], 300)       # a match in column col + 1 behind a Del in column col
        c["del_in_column_%d" % (col + 1)] = case(y[col - 4:col + 1] + b"T" + y[col + 1:col + 6], y, [], 300)       # a Del in column col + 1 under a match
        c["match_behind_del_in_column_%d" % (col - 1)] = case(y[col - 5:col - 1] + b"T" + y[col - 1:col + 6], y, [], 300)   # a match in column col behind a Del
    # a Del run down a column and an Ins run on from it along the last row, where a mismatch costs more than both: the band (the
    # guide's own path, and a radius shorter than the Ins run) keeps the other corner, Ins first and Del then, out
    for col, radius, run in ((63, 63, 70), (126, 126, 130)):
        y = random_seq(rng, col - 3, alphabet=2) + b"GGG" + random_seq(rng, run, alphabet=2)      # GGG can match in one place only
        c["ins_run_behind_del_in_column_%d" % col] = case(b"GGGTT", y, [I] * (col - 3) + [M] * 3 + [D] * 2 + [I] * run, radius,
                                                          scores=(1, -20, -3, -1))
    # ---- ties at the largest scores the call takes: every unit is 1,024, with a gap's extension at that price and free
    for scores, tag in (((1024, -1024, -1024, -1024), "s1024"), ((1024, -1024, -1024, 0), "s1024_ext0")):
        for name in ("all_tie", "all_tie_longer_y", "all_tie_infix", "mismatch_or_two_opens", "one_long_gap", "two_short_gaps", "low_complexity0",
                     "low_complexity1", "low_complexity2", "low_complexity3", "hand_two_placements"):
            c[name + "_" + tag] = dict(c[name], scores=scores)
    return c


CASES = _cases()


def mixed_batch(seed=7302, count=70):
    """pairs of every small shape, with guides that fit, guides that do not, and radii from 0 to wider than the matrix"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        x = random_seq(rng, int(rng.integers(0, 121)), alphabet=(4, 4, 2)[k % 3])
        y, guide = mutate_with_guide(rng, x, (0.0, 0.1, 0.3)[k % 3], alphabet=(4, 4, 2)[k % 3])
        if k % 5 == 0:
            y = y + random_seq(rng, int(rng.integers(0, 40)))
        if k % 7 == 0:
            guide = [int(v) for v in rng.integers(0, 4, int(rng.integers(0, 200)))]
        if k % 11 == 0:
            guide = guide[:len(guide) // 2]
        out.append(case(x, y, guide, (0, 1, 2, 5, 16, 33, 70, 400)[int(rng.integers(0, 8))]))
    return out


def over_wide_pair():
    """a 5,000-op Ins run: row 25 of the band spans 5,001 + 2 radius cells, more than JTK_GUIDED_MAX_WIDTH = 4,096"""
    rng = np.random.default_rng(7303)
    x = random_seq(rng, 50)
    y = x[:25] + random_seq(rng, 5000) + x[25:]
    return case(x, y, [M] * 25 + [I] * 5000 + [M] * 25, 4)


def over_cap_pair(infix=False):
    """rows_of_4096 with one base more: four rows of 4,097 cells, one more than JTK_GUIDED_MAX_WIDTH"""
    rng = np.random.default_rng(7307)
    return case(random_seq(rng, 3), random_seq(rng, 4096, alphabet=2), [M] * 3, 5000, infix)


LARGE_BATCH_WIDE = 520


def large_batch(seed=7308):
    """520 pairs of one to three rows by 513 ..= 700 cells (a radius beyond the matrix), more than the 512 waves of the
    global-rows launch, so that waves take a second pair on rows their first one left; every fifth pair in between is one for
    the LDS launch.  No two wide pairs have the same width and content."""
    rng = np.random.default_rng(seed)
    out, wide = [], 0
    while wide < LARGE_BATCH_WIDE:
        if len(out) % 5 == 4:
            x = random_seq(rng, int(rng.integers(1, 40)))
            y, guide = mutate_with_guide(rng, x, 0.2)
            out.append(case(x, y, guide, int(rng.integers(0, 9))))
            continue
        n, m = int(rng.integers(0, 3)), int(rng.integers(512, 700))
        x = random_seq(rng, n)
        y = random_seq(rng, m, alphabet=(4, 2)[wide % 2])
        out.append(case(x, y, [int(v) for v in rng.integers(0, 4, int(rng.integers(0, 6)))], m + 1 + wide % 3))
        wide += 1
    return out


MAX_LEN = 32000      # GD_MAX_LEN of guided.hip
MAX_SCORES = ((1024, -1024, -1024, -1024), (1024, -1024, -1024, 0))      # +- JTK_GUIDED_MAX_SCORE


def limit_pair(scores=SCORES, radius=2):
    """32,000 against 32,000 bases, the longest the call takes, mostly mismatching: x is a run of A with a C every 997 bases, y a
    run of C with an A every 991 bases, so fewer than a hundred columns of any diagonal match.  With every unit at 1,024 the
    score is below -3e7 (asserted in tests/test_guided_reference.py)."""
    x = bytearray(b"A" * MAX_LEN)
    y = bytearray(b"C" * MAX_LEN)
    x[::997] = b"C" * len(x[::997])
    y[::991] = b"A" * len(y[::991])
    return case(x, y, [M] * MAX_LEN, radius, scores=scores)


# (scores, radius) the 32,000-base pair runs at.  The first three are what the limit and the score range ask for; with a free
# extension a radius of 2 lets runs of four gaps undercut four mismatches, so the -3e7 case is at radius 1 and radius 2 is a
# fourth run, whose path is runs of Dels and Ins throughout.
LIMIT_RUNS = ((SCORES, 2), (MAX_SCORES[0], 2), (MAX_SCORES[1], 1), (MAX_SCORES[1], 2))


def over_length_batch(seed=7309):
    """five pairs: pair 1 has 32,001 x bases, pair 3 has 32,001 y bases, the others are small"""
    rng = np.random.default_rng(seed)
    out = mixed_batch(seed, count=5)
    out[1] = case(random_seq(rng, MAX_LEN + 1), random_seq(rng, 20), [M] * 20, 2)
    out[3] = case(random_seq(rng, 20), random_seq(rng, MAX_LEN + 1), [M] * 20, 2)
    return out


def big_pair(radius, infix=False):
    """2,000 against about 2,100 bases at 10 % error, guided by the alignment that made them"""
    rng = np.random.default_rng(7304)
    x = random_seq(rng, 2000)
    y, guide = mutate_with_guide(rng, x, 0.10)
    tail = random_seq(rng, max(0, 2100 - len(y)))
    return case(x, y + tail, guide, radius, infix)


def _key(cs):
    return (cs["x"], cs["y"], tuple(cs["guide"]), cs["radius"], cs["infix"], cs["scores"])


@functools.lru_cache(maxsize=None)
def _expected(key):
    x, y, guide, radius, infix, scores = key
    return G.align_guided(x, y, list(guide), radius, infix=infix, scores=scores)


def expected(cs):
    """the reference's answer for a case, computed once and shared (callers must not change it)"""
    return _expected(_key(cs))


EVENT_STATES = "MDI"


def events(cs):
    """the events on the optimal path of a case that the kernel's structure tells apart (the census of
    tests/test_guided_reference.py): a set of strings"""
    trace = {}
    out = G.align_guided(cs["x"], cs["y"], cs["guide"], cs["radius"], infix=cs["infix"], scores=cs["scores"], trace=trace)
    assert out == expected(cs)
    band, found = trace["band"], set()
    run_end = None
    for state, i, j, pred in trace["steps"]:
        name = "%s from %s" % (EVENT_STATES[state], EVENT_STATES[pred])
        found.add(name)
        col = j - band[i][0]
        if col >= 64 and col % 64 in (0, 63):
            found.add("%s at band column %d mod 64" % (name, col % 64))
        if state == 0 and j - 1 in band[i - 1]:
            found.add("M from the %s cell of the row above" % ("first", "last")[band[i - 1].index(j - 1)])
        if state == 1 and j in band[i - 1]:
            found.add("D from the %s cell of the row above" % ("first", "last")[band[i - 1].index(j)])
        if state == 2:      # (the walk goes back: the run's last cell comes first)
            run_end = col if run_end is None else run_end
            if pred != 2:
                if run_end // 64 - (col - 1) // 64 >= 2:
                    found.add("an I gap over two piece boundaries")
                run_end = None
    if trace["tied_end_rows"] > 1:
        found.add("the end row chosen among tied rows")
    if trace["tied_states"] > 1:
        found.add("the end state chosen among tied states")
    return found


ALL_EVENTS = (["%s from %s" % (a, b) for a in EVENT_STATES for b in EVENT_STATES]
              + ["%s from %s at band column %d mod 64" % (a, b, c) for a in EVENT_STATES for b in EVENT_STATES for c in (0, 63)]
              + ["%s from the %s cell of the row above" % (a, b) for a in "MD" for b in ("first", "last")]
              + ["an I gap over two piece boundaries", "the end row chosen among tied rows", "the end state chosen among tied states"])


def row_widths(cs):
    band = G.band_cells(len(cs["x"]), len(cs["y"]), cs["guide"], cs["radius"])
    return [hi - lo + 1 for lo, hi in band.values()]
