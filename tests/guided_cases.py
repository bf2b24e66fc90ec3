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


def row_widths(cs):
    band = G.band_cells(len(cs["x"]), len(cs["y"]), cs["guide"], cs["radius"])
    return [hi - lo + 1 for lo, hi in band.values()]
