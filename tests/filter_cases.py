"""Planted input for the variant filter and the pick (jtk_amd/csrc/filter_kernels.hip through jtk_lc_debug_filter): pure numpy, no
GPU, no oracle.  tests/test_filter_reference.py evaluates the cases with tests/clustering_reference.py (filter_candidates,
pick_filtered_profiles, compress_small_gains, homopolymer_lengths, pvalues) and asserts from that record that every case
reaches the branch it names (REACHES); tests/golden/filter_reference.json holds the record; tests/test_gpu_filter.py hands the
same input to the device.

A case is one call: dict(mode "table" | "rows", coverage (haploid), gains (None: the default ones), chunks).  A table chunk is
dict(tmpl, strands, copy_num, table [n, 14 (L + 1)]): the per-read table minus the read's likelihood, as planted_profiles()
makes it -- -2 where nothing is planted (compress_small_gains turns it into 0), +6 in a planted column's carriers and -6 in its
other reads, unless a case says otherwise.  A row-sum chunk is dict(tmpl, strands, copy_num, rows [n, L + 1, 16], exps
[n, L + 1], lk [n]): the pair-HMM's row sums as DESIGN.md section 4 ("Row sums") lays them out; table_from_row_sums turns them
into the table.  Every number is a literal, a power of two times a short mantissa, or a sum of such: a case is the same bytes
on every machine (input_sha256).
"""
import hashlib
from fractions import Fraction

import numpy as np

NUM_ROW, ACC_N, MASK_LENGTH, MAX_DIM = 14, 16, 7, 21
POS_THR = 0.00001
LOG_ZERO, LN2 = -1.0e300, 0.6931471805599453094
BG, HI = -2.0, 6.0
DEL1 = 11   # the one deletion row filter_profiles looks at


def seq(s):
    return np.frombuffer(s.encode(), dtype=np.uint8).copy()


def planted_profiles():
    """A pile-up at the filter's interface: 12 reads (6 per strand, alternating) on a 60 bp template without runs except AAAA
    at 30..33; every entry -2 (no gain), and columns planted with +6 in the six carriers (three per strand) and -6 elsewhere,
    one to pass and one to fail each filter of filter_profiles (:440-465) on its own.  Returns (template, profiles, strands,
    {name: (bp, row)}, {name: the filter that must drop it, None for the columns that must stay})."""
    tmpl = seq("ACGTCAGTCTGACTGATCGATGCATGCTAC" + "AAAA" + "CGTACTGACGTCATGCAGTCGATCGT")
    tl, n = len(tmpl), 12
    assert tl == 60
    strands = [r % 2 == 0 for r in range(n)]
    carriers = [0, 1, 2, 3, 4, 5]                 # three forward, three reverse
    forward_only = [r for r in range(n) if strands[r]]
    prof = np.full((n, 14 * (tl + 1)), -2.0)
    where = dict(passes=(20, 1), passes_too=(12, 6), edge_low=(6, 1), edge_high=(55, 2), first_kept=(7, 1), last_kept=(54, 0), ins_in_run=(31, 4),
                 del_in_run=(31, 11), ins_next_to_its_base=(22, 4 + "ACGT".index(chr(tmpl[22]))), strand_biased=(40, 2), small_gain=(46, 3),
                 copy_row=(26, 9), copy_row_10=(44, 10), del_2=(16, 12))
    why = dict(passes=None, passes_too=None, edge_low="edge", edge_high="edge", first_kept=None, last_kept=None, ins_in_run="homopolymer",
               del_in_run="homopolymer", ins_next_to_its_base=None, strand_biased="strand", small_gain="gain_per_count", copy_row="row",
               copy_row_10="row", del_2="row")
    for name, (bp, row) in where.items():
        who = forward_only if name == "strand_biased" else carriers
        value = 3.0 if name == "small_gain" else 6.0
        prof[:, bp * 14 + row] = [value if r in who else -6.0 for r in range(n)]
    return tmpl, prof, strands, where, why


# ---------------------------------------------------------------------------------------------------------------------------
# building blocks
# ---------------------------------------------------------------------------------------------------------------------------
def plain_template(L, shift=0):
    """L bases without a run of two: ACGT shifted by one every four bases"""
    i = np.arange(L)
    return np.frombuffer(b"ACGT", dtype=np.uint8)[(i + i // 4 + shift) % 4].copy()


def other_base(tmpl, bp, k=1):
    """the row (0..3) of a base that is neither tmpl[bp - 1] nor tmpl[bp]"""
    near = {b"ACGT".index(bytes([int(tmpl[q])])) for q in (bp - 1, bp) if 0 <= q < len(tmpl)}
    return [b for b in range(4) if b not in near][k % 2]


def alternating(n):
    return [r % 2 == 0 for r in range(n)]


def table_chunk(tmpl, n, copy_num, plants, strands=None):
    """plants: (bp, row, carriers) or (bp, row, carriers, hi) or (bp, row, values [n])"""
    table = np.full((n, NUM_ROW * (len(tmpl) + 1)), BG)
    where = []
    for pl in plants:
        bp, row, who = pl[0], pl[1], pl[2]
        if isinstance(who, np.ndarray):
            col = who
        else:
            hi = pl[3] if len(pl) > 3 else HI
            col = np.array([hi if r in who else -HI for r in range(n)])
        table[:, bp * NUM_ROW + row] = col
        where.append(bp * NUM_ROW + row)
    return dict(tmpl=np.asarray(tmpl, dtype=np.uint8), strands=alternating(n) if strands is None else list(strands), copy_num=copy_num,
                table=table, planted=where)


def case(mode, chunks, coverage=5.0, gains=None, reverse_emit=None):
    return dict(mode=mode, chunks=chunks, coverage=float(coverage), gains=gains, reverse_emit=reverse_emit)


def gains_of(H, subst=None):
    """gain profiles that differ per homopolymer length, so that the clamp min(h, H) shows"""
    return dict(subst=[(3.0 + 0.5 * h if subst is None else subst, 0.02 - 0.001 * h) for h in range(H)],
                deletions=[(3.2 + 0.4 * h, 0.04 - 0.002 * h) for h in range(H)],
                insertions=[(3.1 + 0.45 * h, 0.03 - 0.001 * h) for h in range(H)])


SIX_OF_8 = [0, 1, 2, 3, 4, 5]


# ---------------------------------------------------------------------------------------------------------------------------
# table cases
# ---------------------------------------------------------------------------------------------------------------------------
def planted_60():
    """planted_profiles() itself: every filter once, on the device's table path"""
    tmpl, prof, strands, where, _ = planted_profiles()
    return case("table", [dict(tmpl=tmpl, strands=strands, copy_num=2, table=prof, planted=[bp * 14 + row for bp, row in where.values()])])


TILE_EDGE_LENGTHS = (126, 127, 128, 129, 141)


def tile_edges():
    """five chunks in one call (the grid is the longest one's): columns on both sides of a 128-thread block of column_filter_kernel
    (127 | 128, and 14 bp + row around 1792 = 14 * 128), the first and last kept positions, their neighbours beyond the mask, and
    the deletion row at the last kept position"""
    chunks = []
    for j, L in enumerate(TILE_EDGE_LENGTHS):
        tmpl = plain_template(L, j)
        last = L + 1 - MASK_LENGTH
        plants = [(6, 1, SIX_OF_8), (7, 2, SIX_OF_8), (9, 1, SIX_OF_8), (9, 2, SIX_OF_8, 6.5), (last, 0, SIX_OF_8), (last, DEL1, SIX_OF_8, 6.25),
                  (last + 1, 3, SIX_OF_8), (60, 5, SIX_OF_8)]
        if last > 128:
            plants += [(127, 13, SIX_OF_8), (128, 0, SIX_OF_8, 6.75)]   # columns 1791 and 1792; row 13 is never a candidate
        chunks.append(table_chunk(tmpl, 8, 2, plants))
    return case("table", chunks)


def short_templates():
    """L = 12: no live position (7 <= bp <= L + 1 - 7 is empty); 13: exactly bp = 7; 14: 7 and 8"""
    return case("table", [table_chunk(plain_template(L, L), 8, 2, [(bp, 1 + bp % 2, SIX_OF_8) for bp in (5, 6, 7, 8)]) for L in (12, 13, 14)])


THRESHOLD_GAIN = 5.0   # min_req = 2.5 and expt = 5.0 * 0.8 == 4.0 in doubles


def thresholds():
    """substitution gain 5.0, so that the strict comparisons have exact boundaries: |x| == min_req = 2.5 is kept (`<`) and
    nextafter(2.5, 0) is zeroed (the count and the score differ); count x expt == gain (six times 4.0 against 24.0) is dropped,
    2^-40 more (the sum stays exact) passes"""
    assert THRESHOLD_GAIN * 0.8 == 4.0
    n, six = 12, [0, 1, 2, 3, 4, 5]
    col = lambda extra: np.array([HI] * 6 + [extra] + [-HI] * 5)   # noqa: E731
    four = lambda first: np.array([first] + [4.0] * 5 + [-HI] * 6)   # noqa: E731
    plants = [(10, 1, col(2.5)), (20, 1, col(np.nextafter(2.5, 0.0))), (30, 1, col(-2.5)), (40, 1, col(-np.nextafter(2.5, 0.0))),
              (50, 2, four(4.0)), (60, 2, four(4.0 + 2.0 ** -40)), (70, 0, six)]
    return case("table", [table_chunk(plain_template(90), n, 2, plants)], gains=gains_of(3, subst=THRESHOLD_GAIN))


def thresholds_pos_thr():
    """substitution gain 2 x POS_THR, so that min_req == POS_THR and nothing is compressed away: a value of exactly POS_THR is not
    counted and nextafter above it is (count 6 / 7); |x| == 0.0001 is counted but stays out of the strand x sign table (11 entries)
    and nextafter above it is in (12); -0.0 in a column that is picked: its feature is +0.0"""
    g = 2.0 * POS_THR
    assert g * 0.5 == POS_THR
    n = 12
    base = [HI, HI, HI, HI, HI, HI, -HI, -HI, -HI, -HI, -HI, -HI]
    col = lambda r, v: np.array(base[:r] + [v] + base[r + 1:])   # noqa: E731
    plants = [(10, 1, col(11, POS_THR)), (20, 1, col(11, np.nextafter(POS_THR, 1.0))), (30, 2, col(11, -0.0001)),
              (40, 2, col(11, -np.nextafter(0.0001, 1.0))), (50, 3, col(11, -0.0)), (60, 0, col(11, 0.0001))]
    ch = table_chunk(plain_template(80), n, 2, plants)
    return case("table", [ch], gains=gains_of(3, subst=g))


# strand x sign cells (obs[strand][sign]: reverse-, reverse+, forward-, forward+) of the two chi-square columns: chi-square 8.22..
# and 10.66.. (tests/test_filter_reference.py recomputes them)
CHISQ_BELOW = (9, 3, 2, 10)
CHISQ_ABOVE = (10, 2, 2, 10)


def _cells_column(cells, strands):
    """+6 / -6 per read so that the strand x sign table is `cells`: each strand's positives first"""
    r_neg, r_pos, f_neg, f_pos = cells
    left = {(False, 0): r_neg, (False, 1): r_pos, (True, 0): f_neg, (True, 1): f_pos}
    col = []
    for s in strands:
        sg = 1 if left[(s, 1)] > 0 else 0
        left[(s, sg)] -= 1
        col.append(HI if sg else -HI)
    assert not any(left.values())
    return np.array(col)


def strand_and_sign():
    """chunk 0: every read forward -- a strand is absent, the chi-square is NaN and every column goes; chunk 1: a column whose
    counted values are all positive (the others are 0 after compression) -- a sign is absent; two columns with the four cells
    CHISQ_BELOW / CHISQ_ABOVE on either side of 10"""
    n = 24
    strands = alternating(n)
    one = table_chunk(plain_template(50), 12, 2, [(20, 1, [0, 1, 2, 3, 4, 5]), (30, 2, [0, 2, 4, 6, 8, 10])], strands=[True] * 12)
    all_pos = np.array([HI] * 10 + [BG] * 14)
    two = table_chunk(plain_template(70, 1), n, 2, [(15, 1, all_pos), (30, 2, _cells_column(CHISQ_BELOW, strands)),
                                                    (45, 3, _cells_column(CHISQ_ABOVE, strands)), (55, 0, list(range(10)))], strands=strands)
    return case("table", [one, two])


RUNS = (1, 2, 3, 8, 9, 300)


def _run_template():
    """runs of RUNS bases between run-free stretches of 9 (none of which begins or ends with a neighbouring run's base):
    returns the template and each run's first position"""
    def stretch(length, not_first, not_last):
        for shift in range(16):
            t = plain_template(length, shift)
            if t[0] != not_first and t[-1] != not_last:
                return t
        raise AssertionError("no stretch")
    parts, starts, at, prev = [], {}, 0, 0
    for j, run in enumerate(RUNS):
        b = b"ACGT"[j % 4]
        parts += [stretch(9, prev, b), np.full(run, b, dtype=np.uint8)]
        starts[run] = at + 9
        at += 9 + run
        prev = b
    parts.append(stretch(12, prev, 0))
    return np.concatenate(parts), starts


def homopolymers(H):
    """runs of 1, 2, 3, 8, 9 and 300 bases (homop is 16 bits wide) with gains of H homopolymer lengths that differ per length:
    a substitution inside every run whose reads 6 and 7 carry 1.9 and 3.0 -- kept or zeroed by min_req = half the gain of length
    min(h, H) (1.5, 2.0, 3.25 for H = 1, 3, 8 in the long runs), so the count and the score show the clamp of gains_expected and
    of the p-value index; insertions of another base and deletions at run lengths 2 (kept) and 3 (dropped); an insertion of a
    base next to itself on either side: kept in a run-free stretch (1 + 1), dropped behind a run of two (2 + 1)"""
    tmpl, starts = _run_template()
    code = lambda q: b"ACGT".index(bytes([int(tmpl[q])]))   # noqa: E731
    six, seven = [0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5, 6]   # (seven carriers where the p-value of an insertion or deletion needs them)
    plants = []
    for run in RUNS:
        mid = starts[run] + run // 2
        plants.append((mid, (code(mid) + 1) % 4, np.array([HI] * 6 + [1.9, 3.0] + [-HI] * 4)))   # a substitution inside the run
    for run in (2, 3):
        s = starts[run]
        plants.append((s + 1, 4 + (code(s) + 2) % 4, seven))             # Ins of another base inside the run
        plants.append((s, DEL1, seven))                                  # Del of a base of the run
    s2 = starts[2]
    plants.append((s2 + 2, 4 + code(s2), seven))                         # Ins of the run's base behind the run of two: 2 + 1
    s9 = starts[9]
    plants.append((s9 - 4, 4 + code(s9 - 5), seven))                     # Ins of the base in front of it: 1 + 1
    plants.append((s9 - 6, 4 + code(s9 - 6), seven, 6.5))                # Ins of the base behind it: 1 + 1
    s300 = starts[300]
    plants.append((s300 + 299, (code(s300) + 2) % 4, six, 6.25))       # the run's last base
    return case("table", [table_chunk(tmpl, 12, 2, plants)], gains=gains_of(H))


def copy_numbers():
    """copy number 1 (every cand -1, dim 0), 2, 3 and 7 in one call, with other n and L beside them; haploid coverage 2 and a
    count of 6: the Poisson maximum over k = 1 .. copy_num falls on k = 3, an inner k of the chunk of copy number 7"""
    six12 = [0, 1, 2, 3, 4, 5]
    return case("table", [table_chunk(plain_template(40), 8, 1, [(10, 1, SIX_OF_8), (25, 2, SIX_OF_8)]),
                          table_chunk(plain_template(50, 1), 8, 2, [(10, 1, SIX_OF_8), (25, 2, SIX_OF_8)]),
                          table_chunk(plain_template(60, 2), 12, 3, [(10, 1, six12), (25, 2, [0, 1, 2, 3, 4, 5, 6, 7]), (40, 3, [4, 5, 6, 7, 8, 9])]),
                          table_chunk(plain_template(70, 3), 20, 7, [(10, 1, six12), (25, 2, [6, 7, 8, 9, 10, 11, 12]), (40, 3, [13, 14, 15, 16, 17, 18, 19, 0]),
                                                                     (55, 0, [2, 3, 9, 10, 15, 16])])],
                coverage=2.0)


# pick_many: 24 reads, copy number 4 (four picks per round, three rounds).  Candidate i of the list sits at bp 10 + 7 i for
# i <= 70, the 6-bp neighbour is candidate 71 and the later grid positions follow.
PM_N, PM_L = 24, 520
PM_A = [0, 3, 6, 9, 12, 15, 18, 21]          # carriers of the three tied columns
PM_B = [1, 4, 7, 10, 13, 16, 19, 22]
PM_C = [2, 5, 8, 11, 14, 17, 20, 23]
PM_TIED = (5, 40, 70)                        # lanes 5, 40 and 6; strides 0, 0 and 1
PM_P2, PM_Q80, PM_Q56, PM_QCOS = 20, 24, 28, 32


def _pm_bp(i):
    return 10 + 7 * i


def pick_many():
    """74 candidates, so every loop of pick_body strides twice.  Three columns of equal score bits at list indices 5, 40 and 70 (the
    highest score): the last is picked first, the others are flagged 3 by it and picked first in rounds 2 and 3.  Candidate 71 is 6
    bp behind that pick (masked for good), candidate 72 is 7 bp behind it (not masked: the second pick).  P2 (list index 20) is
    non-zero in reads 0 .. 12 only; Q80 shares five of them and agrees in four (Sokal-Michener exactly 0.8, cosine 0.6: picked
    right after P2), Q56 shares six and agrees in five (flagged), QCOS shares five, agrees in four and has cosine 0.858 (flagged)."""
    n = PM_N
    tmpl = plain_template(PM_L)
    generic = [PM_B, PM_C, [0, 1, 2, 3, 12, 13, 14, 15], [4, 5, 6, 7, 16, 17, 18, 19], [8, 9, 10, 11, 20, 21, 22, 23]]
    plants = []
    for i in range(73):
        bp = _pm_bp(i)
        row = i % 4
        if i in PM_TIED:
            plants.append((bp, row, PM_A, 9.0))
        elif i == 71:
            plants.append((bp, row, PM_B, 8.5))            # 7 bp behind the first pick
        elif i == PM_P2:
            plants.append((bp, row, np.array([8.0] * 8 + [-HI] * 5 + [BG] * 11)))
        elif i == PM_Q80:    # reads 8 .. 23; of 8 .. 12 it agrees with P2 (negative there) in four
            plants.append((bp, row, np.array([BG] * 8 + [-HI, -HI, -HI, -HI, 7.5] + [7.5, -HI, 7.5, -HI, 7.5, 7.5, -HI, 7.5, -HI, 7.5, 7.5])))
        elif i == PM_Q56:    # reads 7 .. 23; of 7 .. 12 it agrees with P2 in five
            plants.append((bp, row, np.array([BG] * 7 + [7.25, -HI, -HI, -HI, -HI, 7.25] + [7.25, -HI, 7.25, -HI, 7.25, 7.25, -HI, 7.25, -HI, 7.25, -HI])))
        elif i == PM_QCOS:   # reads 8 .. 23: four large agreements and one small disagreement with P2
            plants.append((bp, row, np.array([BG] * 8 + [-20.0, -20.0, -20.0, -20.0, 3.0] + [7.0, -HI, 7.0, -HI, 7.0, 7.0, -HI, 7.0, -HI, 7.0, 7.0])))
        else:
            plants.append((bp, row, generic[i % 5], 6.0 + i / 64.0))
        if i == 70:
            plants.append((bp + 6, 1, PM_C, 8.75))         # candidate 71: 6 bp behind the first pick
    return case("table", [table_chunk(tmpl, n, 4, plants)])


def _spread_sets(n, size, count, seed):
    """`count` carrier sets of `size` reads out of n that share at most 3 reads pairwise and hold as many even as odd reads"""
    rng = np.random.default_rng(seed)
    sets = []
    while len(sets) < count:
        s = sorted(int(x) for x in np.concatenate([2 * rng.choice(n // 2, size // 2, replace=False), 2 * rng.choice(n // 2, size // 2, replace=False) + 1]))
        if all(len(set(s) & set(t)) <= 3 for t in sets):
            sets.append(s)
    return sets


def pick_cap():
    """copy number 7, 48 reads: 23 mutually dissimilar candidates, so that three rounds of seven picks fill all JTK_MAX_DIM = 21
    columns; a second chunk with five candidates, where the first round takes all and the others end at once; a third whose four
    candidates are one column four times: one pick per round, dim 3"""
    n = 48
    sets = _spread_sets(n, 10, 23, 20241)
    full = table_chunk(plain_template(180), n, 7, [(8 + 7 * j, j % 4, sets[j], 6.0 + j / 32.0) for j in range(23)])
    few = table_chunk(plain_template(60, 1), n, 7, [(8 + 9 * j, (j + 1) % 4, sets[j], 6.0 + j / 32.0) for j in range(5)])
    same = table_chunk(plain_template(60, 2), n, 7, [(8 + 9 * j, (j + 2) % 4, sets[0], 6.0 + j / 32.0) for j in range(4)])
    return case("table", [full, few, same], coverage=2.0)


# ---------------------------------------------------------------------------------------------------------------------------
# row sums
# ---------------------------------------------------------------------------------------------------------------------------
REVERSE_EMIT = [0.94 if r == q else 0.02 for r in range(4) for q in range(4)]   # the forward model's is 0.97 / 0.01


def fma(a, b, c):
    """a * b + c rounded once (this Python has no math.fma): exact rationals; the two cases that need none are taken first"""
    a, b, c = float(a), float(b), float(c)
    if c == 0.0 or a == 0.0 or b == 0.0:
        return a * b + c   # one of the two operations is exact
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _entry(v, G, lk, log):
    return ((log(v) + float(G) * LN2) if v > 0.0 else LOG_ZERO) - lk


def read_table(rows, exps, lk, emit, L, log):
    """one read's 14 (L + 1) entries, minus lk, from its row sums ("Row sums")"""
    out = np.full((L + 1, NUM_ROW), LOG_ZERO - (lk if lk > LOG_ZERO else 0.0))
    if not lk > LOG_ZERO:   # a dead read
        return out.ravel()

    def mixed(a, first, G):
        res = []
        for b in range(4):
            v = emit[4 * b] * float(a[first])
            for c in (1, 2, 3):
                v = fma(emit[4 * b + c], a[first + c], v)
            res.append(_entry(v + float(a[first + 4]), G, lk, log))
        return res

    for p in range(L + 1):
        if p + 1 <= L:
            out[p, 0:4] = mixed(rows[p + 1], 0, exps[p + 1])
            out[p, 8:11] = [_entry(float(rows[p + 1][10 + c]), exps[p + 1], lk, log) for c in range(3)]
        out[p, 4:8] = mixed(rows[p], 5, exps[p])
        for d in (1, 2, 3):
            if p + d + 1 <= L:
                out[p, 10 + d] = _entry(float(rows[p + d + 1][12 + d]), exps[p + d + 1], lk, log)
    return out.ravel()


def table_from_row_sums(chunk, forward_emit, reverse_emit, log):
    """[n, 14 (L + 1)]: the table (minus lk) of every read of a row-sum chunk; reads of equal bytes are evaluated once"""
    L = len(chunk["tmpl"])
    rows, exps, lk = chunk["rows"], chunk["exps"], chunk["lk"]
    out = np.empty((len(lk), NUM_ROW * (L + 1)))
    seen = {}
    for r in range(len(lk)):
        key = (bool(chunk["strands"][r]), float(lk[r]), rows[r].tobytes(), exps[r].tobytes())
        if key not in seen:
            seen[key] = read_table(rows[r], exps[r], float(lk[r]), forward_emit if chunk["strands"][r] else reverse_emit, L, log)
        out[r] = seen[key]
    return out


def _p2(mantissa, e):
    return float(np.ldexp(mantissa, int(e)))


# levels of log(V) + G ln 2 - lk for lk = -44: 1.75 x 2^-55 is about +6.4 (times the emission of the planted base), 1.25 x 2^-72
# about -5.7, 2^-66 about -1.75 (zero after compression)
def _row_sum_read(L, G, planted, zero_row=None, salt=0):
    """one read's rows: `planted` = [(p, row, the read carries the gain)]; the mantissa of a gain runs with the row and `salt`"""
    rows = np.zeros((L + 1, ACC_N))
    for q in range(L + 1):
        bg = _p2(1.0, -66 - int(G[q]))
        rows[q, 4] = rows[q, 9] = bg
        rows[q, 10:16] = bg
    for p, row, carries in planted:
        q = p + 1 if row < 4 else (p if row < 8 else p + 2)
        hi, lo = _p2(1.5 + ((7 * q + 3 * salt) % 16) / 64.0, -55 - int(G[q])), _p2(1.25, -72 - int(G[q]))
        if row < 4:      # a substitution: the sums over the read bases at [0 .. 3], the rest at [4]
            rows[q, 4] = lo
            rows[q, row] = hi if carries else 0.0
        elif row < 8:    # an insertion: [5 .. 8] and [9]
            rows[q, 9] = lo
            rows[q, 5 + row - 4] = hi if carries else 0.0
        else:
            assert row == DEL1
            rows[q, 13] = hi if carries else lo
    if zero_row is not None:
        rows[zero_row, :] = 0.0
    return rows


ROWS_LENGTHS = (127, 128, 129, 255, 256, 260)
ROWS_ZERO_ROW = 126      # read 3 has no sum in this row: the substitutions at 125, the insertions at 126, the deletion at 124


def _rows_chunk(L, shift, n=6, dead=5):
    tmpl = plain_template(L, shift)
    last = L + 1 - MASK_LENGTH
    planted = [(p, (p + shift) % 4) for p in list(range(120, 135)) + list(range(250, 261)) if p <= last]
    planted += [(L - 6, DEL1)]
    if L >= 140:
        planted += [(140, 4 + other_base(tmpl, 140)), (127, DEL1)]   # the deletion at 127 reads row 129, beyond its tile
    planted = sorted(set(planted))
    # exponents: negative, zero, small and large, another one per row
    G = np.array([(-40, 0, 7, 300, -3, 0, 64)[(q + shift) % 7] for q in range(L + 1)], dtype=np.int32)
    rows = np.stack([_row_sum_read(L, G, [(p, row, r != dead) for p, row in planted], ROWS_ZERO_ROW if r == 3 else None, salt=r) for r in range(n)])
    lk = np.array([LOG_ZERO if r == dead else -44.0 - r / 16.0 for r in range(n)])
    return dict(tmpl=tmpl, strands=alternating(n), copy_num=2, rows=rows, exps=np.tile(G, (n, 1)), lk=lk,
                planted=[p * NUM_ROW + row for p, row in planted])


def rows_tile_edges():
    """six chunks in one call; candidates at 120 .. 134 and 250 .. 260 where they are inside the template (position 127 reads rows
    128 .. 131, beyond its tile's own 128; so do 255 and 383), a deletion column at L - 6, an insertion column at 140; read 5 of
    every chunk is dead (lk = LOG_ZERO: every entry -1e300, the one negative of every column), read 3 has a row without sums
    (LOG_ZERO - lk), the exponents run through -40, 0, 7, 300, -3, 0, 64; the reverse model's emissions differ from the forward's"""
    return case("rows", [_rows_chunk(L, j) for j, L in enumerate(ROWS_LENGTHS)], reverse_emit=REVERSE_EMIT)


DEEP_N = 65535


def rows_deep():
    """the fused filter's 16-bit fields at their limit: one chunk of 65,535 reads on 14 bp (two live positions).  Column (7, sub):
    65,534 reads positive, split over both strands, and the last one negative -- count 65,534, strand x sign products of
    32,767 x 65,534; column (8, sub): 32,768 positive and 32,767 negative, alternating.  Haploid coverage 30,000, so that both are
    candidates."""
    L, n = 14, DEEP_N
    tmpl = plain_template(L, 1)
    G = np.array([(0, 5, -2)[q % 3] for q in range(L + 1)], dtype=np.int32)
    c0, c1 = (7, 1), (8, 2)
    kinds = {(a, b): _row_sum_read(L, G, [c0 + (a,), c1 + (b,)]) for a in (False, True) for b in (False, True)}
    r = np.arange(n)
    first, second = r != n - 1, r % 4 < 2        # column c0: all but the last read; c1: 32,768 reads, half of them on each strand
    assert int(second.sum()) == 32768 and int(first.sum()) == 65534
    rows = np.empty((n, L + 1, ACC_N))
    for (a, b), kind in kinds.items():
        rows[(first == a) & (second == b)] = kind
    return case("rows", [dict(tmpl=tmpl, strands=alternating(n), copy_num=2, rows=rows, exps=np.tile(G, (n, 1)), lk=np.full(n, -44.0),
                              planted=[c0[0] * NUM_ROW + c0[1], c1[0] * NUM_ROW + c1[1]])], coverage=30000.0, reverse_emit=REVERSE_EMIT)


TABLE_CASES = dict(planted_60=planted_60, tile_edges=tile_edges, short_templates=short_templates, thresholds=thresholds,
                   thresholds_pos_thr=thresholds_pos_thr, strand_and_sign=strand_and_sign, homopolymers_h1=lambda: homopolymers(1),
                   homopolymers_h3=lambda: homopolymers(3), homopolymers_h8=lambda: homopolymers(8), copy_numbers=copy_numbers,
                   pick_many=pick_many, pick_cap=pick_cap)
ROW_CASES = dict(rows_tile_edges=rows_tile_edges, rows_deep=rows_deep)
CASES = dict(TABLE_CASES, **ROW_CASES)


def input_sha256(cs):
    """of everything a call is given"""
    h = hashlib.sha256()
    h.update(repr((cs["mode"], cs["coverage"], cs["gains"], cs["reverse_emit"])).encode())
    for ch in cs["chunks"]:
        h.update(np.asarray(ch["tmpl"], dtype=np.uint8).tobytes())
        h.update(np.asarray(ch["strands"], dtype=np.uint8).tobytes())
        h.update(repr(ch["copy_num"]).encode())
        for key in ("table", "rows", "exps", "lk"):
            if key in ch:
                h.update(np.ascontiguousarray(ch[key]).tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------------------------------------
# the reference's record of a case (tests/clustering_reference.py; B: its exp / ln back end)
# ---------------------------------------------------------------------------------------------------------------------------
def params_of(cs):
    """jtk_lc_params_t of a case (the forward model is the default one)"""
    from jtk_amd import batch as jb
    p = jb.default_params(cs["coverage"], gains=cs["gains"])
    if cs["reverse_emit"] is not None:
        for k, v in enumerate(cs["reverse_emit"]):
            p.reverse.mat_emit[k] = v
    return p


def tables_of(cs, log):
    """every chunk's [n, 14 (L + 1)] table minus lk"""
    if cs["mode"] == "table":
        return [ch["table"] for ch in cs["chunks"]]
    p = params_of(cs)
    fwd, rev = [float(x) for x in p.forward.mat_emit], [float(x) for x in p.reverse.mat_emit]
    return [table_from_row_sums(ch, fwd, rev, log) for ch in cs["chunks"]]


def bits(x):
    return [int(b) for b in np.asarray(x, dtype=np.float64).ravel().view(np.uint64)]


def reference(cs, B, tables=None):
    """per chunk what the filter stage must leave: cand (the whole array: -1 or the score), cands [(pos, score, count)], dropped,
    order (the picked candidates' list indices in pick order), probes (the picked columns in column order), vtype, feat [n, dim],
    comp (the compressed profiles)"""
    import clustering_reference as R
    gains = R.Gains.from_params(params_of(cs))
    out = []
    for ch, prof in zip(cs["chunks"], tables_of(cs, B.log) if tables is None else tables):
        tmpl, n = ch["tmpl"], len(ch["strands"])
        cand = np.full(prof.shape[1], -1.0)
        if ch["copy_num"] < 2:   # clustering() returns before search_variants (pseudo_mcmc.rs:86-88)
            out.append(dict(cand=cand, cands=[], dropped={}, order=[], probes=[], vtype=[], feat=np.zeros((n, 0)), comp=None))
            continue
        comp = R.compress_small_gains(prof, tmpl, gains)
        cands, dropped = R.filter_candidates(comp, tmpl, ch["strands"], gains, ch["copy_num"], cs["coverage"], B)
        order = []
        probes = [pos for pos, _ in R.pick_filtered_profiles(cands, comp, ch["copy_num"], order=order)]
        homop = R.homopolymer_lengths(tmpl)
        vtype = [[int(homop[pos // NUM_ROW]) if pos // NUM_ROW < len(tmpl) else 0, R.diff_type_of(pos % NUM_ROW)] for pos in probes]
        for pos, lk, _ in cands:
            cand[pos] = lk
        out.append(dict(cand=cand, cands=cands, dropped=dropped, order=order, probes=probes, vtype=vtype, feat=comp[:, probes].copy(), comp=comp))
    return out


FEAT_INLINE = 600   # feature matrices of up to this many entries are stored as bits, larger ones as the SHA-256 of their bytes


def as_record(ref):
    """a chunk's reference output as the golden file holds it"""
    feat = np.ascontiguousarray(ref["feat"], dtype=np.float64)
    return dict(cands=[[int(pos), "%016x" % bits([lk])[0], int(count)] for pos, lk, count in ref["cands"]],
                dropped={str(pos): why for pos, why in sorted(ref["dropped"].items())}, order=[int(i) for i in ref["order"]],
                probes=[int(pos) for pos in ref["probes"]], vtype=[[int(h), int(dt)] for h, dt in ref["vtype"]],
                feat_shape=list(feat.shape), feat=["%016x" % b for b in bits(feat)] if feat.size <= FEAT_INLINE else None,
                feat_sha256=hashlib.sha256(feat.tobytes()).hexdigest(), cand_sha256=hashlib.sha256(np.ascontiguousarray(ref["cand"]).tobytes()).hexdigest())
