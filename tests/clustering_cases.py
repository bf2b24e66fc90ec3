"""The feature-level problems of tests/test_clustering_reference.py and tests/test_gpu_clustering_reference.py: small read
counts (the Python chain of tests/clustering_reference.py makes 2000 n proposals per restart, 20 restarts per tried cluster count),
every case built for a branch of pseudo_mcmc.rs:213-408, 649-869 / misc.rs:231-341 and listed with the predicate on the
reference's own log that shows the branch was entered (REACHES).  The device's dispatch decides the shapes: every case of CASES
has n <= 63 reads, so the diploid ones run mcmc_chain_k2<D, 1> with D = the column count (1, 2, 3, 4, 5-8), copy numbers 3 and 4 run
mcmc_chain_tab<3> / <4>, and diploid_nine_columns runs mcmc_chain_tab<2> (D > 8).  LARGE_CASES (64 to 256 reads) are the
smallest shapes of every other path of that dispatch short of mcmc_kernel_huge and the recursive split.

A case is dict(x = n x dim matrix, vt = dim x (homopolymer length, diff type), copy_num, coverage (haploid), local_coverage,
chunk_id).  Values are drawn once from numpy's PCG64 with fixed seeds and rounded to 1/64, so a case is the same on every machine.
"""
import os

import numpy as np

POS_THR = 0.00001
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clustering_reference.json")


def _clean(seed, labels, owners, hi=4.5, lo=-4.5, spread=0.5):
    """+hi where the read's cluster owns the column, lo elsewhere, plus noise; multiples of 1/64"""
    rng = np.random.default_rng(seed)
    labels, owners = np.asarray(labels), np.asarray(owners)
    x = np.where(labels[:, None] == owners[None, :], hi, lo) + rng.uniform(-spread, spread, (len(labels), len(owners)))
    return np.round(x * 64) / 64


def _vt(dim, homop=1, dt=0):
    return np.array([[homop, dt]] * dim, dtype=np.uint32).reshape(dim, 2)


def _case(x, copy_num, chunk_id, vt=None, coverage=4.0, local_coverage=None):
    x = np.asarray(x, dtype=np.float64).reshape(len(x), -1)
    n, dim = x.shape
    return dict(x=x, vt=_vt(dim) if vt is None else np.asarray(vt, dtype=np.uint32).reshape(dim, 2), copy_num=copy_num,
                coverage=float(coverage), local_coverage=float(n / copy_num if local_coverage is None else local_coverage),
                chunk_id=chunk_id)


def _diploid(dim, seed, n=8):
    labels = [0, 1] * (n // 2)
    return _case(_clean(seed, labels, [d % 2 for d in range(dim)]), 2, 100 + dim)


def _with(case, **kw):
    out = dict(case)
    out.update(kw)
    return out


def _poke(case, value, row=3, col=0):
    x = case["x"].copy()
    x[row, col] = value
    return _with(case, x=x)


def _tie_local_coverage(score, homop=1, dt="subst"):
    """the local coverage at which expected_gains(..) * local_coverage + 0.1 (pseudo_mcmc.rs:253-255) is EXACTLY `score` in
    doubles, for a column of the default gains: searched ulp by ulp around (score - 0.1) / (0.8 gain)"""
    import math
    from jtk_amd import batch as jb
    per_read = max(0.8 * jb.DEFAULT_GAINS[dt][homop - 1][0], 0.1)
    for start, to in (((score - 0.1) / per_read, math.inf), ((score - 0.1) / per_read, -math.inf)):
        x = start
        for _ in range(4096):
            if per_read * x + 0.1 == score:
                return x
            x = math.nextafter(x, to)
    raise AssertionError("no local coverage gives an exact tie")


def weak(seed, n=8, dim=2, amp=0.4):
    rng = np.random.default_rng(seed)
    return np.round(rng.uniform(-amp, amp, (n, dim)) * 64) / 64


CASES = {
    # copy number 2, D = 1, 2, 3, 4 and 5-8: one mcmc_chain_k2<D, 1> instantiation each
    "diploid_1_column": lambda: _diploid(1, 11),
    "diploid_2_columns": lambda: _diploid(2, 12),
    "diploid_3_columns": lambda: _diploid(3, 13),
    "diploid_4_columns": lambda: _diploid(4, 14),
    "diploid_6_columns": lambda: _diploid(6, 15),
    "diploid_nine_columns": lambda: _diploid(9, 16, n=6),
    # copy numbers 3 and 4 with as many true clusters: k = 2, 3 (, 4) tried and accepted
    "three_copies": lambda: _case(_clean(21, [0, 1, 2] * 3, [0, 1, 2]), 3, 203, coverage=3.0, local_coverage=1.0),
    "four_copies": lambda: _case(_clean(22, [0, 1, 2, 3] * 2 + [0], [0, 1, 2, 3]), 4, 204, coverage=2.0, local_coverage=0.5),
    # two true clusters under copy number 3: k = 2 accepted, the stop rule breaks at k = 3 with no newly used column
    "two_of_three_copies": lambda: _case(_clean(23, [0, 1] * 4, [0, 1]), 3, 205),
    # 1 + 2 dim < copy_num: RANGE ends at 3, not at 4
    "one_column_four_copies": lambda: _case(_clean(24, [0, 1] * 3, [1]), 4, 206, coverage=1.5),
    # nothing to find: the k = 2 alternative beats the chain and the stop rule breaks at the first k
    "noise_only": lambda: _case(weak(31), 2, 301),
    # weak columns and a flat size prior: most proposals are taken
    "weak_columns": lambda: _case(weak(32, amp=0.2), 2, 302, coverage=4.0),
    # all-zero rows: their moves change the sizes only, equal sizes swap with diff == 0 and gen_bool(1.0) draws nothing
    "zero_rows": lambda: _case(np.vstack([_clean(33, [0, 1] * 3, [0, 1]), np.zeros((3, 2))]), 2, 303, coverage=4.5),
    # one strong column and a second one across it: the chain beats the k = 2 alternative, and the tail moves reads
    "one_strong_column": lambda: _case(np.hstack([_clean(34, [0, 1] * 4, [1], hi=6.0, lo=-0.25, spread=0.1),
                                                  _clean(35, [0, 1, 1, 0] * 2, [0], hi=1.0, lo=-1.0, spread=0.2)]), 2, 304,
                                       coverage=1.0),
    # a read with evidence of 0.0005 / 0.0002 that the chain's size prior misplaces: the k = 2 alternative wins by 0.0003 and is accepted
    "highest_gain_accepted": lambda: _case(np.vstack([_clean(36, [0] * 5 + [1] * 4, [0, 1]), [[0.0005, 0.0002]]]), 2, 305,
                                              coverage=5.0),
    # the stop rule on an exact tie: the local coverage is chosen so that the expected gain IS the k = 2 score (34.875, a sum of
    # multiples of 1/64 after the size terms cancel): `expected_gain < score - max` is false, the chunk stays one cluster
    "stop_rule_exact_tie": lambda: _with(_diploid(2, 12), local_coverage=_tie_local_coverage(34.875), chunk_id=307),
    # k = 3 uses the columns k = 2 used and gains 1.0 by setting one read apart (a haploid coverage of 1 makes a cluster of one
    # cheap): more than 0.1 local + 0.1 = 0.15, which is what the expected gain would be without the no_new_variants branch,
    # less than 0.8 gain local + 0.1 = 1.93
    "no_new_variants_decides": lambda: _case(np.vstack([_clean(23, [0, 1] * 4, [0, 1]), [[-1.0, -4.5]]]), 3, 308, coverage=1.0,
                                             local_coverage=0.5),
    # the chain wins (the alternative splits on column 0 alone and misplaces the read [-0.25, -4.5]) and its size prior holds the
    # read [0.0005, 0.0002] where its own evidence is 0.0003 worse: less than the tail's 0.001, the label stays
    "tail_margin_keeps_a_read": lambda: _case(np.vstack([_clean(36, [0] * 5 + [1] * 4, [0, 1]), [[-0.25, -4.5]], [[0.0005, 0.0002]]]), 2,
                                              309, coverage=5.0),
    # every value negative: no column is ever used, min_gain falls back to 1
    "no_used_column": lambda: _case(-np.abs(weak(37)) - 0.25, 2, 306),
    # early returns
    "as_many_reads_as_copies": lambda: _case(_clean(41, [0, 1], [0, 1]), 2, 401),
    "no_column": lambda: _case(np.zeros((5, 0)), 2, 402),
    "copy_number_one": lambda: _case(_clean(42, [0, 1] * 3, [0, 1]), 1, 403),
    # duplicate rows: zero weights in suggest_first; with fewer distinct rows than k every weight is zero (a panic)
    "duplicate_rows": lambda: _case(np.array([[4.5, -4.5], [-4.5, 4.5]] * 4), 2, 501),
    "fewer_distinct_rows_than_k": lambda: _case(np.array([[4.5, -4.5], [-4.5, 4.5]] * 4), 3, 502, local_coverage=1.0),
    # LKCount's zero band, NaN
    "value_plus_pos_thr": lambda: _poke(_diploid(2, 12), POS_THR),
    "value_minus_pos_thr": lambda: _poke(_diploid(2, 12), -POS_THR),
    "value_just_inside_the_band": lambda: _poke(_diploid(2, 12), 0.99 * POS_THR),
    "value_nan": lambda: _poke(_diploid(2, 12), float("nan")),
    "coverage_nan": lambda: _with(_diploid(2, 12), coverage=float("nan")),
    "coverage_zero": lambda: _with(_diploid(2, 12), coverage=0.0),
    "coverage_negative": lambda: _with(_diploid(2, 12), coverage=-3.0),
}

PANICS = ("fewer_distinct_rows_than_k", "value_plus_pos_thr", "value_minus_pos_thr", "value_nan", "coverage_nan", "coverage_zero",
          "coverage_negative")


# case -> predicate on the reference's log (clustering_reference.Log): the branch the case was built for was entered
REACHES = {
    "diploid_1_column": lambda g: g.range == (2, 2) and g.tried[0]["accepted"],
    "diploid_2_columns": lambda g: g.range == (2, 2) and g.tried[0]["accepted"] and all(g.tried[0]["newly_used"]),
    "diploid_3_columns": lambda g: g.tried[0]["accepted"],
    "diploid_4_columns": lambda g: g.tried[0]["accepted"],
    "diploid_6_columns": lambda g: g.tried[0]["accepted"],
    "diploid_nine_columns": lambda g: g.tried[0]["accepted"],
    "three_copies": lambda g: g.range == (2, 3) and [t["accepted"] for t in g.tried] == [True, True] and any(g.tried[1]["newly_used"]),
    "four_copies": lambda g: g.range == (2, 4) and [t["accepted"] for t in g.tried] == [True, True, True],
    "two_of_three_copies": lambda g: [t["accepted"] for t in g.tried] == [True, False] and g.tried[1]["no_new_variants"],
    "one_column_four_copies": lambda g: g.range == (2, 3),
    "noise_only": lambda g: [t["accepted"] for t in g.tried] == [False] and g.tried[0]["source"] == "highest_gain"
    and g.tried[0]["chain_score"] < g.tried[0]["highest_gain_score"],
    "stop_rule_exact_tie": lambda g: len(g.tried) == 1 and not g.tried[0]["accepted"] and g.tried[0]["expected_gain"] == g.tried[0]["score"],
    "no_new_variants_decides": lambda g: [t["accepted"] for t in g.tried] == [True, False] and g.tried[1]["no_new_variants"]
    and 0.1 * 0.5 + 0.1 < g.tried[1]["score"] - g.tried[0]["score"] < g.tried[1]["expected_gain"],
    "tail_margin_keeps_a_read": lambda g: g.tried[0]["source"] == "chain" and g.tail["within_margin"] > 0 and g.tail["changed"] == 0,
    "no_used_column": lambda g: not any(g.tried[0]["used_columns"]) and g.tried[0]["min_gain"] == 1.0 and not g.tried[0]["accepted"],
    "weak_columns": lambda g: g.chain["downhill_taken"] + g.chain["zero_diff"] + g.chain["uphill"] > 0.5 * g.chain["proposals"],
    "zero_rows": lambda g: g.chain["zero_diff"] > 0,
    "one_strong_column": lambda g: g.tried[0]["source"] == "chain" and g.tried[0]["chain_score"] > g.tried[0]["highest_gain_score"]
    and g.tail["changed"] > 0,
    "highest_gain_accepted": lambda g: g.tried[0]["source"] == "highest_gain" and g.tried[0]["accepted"],
    "as_many_reads_as_copies": lambda g: g.early_return,
    "no_column": lambda g: g.early_return,
    "copy_number_one": lambda g: g.early_return,
    "duplicate_rows": lambda g: g.kmeans["zero_weights"] > 0,
    "value_just_inside_the_band": lambda g: g.tried[0]["accepted"],
}

# across the cases (any one of them): the branches no single case is named for
REACHED_SOMEWHERE = {
    "the chain wins over highest_gain at k = 2": lambda g: any(t["k"] == 2 and t["source"] == "chain" and t["chain_score"] > t["highest_gain_score"]
                                                              for t in g.tried),
    "a chain whose best state is not its last": lambda g: g.chain["best_not_last"] > 0,
    "a cluster that empties": lambda g: g.chain["emptied"] > 0,
    "the last of several equal restarts is kept": lambda g: any(t["restarts"] and t["source"] == "chain" and t["restarts"]["distinct_at_max"] > 1
                                                               for t in g.tried),
    "equal restarts with different labels, the first not the last": lambda g: any(
        t["restarts"] and t["source"] == "chain" and t["accepted"] and t["restarts"]["first_max_differs"] for t in g.tried),
    "the random start of kmeans": lambda g: g.kmeans["random_start"] > 0,
    "the seeded start of kmeans": lambda g: g.kmeans["seeded_start"] > 0,
}


# ---------------------------------------------------------------------------------------------------------------------------
# 64 reads and more: the device paths no case above reaches.  The dispatch (chain_split_kernel, mcmc_chain_dispatch):
#   copy 2, n <= 127, D <= 2          mcmc_kernel_light, mcmc_chain_k2<1, 2> (D == 1) / <2, 2> (D == 2): two table registers,
#                                     read and size indices 64 r + lane
#   copy 2, n <= 127, 3 <= D <= 8     mcmc_kernel, mcmc_chain_k2<4, 2> (D = 3 AND 4) / <8, 2> (D = 5 .. 8)
#   copy 2, n >= 128 or D >= 9        mcmc_kernel, mcmc_chain_tab<2> with SMALL false (n >= 64); its tables leave the registers
#   copy 3, 4                         mcmc_chain_tab<3> / <4>, SMALL false                   for LDS beyond 255 reads (big)
# The haploid coverage is about n / copy_num (the size prior of a real pile-up) and shared within a group, since it is a
# parameter of the device call: 32 (n = 64 .. 70), 40 (n = 80 .. 88), 60 (n = 120 .. 128), 20 (copies 3 and 4), 128 (n = 255, 256).
# Moving a read out of its cluster costs D amp (amp where it leaves, amp where it lands), so the columns of D >= 2 have an
# amplitude of 7 / D: about one proposal in a thousand is taken and reversed, among them reads of index >= 64, while the
# clusters stay the true ones (n D amp / 2 = 3.5 n is above the expected gain of 0.8 * 4.56 n / 2).
# ---------------------------------------------------------------------------------------------------------------------------
def _large_diploid(n, dim, seed, chunk_id, coverage, first=None):
    """two clusters taking turns over the first 2 * min(first, n - first) reads, the rest of cluster 0 (`first` = its size)"""
    first = (n + 1) // 2 if first is None else first
    turns = 2 * min(first, n - first)
    labels = [r % 2 for r in range(turns)] + [0 if first > n - first else 1] * (n - turns)
    assert labels.count(0) == first
    amp = 4.5 if dim == 1 else 7.0 / dim
    return _case(_clean(seed, labels, [d % 2 for d in range(dim)], hi=amp, lo=-amp, spread=amp / 4), 2, chunk_id, coverage=coverage)


def _copies(n, copy_num, seed, chunk_id, coverage):
    """as many true clusters as copies, one column each: +4.5 in its own reads, -2.5 elsewhere (a move costs 7, a new cluster
    gains 4.5 per read, above the 0.8 * 4.56 expected)"""
    labels = [r % copy_num for r in range(n)]
    return _case(_clean(seed, labels, list(range(copy_num)), hi=4.5, lo=-2.5), copy_num, chunk_id, coverage=coverage)


LARGE_CASES = {
    # mcmc_kernel_light, mcmc_chain_k2<1, 2>: read 64 is the first in the second table register
    "light_64_reads_1_column": lambda: _large_diploid(64, 1, 601, 601, 32.0),
    # mcmc_kernel_light, <2, 2>: both ends of its range
    "light_65_reads_2_columns": lambda: _large_diploid(65, 2, 602, 602, 32.0),
    "light_127_reads_2_columns": lambda: _large_diploid(127, 2, 603, 603, 60.0),
    # mcmc_kernel, <4, 2> by D = 3 and by D = 4 (one instantiation, unlike <3, 1> and <4, 1>), <8, 2> by D = 6 and D = 8
    "k2_64_reads_3_columns": lambda: _large_diploid(64, 3, 604, 604, 32.0),
    "k2_88_reads_4_columns": lambda: _large_diploid(88, 4, 605, 605, 40.0),
    "k2_80_reads_6_columns": lambda: _large_diploid(80, 6, 606, 606, 40.0),
    "k2_127_reads_8_columns": lambda: _large_diploid(127, 8, 607, 607, 60.0),
    # the headline read count, <4, 2>: a cluster of 70 reads, whose size prior is read from the size table's second register
    "k2_120_reads_70_and_50": lambda: _large_diploid(120, 3, 608, 608, 60.0, first=70),
    # <2, 2>, weak columns: most proposals are taken, so the walk over certainly-rejected proposals keeps restarting and the
    # per-read flipped likelihoods are rebuilt after every move
    "light_80_reads_weak_columns": lambda: _case(weak(609, n=80, dim=2, amp=0.2), 2, 609, coverage=40.0),
    # <2, 2>, 13 all-zero rows at 68 .. 80: their moves change the sizes only; 41 against 40 (n is odd for that) a move swaps
    # the sizes, diff == 0 and gen_bool(1.0) draws nothing
    "light_81_reads_zero_rows": lambda: _case(np.vstack([_large_diploid(68, 2, 610, 0, 0.0)["x"], np.zeros((13, 2))]), 2, 610,
                                              coverage=40.0),
    # mcmc_chain_tab<2>, SMALL false: by the first n past the diploid chain, and by the column count
    "tab2_128_reads_3_columns": lambda: _large_diploid(128, 3, 611, 611, 60.0),
    "tab2_70_reads_9_columns": lambda: _large_diploid(70, 9, 612, 612, 32.0),
    # mcmc_chain_tab<3> / <4>, SMALL false, for k = 3 (and 4); their k = 2 round is mcmc_chain_k2<4, 2> once more
    "tab3_66_reads": lambda: _copies(66, 3, 613, 613, 20.0),
    "tab4_68_reads": lambda: _copies(68, 4, 614, 614, 20.0),
    # either side of big = n > 255: mcmc_chain_tab<2> with its tables in registers (255) and in LDS (256)
    "tab2_255_reads": lambda: _large_diploid(255, 1, 615, 615, 128.0),
    "tab2_256_reads": lambda: _large_diploid(256, 1, 616, 616, 128.0),
}


def device_path(case):
    """(kernel, chain) that chain_split_kernel and mcmc_chain_dispatch send a case to, restated from their conditions; for a
    copy number above 2 the chain of k = copy_num (the rounds of smaller k dispatch on k as a diploid case does on 2)"""
    (n, dim), cp = case["x"].shape, case["copy_num"]
    if cp == 2 and n <= 127 and 1 <= dim <= 8:
        if n <= 63:
            return ("mcmc_kernel_light" if dim <= 2 else "mcmc_kernel", "mcmc_chain_k2<%d, 1>" % (dim if dim <= 4 else 8))
        return ("mcmc_kernel_light" if dim <= 2 else "mcmc_kernel", "mcmc_chain_k2<%d, 2>" % (dim if dim <= 2 else 4 if dim <= 4 else 8))
    return ("mcmc_kernel", "mcmc_chain_tab<%d>%s" % (cp, " SMALL" if n <= 63 else " big" if n > 255 else ""))


def _accepted(g):
    return all(t["accepted"] for t in g.tried)


_moves_a_high_read = lambda g: g.chain["high_read_moves"] > 0
_crosses_64 = lambda g: g.chain["crossed_64"] > 0
# case -> predicate on the reference's log
LARGE_REACHES = {
    "light_64_reads_1_column": lambda g: _accepted(g),   # (reads 0 .. 63: what it adds is the size 64 and the two-register chain)
    "light_65_reads_2_columns": lambda g: _moves_a_high_read(g) and _accepted(g),
    "light_127_reads_2_columns": lambda g: _moves_a_high_read(g) and _crosses_64(g) and _accepted(g),
    "k2_64_reads_3_columns": lambda g: _accepted(g),
    "k2_88_reads_4_columns": lambda g: _moves_a_high_read(g) and _accepted(g),
    "k2_80_reads_6_columns": lambda g: _moves_a_high_read(g) and _accepted(g),
    "k2_127_reads_8_columns": lambda g: _moves_a_high_read(g) and _crosses_64(g) and _accepted(g),
    "k2_120_reads_70_and_50": lambda g: _moves_a_high_read(g) and sorted(g.tried[0]["sizes"]) == [50, 70] and _accepted(g),
    # more than half of ALL proposals are taken, and more than half of those that go downhill (an uphill proposal is always
    # taken and in equilibrium as many moves go up as down, so downhill_taken alone stays below half of all proposals)
    "light_80_reads_weak_columns": lambda g: _moves_a_high_read(g)
    and g.chain["downhill_taken"] + g.chain["zero_diff"] + g.chain["uphill"] > 0.5 * g.chain["proposals"]
    and g.chain["downhill_taken"] > 0.5 * (g.chain["downhill_taken"] + g.chain["rejected"]),
    "light_81_reads_zero_rows": lambda g: g.chain["zero_diff"] > 0 and _moves_a_high_read(g) and _accepted(g),
    "tab2_128_reads_3_columns": lambda g: _moves_a_high_read(g) and _crosses_64(g) and _accepted(g),
    "tab2_70_reads_9_columns": lambda g: _moves_a_high_read(g) and _accepted(g),
    "tab3_66_reads": lambda g: g.range == (2, 3) and [t["k"] for t in g.tried] == [2, 3] and _moves_a_high_read(g) and _accepted(g),
    "tab4_68_reads": lambda g: g.range == (2, 4) and [t["k"] for t in g.tried] == [2, 3, 4] and _moves_a_high_read(g) and _accepted(g),
    "tab2_255_reads": lambda g: _moves_a_high_read(g) and min(g.tried[0]["sizes"]) > 63 and _accepted(g),
    "tab2_256_reads": lambda g: _moves_a_high_read(g) and min(g.tried[0]["sizes"]) > 63 and _accepted(g),
}
LARGE_REACHED_SOMEWHERE = {
    "a chain whose best state is not its last": lambda g: g.chain["best_not_last"] > 0,
}
# what the large cases cover between them: (copy number, reads, columns) classes of the dispatch -> (kernel, chain)
LARGE_PATHS = {
    ("mcmc_kernel_light", "mcmc_chain_k2<1, 2>"), ("mcmc_kernel_light", "mcmc_chain_k2<2, 2>"), ("mcmc_kernel", "mcmc_chain_k2<4, 2>"),
    ("mcmc_kernel", "mcmc_chain_k2<8, 2>"), ("mcmc_kernel", "mcmc_chain_tab<2>"), ("mcmc_kernel", "mcmc_chain_tab<2> big"),
    ("mcmc_kernel", "mcmc_chain_tab<3>"), ("mcmc_kernel", "mcmc_chain_tab<4>"),
}


# ---------------------------------------------------------------------------------------------------------------------------
# pile-ups: reads, not feature matrices (the candidate filter, jtk_lc_cluster_polished, Session.trace)
# ---------------------------------------------------------------------------------------------------------------------------
PILEUPS = {"ont_diploid": {}, "hifi_diploid": {}, "ont_4copy": dict(reads_per_hap=8, tmpl_len=200, divergence=2e-2, min_variants=3),
           "planted": None,
           # 80 reads through the session path, which classifies chains by their LDS need: ont_diploid at 40 reads per haplotype on
           # 200 bp, diverged enough for five candidate columns, three of them picked; the haploid coverage is the reads per haplotype
           "ont_diploid_80_reads": dict(base="ont_diploid", coverage=40.0, reads_per_hap=40, tmpl_len=200, divergence=3e-2, min_variants=3)}

# planted(): the variants the reads carry, as (name, template position, row of the 14, the filter of filter_profiles :440-465 that
# must drop the column, None = it must become a candidate)
PLANTED_TL = 150
PLANTED = [("kept", 60, None), ("edge_low", 4, "edge"), ("edge_high", 147, "edge"), ("ins_in_run", 91, "homopolymer"),
           ("del_in_run", 111, "homopolymer"), ("one_strand", 40, "strand"), ("weak", 75, "gain_per_count")]


def planted():
    """A real pile-up made by hand: a 150 bp template without runs except AAAA at 90..93 and CCCC at 110..113, and 24 error-free
    reads, 12 per strand.  Haplotype B is the template.  The 12 reads of haplotype A (6 per strand) carry a substitution at 60
    (must become a candidate), one 4 bp from either end (inside MASK_LENGTH), an extra A in the A run and one C less in the C run
    (long homopolymers, Ins and Del), and A -> G at 75 under a model whose A -> G mismatch costs 0.03 instead of 0.01: the gain
    per read is ln(0.95 / 0.03) = 3.46, above half the expected 4.56 (so compress_small_gains keeps it) and below 0.8 * 4.56 =
    3.65 (count * expt is not reached while the count's p-value passes).  Every FORWARD read of both haplotypes carries a
    substitution at 40: chi-square 24.  Returns (batch, params, {name: column position bp * 14 + row})."""
    from jtk_amd import batch as jb, ffi
    rng = np.random.default_rng(150)
    t = []
    while len(t) < PLANTED_TL:
        b = int(rng.integers(0, 4))
        if not t or b != t[-1]:
            t.append(b)
    for lo, base in ((90, 0), (110, 1)):
        t[lo:lo + 4] = [base] * 4
        for q in (lo - 1, lo + 4):
            t[q] = (base + 2) % 4 if t[q] == base or t[q] == t[q + (1 if q > lo else -1)] else t[q]
    t[75] = 0
    t[74], t[76] = (1 if t[73] != 1 else 3), (3 if t[77] != 3 else 1)
    for q in range(1, PLANTED_TL):   # (the repairs above must not have made a run)
        assert t[q] != t[q - 1] or 90 < q <= 93 or 110 < q <= 113, q
    other = lambda b: (b + 1) % 4
    col = {"kept": 60 * 14 + other(t[60]), "edge_low": 4 * 14 + other(t[4]), "edge_high": 147 * 14 + other(t[147]),
           "ins_in_run": 91 * 14 + 4 + 0, "del_in_run": 111 * 14 + 11, "one_strand": 40 * 14 + other(t[40]), "weak": 75 * 14 + 2}
    reads, ops, strands = [], [], []
    for r in range(24):
        hap_a, fwd = r % 2 == 0, (r // 2) % 2 == 0
        seq, op = [], []
        for q, b in enumerate(t):
            if hap_a and q == 91:
                seq.append(0)
                op.append(2)                                  # Ins
            if hap_a and q == 111:
                op.append(3)                                  # Del
                continue
            sub = (hap_a and q in (60, 4, 147)) or (fwd and q == 40)
            new = 2 if (hap_a and q == 75) else (other(b) if sub else b)
            seq.append(new)
            op.append(1 if new != b else 0)
        reads.append(np.frombuffer(bytes(b"ACGT"[x] for x in seq), dtype=np.uint8).copy())
        ops.append(np.array(op, dtype=np.uint8))
        strands.append(1 if fwd else 0)
    tmpl = np.frombuffer(bytes(b"ACGT"[x] for x in t), dtype=np.uint8).copy()
    hmm = ffi.default_hmm()
    hmm.mat_emit[0], hmm.mat_emit[2] = 0.95, 0.03             # ref A: read A 0.95, read G 0.03
    b = jb.pack([(7001, 2, tmpl, reads, ops, strands, [r % 2 for r in range(24)])])
    return b, jb.default_params(12.0, 0.03, hmm=hmm), col


def pileup(config):
    """(batch, params) of one pile-up; with fewer reads per haplotype the haploid coverage is 1.25 times that read count (above
    n / copy_num, so that a copy number above 2 takes the coverage as its local coverage, mod.rs:110) unless the entry names its own"""
    if config == "planted":
        return planted()[:2]
    from jtk_amd import batch as jb, synth
    kw = dict(PILEUPS[config])
    base, coverage = kw.pop("base", config), kw.pop("coverage", None)
    b, cfg = synth.make_batch(base, 1, **kw)
    if coverage is None:
        coverage = 1.25 * kw["reads_per_hap"] if "reads_per_hap" in kw else cfg["coverage"]
    return b, jb.default_params(coverage, cfg["band_frac"])
