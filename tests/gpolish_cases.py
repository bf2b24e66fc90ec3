"""The named cases of the guided polish (tests/test_gpolish_reference.py on the CPU, tests/test_gpu_gpolish.py on the device).

Everything is made from seeds with numpy's RandomState.  A table case is (template, reads, guides, radius); a polish case is a
dict(tmpl, reads, ops, radius, take_num, ignore_edge, max_rounds[, truth]).  Sequences are uint8 arrays of ASCII bases.
"""
import numpy as np

import gpolish_reference as gp

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
MATCH, MISMATCH, INS, DEL = 0, 1, 2, 3


def random_seq(rng, n):
    return ACGT[rng.randint(0, 4, size=n)]


def mutate(rng, seq, rate):
    """every base is substituted, deleted or followed by an inserted base with probability rate / 3 each"""
    out = []
    for b in seq.tolist():
        u = rng.random_sample()
        if u < rate / 3:
            out.append(int(ACGT[(int(np.where(ACGT == b)[0][0]) + 1 + rng.randint(0, 3)) % 4]))
        elif u < 2 * rate / 3:
            continue
        else:
            out.append(b)
            if u < rate:
                out.append(int(ACGT[rng.randint(0, 4)]))
    return np.array(out, dtype=np.uint8)


def pileup(seed, length, n_reads, read_err, draft_err, radius, **kw):
    """a planted case: reads of `truth` at read_err, a draft of it at draft_err as the template, global ops as the guides"""
    rng = np.random.RandomState(seed)
    truth = random_seq(rng, length)
    tmpl = mutate(rng, truth, draft_err)
    reads = [mutate(rng, truth, read_err) for _ in range(n_reads)]
    case = dict(tmpl=tmpl, reads=reads, ops=[gp.global_ops(tmpl, r) for r in reads], radius=radius, take_num=0, ignore_edge=0,
                max_rounds=0, truth=truth)
    case.update(kw)
    return case


# truth of 70 / 150 / 300 bases; 8 / 12 / 10 reads at 8-12 % error; a draft at 3-5 %; radius 6 / 10 / 12
PLANTED = {
    "planted70": lambda: pileup(7001, 70, 8, 0.08, 0.04, 6),
    "planted150": lambda: pileup(15001, 150, 12, 0.10, 0.03, 10),
    "planted300": lambda: pileup(30001, 300, 10, 0.12, 0.05, 12),
}


def no_reads():
    rng = np.random.RandomState(11)
    return dict(tmpl=random_seq(rng, 40), reads=[], ops=[], radius=5, take_num=0, ignore_edge=0, max_rounds=0)


def many_reads():
    """70 reads of about 40 bases: more reads than lanes.  Two rounds, so that the reference stays quick; the limit ends the loop
    after a round that applied edits"""
    return pileup(4001, 40, 70, 0.10, 0.05, 5, max_rounds=2)


def short_template():
    """2 ignore_edge >= n: nothing is scanned, the reads are only aligned"""
    return pileup(601, 6, 4, 0.15, 0.2, 4, ignore_edge=3)


def hand(truth, tmpl, radius=4, n_reads=3, **kw):
    """reads that are exact copies of `truth` over a template that differs from it by edits made by hand"""
    truth, tmpl = gp.as_seq(truth), gp.as_seq(tmpl)
    case = dict(tmpl=tmpl, reads=[truth.copy() for _ in range(n_reads)], ops=[gp.global_ops(tmpl, truth) for _ in range(n_reads)], radius=radius,
                take_num=0, ignore_edge=0, max_rounds=0, truth=truth)
    case.update(kw)
    return case


# the template lacks the second CA of GTCACATG (copying two bases restores it: row 9) and, twelve bases on, the G of ATGCT
# (inserting it: row 6); no single base does what the copy does, so the copy's gain is twice an insertion's
HAND_GROW = (b"TTAGTCACATGATTACCATGCTAATCCGTAAGTC", b"TTAGTCATGATTACCATCTAATCCGTAAGTC")
# the template has ATA in front of its last base that the reads do not: deleting three bases at n - 4 is the last deletion of three
# that exists (an edit must leave a base behind it; its last base is n - 2).  A deletion of three further left would already
# gain, so a substitution at n - 10 is applied first and its 1 + inactive(0) = 6 positions end at n - 4.
HAND_SHRINK = (b"ATCATTTTCTCGATGAAAGCGTTGACCCCA", b"ATCATTTTCTCGATGAAAGCGTTTACCCCCATA")


POLISH = dict(PLANTED)
POLISH.update({
    "hand_grow": lambda: hand(*HAND_GROW),
    "hand_shrink": lambda: hand(*HAND_SHRINK),
    "hand_shrink_edge4": lambda: hand(*HAND_SHRINK, ignore_edge=4),
    "take3of8": lambda: pileup(7001, 70, 8, 0.08, 0.04, 6, take_num=3),
    "ignore_edge3": lambda: pileup(7001, 70, 8, 0.08, 0.04, 6, ignore_edge=3),
    "one_round": lambda: pileup(15001, 150, 12, 0.10, 0.03, 10, max_rounds=1),
    "no_reads": no_reads,
    "short_template": short_template,
    "many_reads": many_reads,
    "ring_rounds": lambda: ring_rounds(),
    "f16_polish": lambda: f16_polish(),
})


def too_wide():
    """a guide whose first row spans more than JTK_GUIDED_MAX_WIDTH columns: 4,200 Ins in front of the diagonal"""
    rng = np.random.RandomState(13)
    tmpl = random_seq(rng, 8)
    read = np.concatenate([random_seq(rng, 4200), tmpl])
    ops = np.array([INS] * 4200 + [MATCH] * 8, dtype=np.uint8)
    return dict(tmpl=tmpl, reads=[read], ops=[ops], radius=2, take_num=0, ignore_edge=0, max_rounds=0)


def table_case(seed, n, lengths, radius, err=0.1):
    rng = np.random.RandomState(seed)
    tmpl = random_seq(rng, n)
    reads = []
    for m in lengths:
        if m is None:
            reads.append(mutate(rng, tmpl, err))
        else:
            reads.append(random_seq(rng, m))
    return tmpl, reads, [gp.global_ops(tmpl, r) for r in reads], radius


def long_runs():
    """a 70-long Ins run and a 70-long Del run in the guide: a row whose path alone spans more than 64 columns, and row offsets
    that jump"""
    rng = np.random.RandomState(17)
    tmpl = random_seq(rng, 110)
    read = np.concatenate([tmpl[:10], random_seq(rng, 70), tmpl[80:]])
    guide = np.array([MATCH] * 10 + [INS] * 70 + [DEL] * 70 + [MATCH] * 30, dtype=np.uint8)
    other = mutate(rng, tmpl, 0.1)
    return tmpl, [read, other], [guide, gp.global_ops(tmpl, other)], 3


def homopolymer():
    tmpl = np.frombuffer(b"AAAAAAAAAA", dtype=np.uint8)
    reads = [np.frombuffer(s, dtype=np.uint8) for s in (b"AAAAAAAAAAA", b"AAAAAAAAA", b"AAAACAAAAAA", b"AAAAAAAAAA")]
    return tmpl, reads, [gp.global_ops(tmpl, r) for r in reads], 4


def spread_guide(n, m):
    """m Ins ops spread evenly in front of, between and behind n Match ops: the widest row's path spans about m / (n + 1) columns"""
    q, rest = divmod(m, n + 1)
    guide = []
    for i in range(n + 1):
        guide += [INS] * (q + (1 if i < rest else 0)) + ([MATCH] if i < n else [])
    return np.array(guide, dtype=np.uint8)


def run_guide(n, m, at):
    """the m - n Ins ops in one run behind `at` Match ops"""
    return np.array([MATCH] * at + [INS] * (m - n) + [MATCH] * (n - at), dtype=np.uint8)


def ring_wide(seed, n, lengths=(513, 600, 700)):
    """reads of 513 ..= 700 bases at a radius beyond the matrix: every row is m + 1 cells, kept in the global ring"""
    rng = np.random.RandomState(seed)
    tmpl = random_seq(rng, n)
    reads = [random_seq(rng, m) for m in lengths]
    return tmpl, reads, [spread_guide(n, m) for m in lengths], 800


def ring_ins_run(seed, n):
    """radius 2 and a 520-op Ins run in the guide: one row passes 512 cells by its path alone, the others are a few cells"""
    rng = np.random.RandomState(seed)
    tmpl = random_seq(rng, n)
    reads, guides = [], []
    for at in sorted({0, n // 2, n}):
        reads.append(np.concatenate([tmpl[:at], random_seq(rng, 520), tmpl[at:]]))
        guides.append(run_guide(n, n + 520, at))
    return tmpl, reads, guides, 2


def ring_mixed_block():
    """eight reads, two blocks of four waves, at radius 3; in each block: a read of at most 511 bases (no ring reserved), a read
    of 600 whose widest row stays under 512 cells (ring reserved, LDS used), and two whose widest row passes 512"""
    rng = np.random.RandomState(31)
    n = 12
    tmpl = random_seq(rng, n)
    reads, guides = [], []
    for m, make in ((400, spread_guide), (600, spread_guide), (540, lambda n, m: run_guide(n, m, 5)), (650, lambda n, m: run_guide(n, m, 0)),
                    (700, lambda n, m: run_guide(n, m, n)), (511, lambda n, m: run_guide(n, m, 7)), (640, spread_guide), (560, lambda n, m: run_guide(n, m, 11))):
        reads.append(random_seq(rng, m))
        guides.append(make(n, m))
    return tmpl, reads, guides, 3


def ring_width4096():
    """a read of 4,095 bases at a radius beyond it: six rows of JTK_GUIDED_MAX_WIDTH cells, the ring's whole stride"""
    rng = np.random.RandomState(37)
    tmpl = random_seq(rng, 5)
    reads = [random_seq(rng, 4095), random_seq(rng, 30)]
    return tmpl, reads, [spread_guide(5, 4095), spread_guide(5, 30)], 5000


# the longest sequences the polish takes, and 16-bit cells above 32,767: template all A, read all C, the guide blocks of 100 Del
# and 100 Ins, so that the band holds little but the guide's own path and the banded distance is nearly n + m
def f16_case(n, radius):
    k = 100
    assert n % k == 0
    tmpl = np.full(n, ord("A"), dtype=np.uint8)
    read = np.full(n, ord("C"), dtype=np.uint8)
    guide = np.array(([DEL] * k + [INS] * k) * (n // k), dtype=np.uint8)
    return tmpl, [read], [guide], radius


F16_TABLE_N = 16600      # the smallest multiple of 100 whose distance at radius 0, n / 100 * 198 + 1, passes 32,767
MAX_LEN = 32000          # GP_MAX_LEN of gpolish.hip


def f16_polish():
    """the 32,000-base pair as a pile-up: ignore_edge leaves nothing to scan, so the read is aligned and measured, not tabled"""
    tmpl, reads, guides, radius = f16_case(MAX_LEN, 1)
    return dict(tmpl=tmpl, reads=reads, ops=guides, radius=radius, take_num=0, ignore_edge=MAX_LEN // 2, max_rounds=0)


def ring_rounds():
    """a planted pile-up whose bands stay in the global ring while the template changes: a truth of 14 bases with a shared
    insertion of 520 in every read, a radius beyond the matrix, two rounds"""
    rng = np.random.RandomState(41)
    truth = random_seq(rng, 14)
    extra = random_seq(rng, 520)
    tmpl = mutate(rng, truth, 0.2)
    reads = [mutate(rng, np.concatenate([truth[:7], mutate(rng, extra, 0.02), truth[7:]]), 0.05) for _ in range(4)]
    return dict(tmpl=tmpl, reads=reads, ops=[spread_guide(len(tmpl), len(r)) for r in reads], radius=700, take_num=0, ignore_edge=0, max_rounds=2)


def too_long_template():
    rng = np.random.RandomState(43)
    tmpl = random_seq(rng, MAX_LEN + 1)
    return dict(tmpl=tmpl, reads=[tmpl[:50]], ops=[np.array([MATCH] * 50 + [DEL] * (MAX_LEN + 1 - 50), dtype=np.uint8)], radius=2, take_num=0,
                ignore_edge=0, max_rounds=0)


def too_long_read():
    rng = np.random.RandomState(47)
    read = random_seq(rng, MAX_LEN + 1)
    other = random_seq(rng, 40)
    return dict(tmpl=read[:50], reads=[other, read], ops=[gp.global_ops(read[:50], other), np.array([MATCH] * 50 + [INS] * (MAX_LEN + 1 - 50), dtype=np.uint8)],
                radius=2, take_num=0, ignore_edge=0, max_rounds=0)


def outgrows():
    """a template of 40 bases under reads of about 300: the consensus grows towards the reads, past tmpl_cap = 40 + 64 + 40 / 8
    = 109, which the device refuses and the reference, which has no cap, does not (tests/test_gpolish_reference.py)"""
    rng = np.random.RandomState(53)
    truth = random_seq(rng, 320)
    tmpl = truth[::8].copy()
    reads = [mutate(rng, truth[:300], 0.03) for _ in range(4)]
    return dict(tmpl=tmpl, reads=reads, ops=[gp.global_ops(tmpl, r) for r in reads], radius=12, take_num=0, ignore_edge=0, max_rounds=0)


OUTGROWS_CAP = 40 + 64 + 40 // 8

# One call at the defaults (every read votes, no edge, 20 rounds) with the three refusals beside pile-ups that are answered
LIMITS = ["planted70", "too_long_template", "no_reads", "too_long_read", "outgrows", "planted150"]
LIMITS_STATUS = {"too_long_template": -3, "too_long_read": -3, "outgrows": -6}
SPECIAL = {"too_wide": too_wide, "too_long_template": too_long_template, "too_long_read": too_long_read, "outgrows": outgrows,
           "ring_rounds": ring_rounds, "f16_polish": f16_polish}


TABLE = {
    "ring_n1_wide": lambda: ring_wide(25, 1),
    "ring_n5_wide": lambda: ring_wide(26, 5),
    "ring_n12_wide": lambda: ring_wide(27, 12),
    "ring_n1_ins_run": lambda: ring_ins_run(28, 1),
    "ring_n5_ins_run": lambda: ring_ins_run(29, 5),
    "ring_n12_ins_run": lambda: ring_ins_run(30, 12),
    "ring_mixed_block": ring_mixed_block,
    "ring_width4096": ring_width4096,
    "f16_table": lambda: f16_case(F16_TABLE_N, 0),
    "n1": lambda: table_case(21, 1, [0, 1, 1, 3], 2),
    "n12_r0": lambda: table_case(22, 12, [None, None, 12, 9], 0),
    "n12_r1": lambda: table_case(22, 12, [None, None, 12, 9], 1),
    "n12_r40": lambda: table_case(22, 12, [None, None, 12, 9], 40),
    "n150_r40": lambda: table_case(23, 150, [None, None], 40),      # a row of 81 cells: two 64-column pieces
    "n150_r70": lambda: table_case(24, 150, [None, None], 70),      # three pieces
    "long_runs": long_runs,
    "homopolymer": homopolymer,
}


_cache = {}


def case(name):
    """a named polish case (or "too_wide"), made once"""
    if ("case", name) not in _cache:
        _cache["case", name] = SPECIAL[name]() if name in SPECIAL else POLISH[name]()
    return _cache["case", name]


def expected(name):
    """the reference's answer for a named polish case, computed once: (consensus, ops, dists, rounds)"""
    if ("polish", name) not in _cache:
        c = case(name)
        _cache["log", name] = []
        _cache["polish", name] = gp.polish(c["tmpl"], c["reads"], c["ops"], c["radius"], c["take_num"], c["ignore_edge"], c["max_rounds"],
                                           log=_cache["log", name])
    return _cache["polish", name]


def rounds_log(name):
    """[(t, n, gain, dead, edits)] of the rounds of a named polish case that scanned, from the run that expected() made"""
    expected(name)
    return _cache["log", name]


def table_expected(name):
    """-> (case, [(dist, T, ops) per read]) of a named table case, computed once"""
    if ("table", name) not in _cache:
        tmpl, reads, guides, radius = TABLE[name]()
        _cache["table", name] = ((tmpl, reads, guides, radius), [gp.table(tmpl, r, g, radius) for r, g in zip(reads, guides)])
    return _cache["table", name]


# One call that mixes the distinct inputs above with a pile-up beyond JTK_GUIDED_MAX_WIDTH.  A call has one take_num, one
# ignore_edge and one round limit: every read votes, nothing is ignored, and two rounds keep the reference quick (the limit then
# ends most of these after a round that applied edits).
MIXED = ["planted70", "no_reads", "planted150", "too_wide", "short_template", "many_reads", "planted300"]
MIXED_ROUNDS = 2


def mixed_expected(name):
    if ("mixed", name) not in _cache:
        c = case(name)
        _cache["mixed", name] = gp.polish(c["tmpl"], c["reads"], c["ops"], c["radius"], 0, 0, MIXED_ROUNDS)
    return _cache["mixed", name]
