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


POLISH = dict(PLANTED)
POLISH.update({
    "take3of8": lambda: pileup(7001, 70, 8, 0.08, 0.04, 6, take_num=3),
    "ignore_edge3": lambda: pileup(7001, 70, 8, 0.08, 0.04, 6, ignore_edge=3),
    "one_round": lambda: pileup(15001, 150, 12, 0.10, 0.03, 10, max_rounds=1),
    "no_reads": no_reads,
    "short_template": short_template,
    "many_reads": many_reads,
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


TABLE = {
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
        _cache["case", name] = too_wide() if name == "too_wide" else POLISH[name]()
    return _cache["case", name]


def expected(name):
    """the reference's answer for a named polish case, computed once: (consensus, ops, dists, rounds)"""
    if ("polish", name) not in _cache:
        c = case(name)
        _cache["polish", name] = gp.polish(c["tmpl"], c["reads"], c["ops"], c["radius"], c["take_num"], c["ignore_edge"], c["max_rounds"])
    return _cache["polish", name]


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
