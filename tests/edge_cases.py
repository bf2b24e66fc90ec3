"""Named trials for `encode_edge` (tests/edge_reference.py, jtk_lc_encode_edges).  A trial is dict(read, start, end, is_forward,
chunks (the edge's chunk sequences), radius, sim_thr); sequences are bytes.  The reference's answers are computed once per
process.  tests/test_edge_reference.py asserts that every trial is what it is named for."""
import functools

import numpy as np

import edge_reference as ER
from encode_reference import window_of
from guided_cases import ACGT, mutate_with_guide, random_seq


def split(seq, chunk_lens):
    out, at = [], 0
    for n in chunk_lens:
        out.append(seq[at:at + n])
        at += n
    assert at == len(seq)
    return out


def place(rng, body, lead, trail, forward=True, lower=False, front=37, back=41):
    """a read that carries `body` in a window with `lead` and `trail` bases of flank (bytes: those bases; int: random ones)"""
    lead = random_seq(rng, lead) if isinstance(lead, int) else lead
    trail = random_seq(rng, trail) if isinstance(trail, int) else trail
    window = lead + body + trail
    if not forward:
        window = window_of(window, 0, len(window), False)
    head = random_seq(rng, front)
    read = head + window + random_seq(rng, back)
    return (read.lower() if lower else read), len(head), len(head) + len(window)


def make(seed, chunk_lens=(200, 200, 200), err=0.08, forward=True, lower=False, sim_thr=0.25, radius=30, lead=25, trail=25, ctg_from=0,
         ctg_to=None, contig=None, body=None):
    """the window carries a copy of contig[ctg_from:ctg_to] at `err` between its flanks"""
    rng = np.random.default_rng(seed)
    contig = random_seq(rng, sum(chunk_lens)) if contig is None else contig
    if body is None:
        body = mutate_with_guide(rng, contig[ctg_from:ctg_to], err)[0]
    read, start, end = place(rng, body, lead, trail, forward, lower)
    return dict(read=read, start=start, end=end, is_forward=forward, chunks=split(contig, chunk_lens), radius=radius, sim_thr=sim_thr)


def leading_ins(seed, k, forward=True):
    """a leading Ins run of k in the guided pass: the first k bases of the contig are A or C, the window's bases in front of the
    copy of the rest G or T.  No two of them match, so both infix alignments tie between k Mismatches and dropping the bases, and
    the walk back takes the diagonal; under (2, -6, -5, -1) k Ins and k Dels (-8 - 2 k) beat k Mismatches (-6 k), and of the two
    orders the walk back takes the Dels first, so the Ins come first in the ops"""
    rng = np.random.default_rng(seed)
    prefix = bytes(b"AC"[v] for v in rng.integers(0, 2, k))
    rest = random_seq(rng, 150)
    junk = bytes(b"GT"[v] for v in rng.integers(0, 2, k + 10))
    return make(seed + 1, chunk_lens=(k + 50, 100), contig=prefix + rest, body=rest, lead=junk, trail=20, radius=80, forward=forward)


def ins_behind_closing_op(seed):
    """six bases that the contig does not have, right behind the copy of chunk 0"""
    rng = np.random.default_rng(seed)
    contig = random_seq(rng, 240)
    extra = bytes(b"ACGT"[(ACGT.index(contig[119]) + 1 + v) % 4] for v in (0, 2, 0, 2, 0, 2))
    return make(seed + 1, chunk_lens=(120, 120), contig=contig, body=contig[:120] + extra + contig[120:])


def _cases():
    c = {}
    c["forward"] = make(1)
    c["reverse"] = make(2, chunk_lens=(150, 250, 200), forward=False)
    c["lower_case"] = make(3, chunk_lens=(100, 100), lower=True)
    c["lower_case_reverse"] = make(4, chunk_lens=(120, 90, 110), lower=True, forward=False)
    # ---- the window against the contig
    c["window_inside_contig"] = make(5, chunk_lens=(150, 150, 150), err=0.03, lead=0, trail=0, ctg_from=100, ctg_to=350)
    c["window_inside_contig_reverse"] = make(6, chunk_lens=(150, 150, 150), err=0.03, lead=0, trail=0, ctg_from=100, ctg_to=350, forward=False)
    c["begins_behind_chunk0"] = make(7, chunk_lens=(150, 150, 150), err=0.03, lead=0, ctg_from=170)
    c["error_free"] = make(8, chunk_lens=(200, 200, 200), err=0.0)
    c["error_free_reverse"] = make(9, chunk_lens=(200, 200, 200), err=0.0, forward=False)
    c["error_40_percent"] = make(10, chunk_lens=(100, 100, 100), err=0.40)
    c["closed_by_virtual_del"] = make(11, chunk_lens=(100, 100, 100), err=0.03, trail=0, ctg_to=150)
    c["ins_behind_closing_op"] = ins_behind_closing_op(12)
    c["chunks_of_3"] = make(13, chunk_lens=(3,) * 70, err=0.05)
    c["chunks_of_3_reverse"] = make(14, chunk_lens=(3,) * 70, err=0.10, forward=False)
    c["one_chunk"] = make(15, chunk_lens=(180,))
    c["contig_longer_than_window"] = make(16, chunk_lens=(200, 200, 200), lead=30, trail=0, ctg_to=250)
    c["window_much_longer"] = make(17, chunk_lens=(60, 60), lead=300, trail=280)
    c["nothing_aligns"] = make(18, chunk_lens=(15, 15), contig=b"AC" * 15, body=b"GT" * 20, lead=0, trail=0)
    # ---- the walk's blocks of 64 ops
    for n in (64, 65, 66):                      # chunk 0's closing op is op n - 1 of the stream
        c["closing_op_%d" % (n - 1)] = make(20 + n, chunk_lens=(n, 70), err=0.0, forward=n != 65)
    for k in (63, 64, 65):
        c["leading_ins_%d" % k] = leading_ins(100 + 2 * k, k, forward=k != 64)
    return c


CASES = _cases()


def wide_band_trial():
    """a radius above 256: rows of more than 512 cells, so the guided pass runs its global-rows kernel"""
    return make(30, chunk_lens=(400, 400), radius=300, lead=30, trail=30)


def big_trial():
    """a 2 kbp contig in 2 chunks"""
    return make(31, chunk_lens=(1000, 1000), err=0.10, radius=100, lead=200, trail=200)


def refused_by_length():
    """a window of 32,001 bases: the first infix alignment refuses it"""
    rng = np.random.default_rng(32)
    return dict(read=random_seq(rng, 32001), start=0, end=32001, is_forward=True, chunks=[random_seq(rng, 100), random_seq(rng, 100)], radius=20, sim_thr=0.25)


def refused_by_band():
    """contig + window >= 32,768 without a distance bound"""
    rng = np.random.default_rng(33)
    return dict(read=random_seq(rng, 32000), start=0, end=32000, is_forward=False, chunks=[random_seq(rng, 400), random_seq(rng, 400)], radius=20,
                sim_thr=0.25)


REFUSED = -3      # JTK_ERR_UNSUPPORTED


def refusal_batch():
    """-> (trials, {index: status of a refused trial}): refused trials first, in the middle and last"""
    names = ("forward", "nothing_aligns", "reverse", "window_inside_contig", "chunks_of_3", "leading_ins_64")
    trials = [CASES[n] for n in names]
    trials.insert(3, refused_by_band())
    trials.insert(0, refused_by_length())
    trials.append(refused_by_band())
    return trials, {0: REFUSED, 4: REFUSED, len(trials) - 1: REFUSED}


def batch70():
    """the named trials and random ones up to 70, in one call"""
    out = list(CASES.values())
    k = 0
    while len(out) < 70:
        lens = ((150, 150), (90, 120, 100), (60,) * 5, (200, 80))[k % 4]
        out.append(make(200 + k, chunk_lens=lens, err=(0.02, 0.1, 0.3)[k % 3], forward=k % 2 == 0, sim_thr=(0.15, 0.25, 0.4)[k % 3], lower=k % 5 == 0,
                        lead=(25, 0, 60)[k % 3], trail=(25, 40, 0)[(k // 3) % 3], ctg_from=(0, 0, 70)[(k // 2) % 3], radius=(20, 30, 45)[k % 3]))
        k += 1
    return out


def contig_of(trial):
    return b"".join(trial["chunks"])


def break_points(trial):
    return np.cumsum([len(c) for c in trial["chunks"]]).tolist()


def _key(t):
    return (t["read"], t["start"], t["end"], t["is_forward"], tuple(t["chunks"]), t["radius"], t["sim_thr"])


@functools.lru_cache(maxsize=None)
def _expected(key):
    read, start, end, forward, chunks, radius, sim_thr = key
    return ER.encode_edge(read, start, end, forward, b"".join(chunks), np.cumsum([len(c) for c in chunks]).tolist(), radius, sim_thr)


def expected(trial):
    """the reference's answer, computed once and shared (callers must not change it)"""
    return _expected(_key(trial))
