"""Named trials for `encode_node` (tests/encode_reference.py, jtk_lc_encode_nodes).  A trial is dict(read, start, end,
is_forward, cons, chunk_seq, sim_thr); sequences are bytes.  The reference's answers are computed once per process."""
import functools

import numpy as np

import encode_reference as E
from guided_cases import ACGT, mutate_with_guide, random_seq


def other_base(b):
    return ACGT[(ACGT.index(b) + 1) % 4]


def make(seed, cons_len=200, err=0.08, forward=True, sim_thr=0.25, lead=None, trail=None, chunk_delta=0, lower=False, spoil_head=0,
         spoil_tail=0):
    """a read that carries a copy of the consensus at `err`, in a window with `lead` and `trail` bases of flank"""
    rng = np.random.default_rng(seed)
    cons = random_seq(rng, cons_len)
    lead = cons_len // 10 if lead is None else lead
    trail = cons_len // 10 if trail is None else trail
    node = bytearray(mutate_with_guide(rng, cons, err)[0])
    # spoiled ends: a run of the letter that the consensus has fewest of there (bases that merely differ column by column
    # would still find half of themselves again in a gapped alignment)
    rare = lambda part: min(ACGT, key=part.count)
    for q in range(min(spoil_head, len(node))):
        node[q] = rare(cons[:100])
    for q in range(min(spoil_tail, len(node))):
        node[len(node) - 1 - q] = rare(cons[-100:])
    window = random_seq(rng, lead) + bytes(node) + random_seq(rng, trail)
    if not forward:
        window = E.window_of(window, 0, len(window), False)
    front = random_seq(rng, 37)
    read = front + window + random_seq(rng, 41)
    if lower:
        read = read.lower()
    if chunk_delta >= 0:
        chunk_seq = mutate_with_guide(rng, cons, 0.01)[0] + random_seq(rng, chunk_delta)
    else:
        chunk_seq = mutate_with_guide(rng, cons, 0.01)[0][:chunk_delta]
    return dict(read=read, start=len(front), end=len(front) + len(window), is_forward=forward, cons=cons, chunk_seq=chunk_seq, sim_thr=sim_thr)


def _cases():
    c = {}
    c["forward"] = make(1, cons_len=200)
    c["reverse"] = make(2, cons_len=250, forward=False)
    c["lower_case"] = make(3, cons_len=150, lower=True)
    c["lower_case_reverse"] = make(4, cons_len=180, lower=True, forward=False)
    # ---- one per verdict
    c["accepted"] = make(5, cons_len=300, err=0.05)
    short = make(6, cons_len=200, lead=0, trail=0)
    short["end"] = short["start"] + 100                      # (200 - 100) / 200 = 0.5 > 0.3
    short["sim_thr"] = 0.3
    c["lower_bound"] = short
    edge = dict(short, sim_thr=0.5)                          # 0.5 < 0.5 is false: the filter lets it pass by equality
    c["lower_bound_equal"] = edge
    c["identity_rejected"] = make(7, cons_len=200, err=0.40, sim_thr=0.25)
    c["head_edge_rejected"] = make(8, cons_len=250, err=0.03, sim_thr=0.4, spoil_head=60)
    c["tail_edge_rejected"] = make(9, cons_len=250, err=0.03, sim_thr=0.4, spoil_tail=60, forward=False)
    # ---- counts and trims
    c["cons_shorter_than_edge"] = make(10, cons_len=80, err=0.05)
    c["trims_reverse"] = make(11, cons_len=160, forward=False, lead=31, trail=9)
    c["trims_forward"] = make(12, cons_len=160, lead=3, trail=40)
    c["no_flanks"] = make(13, cons_len=170, lead=0, trail=0)
    c["chunk_longer"] = make(14, cons_len=200, chunk_delta=5)
    c["chunk_shorter"] = make(15, cons_len=200, chunk_delta=-5)
    c["band_is_10"] = make(16, cons_len=200, err=0.03, sim_thr=0.1)      # ceil(about 240 * 0.1 * 0.3) = 8
    c["band_is_wider"] = make(17, cons_len=200, err=0.2, sim_thr=0.5)    # ceil(about 240 * 0.5 * 0.3) = 36
    # ---- counts at their edges (tests/test_guided_reference.py asserts that they are what they are named for)
    c["cons_len1"] = make(20, cons_len=1, err=0.0, lead=6, trail=5, sim_thr=0.5)      # head_len 0: the verdict goes through 0 / 0
    for n in (99, 100, 101):                                                           # head_end and tail_start at EDGE_LEN
        c["cons_len%d" % n] = make(20 + n, cons_len=n, err=0.05, forward=n != 100)
    for k, (lead, trail) in enumerate(((63, 65), (64, 64), (65, 63))):
        c["trims_%d_%d" % (lead, trail)] = make(130 + k, cons_len=150, err=0.0, lead=lead, trail=trail, sim_thr=0.4)
        c["trims_%d_%d_reverse" % (lead, trail)] = make(140 + k, cons_len=150, err=0.0, lead=lead, trail=trail, sim_thr=0.4, forward=False)
    c["ops_len64"] = make(150, cons_len=64, err=0.0, lead=9, trail=4)
    c["ops_len128"] = make(151, cons_len=128, err=0.0, lead=3, trail=14, forward=False)
    return c


CASES = _cases()


def wide_band_trial():
    """a band of more than 256: rows of more than 512 cells in all three passes, which run the global-rows kernel on descriptors
    that the kernels between the passes wrote.  sim_thr 1.0 makes the band 0.3 of the window, so 860 bases are enough"""
    return make(19, cons_len=770, err=0.08, sim_thr=1.0, lead=45, trail=45)


def refused_by_infix():
    """a consensus of 32,001 bases: the infix alignment refuses it (JTK_ERR_UNSUPPORTED), the filter lets it pass"""
    rng = np.random.default_rng(31)
    cons = random_seq(rng, 32001)
    return dict(read=random_seq(rng, 400), start=50, end=350, is_forward=True, cons=cons, chunk_seq=cons[:300], sim_thr=0.999)


def refused_by_guided_pass(forward=True):
    """the consensus holds 4,200 T between the halves of a window without a T: the infix alignment makes them one Ins run, the
    first guided pass meets a row of more than 4,096 cells and refuses the trial, and the two passes behind it see that status"""
    rng = np.random.default_rng(32)
    node = bytes(b"ACG"[k] for k in rng.integers(0, 3, 200))
    cons = node[:100] + b"T" * 4200 + node[100:]
    window = node if forward else E.window_of(node, 0, len(node), False)
    return dict(read=b"ACGTA" + window + b"GG", start=5, end=205, is_forward=forward, cons=cons, chunk_seq=node, sim_thr=0.97)


def refused_by_length():
    """a chunk sequence of 32,001 bases: the third guided pass would not take it, and the trial is refused before the first"""
    rng = np.random.default_rng(33)
    t = dict(CASES["forward"])
    t["chunk_seq"] = random_seq(rng, 32001)
    return t


REFUSED = -3      # JTK_ERR_UNSUPPORTED


def refusal_batch():
    """-> (trials, {index: status of a refused trial}): refused trials of each kind first, in the middle and last, between trials
    that stop at the lower bound and trials that are answered"""
    names = ("forward", "lower_bound", "reverse", "accepted", "lower_bound", "identity_rejected", "trims_reverse", "lower_bound_equal")
    trials = [CASES[n] for n in names]
    trials.insert(4, refused_by_infix())
    trials.insert(3, refused_by_length())
    trials.insert(0, refused_by_guided_pass())
    trials.append(refused_by_guided_pass(forward=False))
    return trials, {0: REFUSED, 4: REFUSED, 6: REFUSED, len(trials) - 1: REFUSED}


def shared_layout():
    """-> (read, cons, chunk_seq, [(start, end, is_forward, sim_thr)]): trials as production lays them out, windows of one read
    (overlapping ones, and forward and reverse ones over the same bases) against one consensus and one chunk sequence"""
    rng = np.random.default_rng(34)
    cons = random_seq(rng, 180)
    chunk_seq = mutate_with_guide(rng, cons, 0.01)[0]
    first = mutate_with_guide(rng, cons, 0.06)[0]
    second = E.window_of(mutate_with_guide(rng, cons, 0.1)[0], 0, 10 ** 6, False)      # a copy on the reverse strand
    parts = [random_seq(rng, 40), first, random_seq(rng, 25), second, random_seq(rng, 30)]
    read = b"".join(parts).lower()
    a0, a1 = len(parts[0]), len(parts[0]) + len(first)
    b0, b1 = a1 + len(parts[2]), a1 + len(parts[2]) + len(second)
    windows = [(a0 - 18, a1 + 18, True, 0.25), (a0 - 11, a1 + 25, True, 0.25), (a0 - 18, a1 + 18, False, 0.25), (b0 - 18, b1 + 18, False, 0.25),
               (b0 - 18, b1 + 18, True, 0.4), (b0 - 3, b1 + 20, False, 0.15), (a0 - 18, a0 + 60, True, 0.3), (a1 - 30, b0 + 40, True, 0.35)]
    return read, cons, chunk_seq, windows


def shared_trials():
    read, cons, chunk_seq, windows = shared_layout()
    return [dict(read=read, start=s, end=e, is_forward=f, cons=cons, chunk_seq=chunk_seq, sim_thr=thr) for s, e, f, thr in windows]


def big_trial():
    """a 2 kbp consensus in a 2.4 kbp window"""
    return make(18, cons_len=2000, err=0.10, sim_thr=0.15)


def batch70():
    """the named trials and random ones up to 70, in one call"""
    out = list(CASES.values())
    k = 0
    while len(out) < 70:
        out.append(make(100 + k, cons_len=150 + 5 * (k % 31), err=(0.02, 0.1, 0.3)[k % 3], forward=k % 2 == 0, sim_thr=(0.15, 0.25, 0.4)[k % 3],
                        chunk_delta=(0, 5, -5)[k % 3], lower=k % 5 == 0))
        k += 1
    return out


def _key(t):
    return (t["read"], t["start"], t["end"], t["is_forward"], t["cons"], t["chunk_seq"], t["sim_thr"])


@functools.lru_cache(maxsize=None)
def _expected(key):
    return E.encode_node(*key)


def expected(trial):
    """the reference's answer, computed once and shared (callers must not change it)"""
    return _expected(_key(trial))
