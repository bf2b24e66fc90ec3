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
    return c


CASES = _cases()


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
