"""`encode_node` with `fine_mapping` and `fit_query_by_edlib` (haplotyper/src/encode/deletion_fill.rs:451-566), restated on
top of tests/align_modes_reference.py (edlib's infix alignment as DESIGN section 4 specifies it) and
tests/guided_reference.py (kiley's infix_guided as DESIGN section 4 specifies it; parity with kiley itself is not pinned).

One difference from the reference, as jtk_lc_encode_nodes has it: the third pass (:526) is computed for every trial that
passes the lower-bound filter, and the verdict is taken afterwards.
"""
import math

import numpy as np

import align_modes_reference as AM
import guided_reference as G

EDGE_LEN = 100        # deletion_fill.rs:9
EDGE_BOUND = 0.5      # :7
OFFSET_FACTOR = 0.1   # :293
ACCEPTED, LOWER_BOUND, REJECTED = 0, 1, 2
COMPLEMENT = {ord("A"): ord("T"), ord("C"): ord("G"), ord("G"): ord("C"), ord("T"): ord("A")}


def window_of(read, start, end, is_forward):
    """:467-472"""
    w = bytes(read[start:end]).upper()
    return w if is_forward else bytes(COMPLEMENT[b] for b in reversed(w))


def band_of(window_len, sim_thr):
    """:552"""
    return max(int(math.ceil(float(window_len) * sim_thr * 0.3)), 10)


def first_guide(cons, window):
    """:544-550 in the guided orientation (x = window, y = consensus): edlib's ops with the window's free ends as Dels"""
    ops, _dist, start, end = AM.align(np.frombuffer(cons, np.uint8), np.frombuffer(window, np.uint8), AM.INFIX, AM.FREE_READ)
    swap = {G.MATCH: G.MATCH, G.MISMATCH: G.MISMATCH, G.INS: G.DEL, G.DEL: G.INS}   # there Ins is a window base, here a Del is
    return [G.DEL] * start + [swap[int(op)] for op in ops] + [G.DEL] * (len(window) - end)


def trim_head_tail_insertion(ops):
    """:595-609: the tail first"""
    ops = list(ops)
    tail = 0
    while ops and ops[-1] == G.INS:
        ops.pop()
        tail += 1
    head = 0
    while ops and ops[0] == G.INS:
        ops.pop(0)
        head += 1
    return ops, head, tail


def edge_counts(cons_len, ops, length=EDGE_LEN):
    """:568-592 -> head_match, head_len, tail_match, tail_len"""
    head_end = min(length, cons_len)
    tail_start = max(cons_len - length, 0)
    rpos = 0
    hm = hl = tm = tl = 0
    for op in ops:
        if op != G.INS:
            rpos += 1
        if rpos < head_end:
            hl += 1
            hm += op == G.MATCH
        if tail_start <= rpos:
            tl += 1
            tm += op == G.MATCH
    return hm, hl, tm, tl


def _div(a, b):
    return a / b if b else float("nan")     # counts: a <= b, so only 0 / 0 divides by zero


def _rust_min(a, b):
    """f64::min: the other operand when one is NaN"""
    if a != a:
        return b
    if b != b:
        return a
    return min(a, b)


def encode_node(read, start, end, is_forward, cons, chunk_seq, sim_thr):
    assert start < end
    wl = end - start
    out = dict(status=0, verdict=REJECTED, trim_head=0, trim_tail=0, position_from_start=start, query_len=0, band=band_of(wl, sim_thr),
               score=0, mat_num=0, ops_len=0, head_match=0, head_len=0, tail_match=0, tail_len=0, ops=[])
    if sim_thr < max(len(cons) - wl, 0) / len(cons):         # :461-465
        out["verdict"] = LOWER_BOUND
        return out
    window = window_of(read, start, end, is_forward)
    band = out["band"]
    ops = first_guide(cons, window)
    for _ in range(2):                                        # :553-554
        ops = G.align_guided(window, cons, ops, band, infix=True)["ops"]
    ops = [G.DEL if op == G.INS else G.INS if op == G.DEL else op for op in ops]   # :556-562
    ops, head, tail = trim_head_tail_insertion(ops)
    query = window[head:len(window) - tail]
    mat_num = sum(op == G.MATCH for op in ops)
    hm, hl, tm, tl = edge_counts(len(cons), ops)
    third = G.align_guided(chunk_seq, query, ops, band, infix=True)              # :526
    identity = _div(mat_num, len(ops))
    ok = 1.0 - sim_thr < identity and EDGE_BOUND < _rust_min(_div(hm, hl), _div(tm, tl))
    out.update(verdict=ACCEPTED if ok else REJECTED, trim_head=head, trim_tail=tail,
               position_from_start=start + (head if is_forward else tail), query_len=len(query), score=third["score"], mat_num=mat_num,
               ops_len=len(ops), head_match=hm, head_len=hl, tail_match=tm, tail_len=tl, ops=third["ops"], query=query)
    return out


def fill_trials(side, candidates, seq_len, next_node, cons_len_of):
    """try_encoding_head / _tail (:370-446) up to the call of encode_node: which candidates are tried, on which window.
    side 0 = head (position = start_position), 1 = tail (end_position); candidates: (chunk, cluster, is_forward, position);
    next_node: None or (chunk, position_from_start) of nodes.get(idx); -> [(candidate index, start, end)]"""
    out = []
    for k, (chunk, cluster, _forward, position) in enumerate(candidates):
        if side == 0 and not 0 <= position < seq_len:         # :381; a negative position is the wrapped usize
            continue
        if position < 0:      # tail: the wrapped usize gives start = seq_len - (offset + cons_len) >= end, and :428 asserts
            raise ValueError("negative tail position")
        cons_len = cons_len_of(chunk, cluster)
        if cons_len is None:
            continue
        offset = int(math.ceil(OFFSET_FACTOR * cons_len))
        if side == 0:
            end_position = min(position + cons_len + offset, seq_len)
            start_position = max(position - offset, 0)
        else:
            start_position = max(min(position, seq_len) - (offset + cons_len), 0)
            end_position = min(position + offset, seq_len)
        assert start_position < end_position
        if next_node is not None and next_node[0] == chunk and abs(next_node[1] - start_position) < cons_len:
            continue
        out.append((k, start_position, end_position))
    return out
