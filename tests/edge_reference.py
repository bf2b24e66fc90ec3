"""`tune_position`, `encode_edge` and `fill_edges_by_new_chunks` (haplotyper/src/dense_encoding.rs:713-759, :627-697, :202-293),
restated on top of tests/align_modes_reference.py (edlib's infix alignment as DESIGN section 4 specifies it) and
tests/guided_reference.py (kiley's global_guided as DESIGN section 4 specifies it; parity with kiley itself is not pinned).

Differences from the reference, as jtk_lc_encode_edges has them: every chunk gets a record (verdict 0 accepted, 2 rejected,
3 not reached) in chunk order, not only the accepted ones; a truncated window of length 0 gives no chunk reached, where the
reference would hand edlib an empty sequence."""
import numpy as np

import align_modes_reference as AM
import guided_reference as G
from encode_reference import window_of

ACCEPTED, REJECTED, NOT_REACHED = 0, 2, 3
MARGIN = 25         # :209


def tune_position(read, start, end, is_forward, contig, band):
    """:713-759 -> dict(window, seq_start, seq_end (inside the oriented window), ctg_start, ctg_end, score, ops), or with
    ops None when the truncated window is empty"""
    assert start < end
    window = window_of(read, start, end, is_forward)                                  # :722-727
    as_u8 = lambda s: np.frombuffer(bytes(s), np.uint8)                               # noqa: E731
    _ops, _d, seq_start, seq_end = AM.align(as_u8(contig), as_u8(window), AM.INFIX, AM.FREE_READ)        # :731
    out = dict(window=window, seq_start=seq_start, seq_end=seq_end, ctg_start=0, ctg_end=0, score=0, ops=None)
    seq = window[seq_start:seq_end]
    if not seq:
        return out
    guide, _d, ctg_start, ctg_end = AM.align(as_u8(contig), as_u8(seq), AM.INFIX, AM.FREE_TEMPLATE)      # :746-755
    res = G.align_guided(contig[ctg_start:ctg_end], seq, [int(op) for op in guide], band, infix=False)  # :757
    out.update(ctg_start=ctg_start, ctg_end=ctg_end, score=res["score"], ops=res["ops"])
    return out


def _node(verdict=NOT_REACHED):
    return dict(verdict=verdict, mat_num=0, ops_len=0, query_off=0, query_len=0, position_from_start=0, ops=[])


def encode_edge(read, start, end, is_forward, contig, break_points, band, sim_thr):
    """:627-697 -> dict(seq_start, seq_end, ctg_start, ctg_end, score, first_chunk, head_ins, nodes (one per chunk, in chunk
    order), closed_by (per chunk: "lead" is never a closer; "op" = one of the pass's ops, "tail" = a Del behind them, None))"""
    break_points = [int(b) for b in break_points]
    n_chunks = len(break_points)
    assert n_chunks and break_points[-1] == len(contig) and all(a < b for a, b in zip([0] + break_points, break_points))
    tp = tune_position(read, start, end, is_forward, contig, band)
    out = dict(status=0, seq_start=tp["seq_start"], seq_end=tp["seq_end"], ctg_start=tp["ctg_start"], ctg_end=tp["ctg_end"], score=tp["score"],
               first_chunk=n_chunks, head_ins=0, nodes=[_node() for _ in range(n_chunks)], closed_by=[None] * n_chunks, window=tp["window"])
    if tp["ops"] is None:
        return out
    ctg_start, ctg_end, seq_start = tp["ctg_start"], tp["ctg_end"], tp["seq_start"]
    ops = list(tp["ops"])
    real = len(ops)
    ops += [G.DEL] * (len(contig) - ctg_end)                                           # :652
    head_ins = 0                                                                       # :611-620, :655
    while head_ins < len(ops) and ops[head_ins] == G.INS:
        head_ins += 1
    out["head_ins"] = head_ins
    target = next((k for k, b in enumerate(break_points) if ctg_start < b), None)      # :642
    if target is None:
        return out
    out["first_chunk"] = target
    alignments = [G.DEL] * (ctg_start - (break_points[target - 1] if target else 0))   # :647-650
    xpos, ypos = ctg_start, head_ins
    for q in range(head_ins, len(ops)):
        op = ops[q]
        xpos += op != G.INS
        ypos += op != G.DEL
        alignments.append(op)
        if xpos == break_points[target]:
            ylen = sum(o != G.DEL for o in alignments)
            mat = sum(o == G.MATCH for o in alignments)
            ok = 1.0 - sim_thr < mat / len(alignments)                                 # :671
            # (start, end) of :674-677 are the truncated stretch in the read's coordinates, :741-744
            position = start + seq_start + ypos - ylen if is_forward else (end - seq_start) - ypos
            out["nodes"][target] = dict(verdict=ACCEPTED if ok else REJECTED, mat_num=mat, ops_len=len(alignments), query_off=seq_start + ypos - ylen,
                                        query_len=ylen, position_from_start=position, ops=list(alignments))
            out["closed_by"][target] = "op" if q < real else "tail"
            target += 1
            alignments = []
        if target == n_chunks:                                                         # :688-691
            break
    assert target == n_chunks, "the stream reaches contig_len, so every chunk from first_chunk on closes"
    return out


def accepted_nodes(out, is_forward):
    """what encode_edge returns: the accepted nodes as (chunk index, node, seq), reversed for a reverse trial (:693-695)"""
    nodes = [(k, nd, out["window"][nd["query_off"]:nd["query_off"] + nd["query_len"]]) for k, nd in enumerate(out["nodes"]) if nd["verdict"] == ACCEPTED]
    return nodes if is_forward else nodes[::-1]


def fill_edges_by_new_chunks(nodes, seq_len, edges, tips):
    """:202-293 up to the calls of encode_edge.  nodes: (chunk, cluster, is_forward, position_from_start, seq length) each;
    edges: {((chunk, cluster, is_forward), (chunk, cluster, is_forward)): value}; tips: {(chunk, cluster, is_forward, is_tail):
    [value, ...]} -> [(insert index, start, end, direction, value)] in the reference's order"""
    out = []
    if nodes:                                                                          # head tip, :213-234
        chunk, cluster, forward, position, _ = nodes[0]
        start, end = 0, min(position + MARGIN, seq_len)
        for value in tips.get((chunk, cluster, forward, False), ()):
            out.append((0, start, end, True, value))
        for value in tips.get((chunk, cluster, not forward, True), ()):                # "Here is a bug", as it stands
            out.append((0, start, end, False, value))
    for idx in range(len(nodes) - 1):                                                  # :235-267
        a, b = nodes[idx], nodes[idx + 1]
        start = min(max(a[3] + a[4], MARGIN) - MARGIN, seq_len)
        end = min(b[3] + MARGIN, seq_len)
        forward_key = ((a[0], a[1], a[2]), (b[0], b[1], b[2]))
        reverse_key = ((b[0], b[1], not b[2]), (a[0], a[1], not a[2]))
        if forward_key in edges:
            value, direction = edges[forward_key], True
        elif reverse_key in edges:
            value, direction = edges[reverse_key], False
        else:
            continue
        if end <= start:
            continue
        out.append((idx + 1, start, end, direction, value))
    if nodes:                                                                          # tail tip, :269-291
        chunk, cluster, forward, position, length = nodes[-1]
        idx = len(nodes)
        start, end = min(position + length, seq_len), seq_len
        start, end = max(start - MARGIN, 0), min(end + MARGIN, seq_len)
        for value in tips.get((chunk, cluster, forward, True), ()):
            out.append((idx + 1, start, end, True, value))
        for value in tips.get((chunk, cluster, not forward, False), ()):
            out.append((idx + 1, start, end, False, value))
    return out
