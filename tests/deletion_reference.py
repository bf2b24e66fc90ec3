"""`ds.correct_deletion` without re-clustering (haplotyper/src/encode/deletion_fill.rs:36-44, 136-367 and
haplotyper/src/purge_diverged.rs:49-187), restated in plain Python on a JTK `DataSet` as parsed from JSON, composed from the
references of the primitives -- nothing of the library is used:

    tests/fill_reference.py       get_pileup, ins_thr, check_insertion_head / _tail
    tests/encode_reference.py     try_encoding_head / _tail, encode_node (guided passes: DESIGN section 4, not kiley)
    tests/align_reference.py + tests/gpolish_reference.py    take_consensus_sequence (polish: DESIGN section 4, not kiley)
    tests/purge_reference.py      Node::recover's error counts, calc_sim_thr, estimate_error_rate, nodes_to_encoded_read
    tests/settle_reference.py     the list surgery of correct_deletion_error, del_size

Where the reference iterates a HashMap (the pick among trials of equal score) the order is the library's stated one: that of
jtk_lc_fill_candidates' output."""
import copy
import math
import re

import numpy as np

import align_reference as AR
import encode_reference as E
import fill_reference as F
import gpolish_reference as GP
import purge_reference as PR
import settle_reference as S

OUTER_LOOP, INNER_LOOP = 3, 12
THR = 10.0                     # deletion_fill.rs:369
TAKE_THR = 0.999               # determine_chunks.rs:29
MAX_ALLOWED_GAP = 100          # haplotyper/src/lib.rs:43
BAND_FRAC = {"CCS": 0.01, "ONT": 0.03, "CLR": 0.05, "None": 0.05}


def runs(cigar):
    return [({"M": "M", "I": "I", "D": "D"}[k], int(n)) for n, k in re.findall(r"(\d+)([MDI])", cigar)]


def cigar_of(ops):
    """kiley_op_to_ops + Display: Match and Mismatch merge into M"""
    out = []
    for op in ops:
        k = "M" if op <= 1 else "I" if op == 2 else "D"
        if out and out[-1][0] == k:
            out[-1][1] += 1
        else:
            out.append([k, 1])
    return "".join("%d%s" % (n, k) for k, n in out)


def settle_node(n):
    cigar = runs(n["cigar"])
    return dict(chunk=n["chunk"], pos=n["position_from_start"], fwd=bool(n["is_forward"]), qlen=S.query_bases(cigar), cigar=cigar)


def as_purge_ds(ds):
    raw = {r["id"]: r["seq"] for r in ds["raw_reads"]}
    return {"reads": [{"id": r["id"], "seq": raw[r["id"]], "nodes": r["nodes"]} for r in ds["encoded_reads"]], "chunks": ds["selected_chunks"]}


def take_consensus_sequence(ds):
    """:260-285"""
    chunk_seq = {c["id"]: AR.seq(c["seq"].upper()) for c in ds["selected_chunks"]}
    bucket = {}
    for read in ds["encoded_reads"]:
        for n in read["nodes"]:
            bucket.setdefault((n["chunk"], n["cluster"]), []).append(AR.seq(n["seq"].upper()))
    out = {}
    for (cid, cl), seqs in bucket.items():
        if cl == 0:
            out[cid, cl] = bytes(chunk_seq[cid])
            continue
        ops = [AR.align(chunk_seq[cid], s)[0] for s in seqs]
        out[cid, cl] = bytes(GP.polish(chunk_seq[cid], seqs, ops, math.ceil(len(chunk_seq[cid]) * BAND_FRAC[ds["read_type"]]))[0])
    return out


def rebuild(read, raw_seq):
    got = PR.nodes_to_encoded_read(read["id"], read["nodes"], raw_seq)
    for key in ("original_length", "leading_gap", "trailing_gap", "edges"):
        read[key] = got[key]


def fill_round(ds, state, consensi, read_err, chunk_err, stddev):
    """filling_until's loop body (:192-204) = correct_deletion_error (:301-367) for every live read"""
    reads = ds["encoded_reads"]
    raw = {r["id"]: r["seq"] for r in ds["raw_reads"]}
    chunk_of = {c["id"]: c for c in ds["selected_chunks"]}
    skeleton_input = [[(n["chunk"], n["cluster"], int(bool(n["is_forward"])), PR.query_length(n), n["position_from_start"]) for n in r["nodes"]]
                      for r in reads]
    target = [bool(r["nodes"]) and state[i]["alive"] for i, r in enumerate(reads)]
    found = F.fill_candidates(skeleton_input, target)      # every read sees the skeletons as they stand when the round begins
    new_ids = []
    for r, read in enumerate(reads):
        if not target[r]:
            continue
        ft, nodes, seq = state[r], read["nodes"], raw[read["id"]]
        cands = found["cands"][found["cand_off"][r]:found["cand_off"][r + 1]]
        inserts = []
        for idx in range(len(nodes) + 1):
            for side in (0, 1):
                cand = [(c[3], c[4], bool(c[5]), c[7]) for c in cands if c[1] == idx and c[2] == side]
                cand = [c for c in cand if (idx, c[:3]) not in ft["failed"]]
                nxt = (nodes[idx]["chunk"], nodes[idx]["position_from_start"]) if idx < len(nodes) else None
                best = None
                for k, start, end in E.fill_trials(side, cand, len(seq), nxt,
                                                   lambda u, c: len(consensi[u, c]) if u in chunk_of and (u, c) in consensi else None):
                    uid, cluster, forward, _ = cand[k]
                    bound = (read_err[read["id"]] + chunk_err[uid][cluster]) + THR * stddev
                    res = E.encode_node(seq.encode("ascii"), start, end, forward, consensi[uid, cluster],
                                        chunk_of[uid]["seq"].upper().encode("ascii"), bound)
                    if res["verdict"] == E.ACCEPTED and (best is None or best[0]["score"] <= res["score"]):
                        best = (res, uid, cluster, forward)
                if best is None:
                    ft["failed"].update((idx, c[:3]) for c in cand)
                    continue
                res, uid, cluster, forward = best
                k = chunk_of[uid]["cluster_num"]
                inserts.append({"position_from_start": res["position_from_start"], "chunk": uid, "cluster": cluster,
                                "seq": res["query"].decode("ascii"), "is_forward": forward, "cigar": cigar_of(res["ops"]),
                                "posterior": [math.log(1.0 / max(k, 1))] * k})
        ft["alive"] = bool(inserts)
        if inserts:
            ft["failed"] = set()
            new_ids += [n["chunk"] for n in inserts]
            nodes = nodes + inserts
            kept = S.settle_read([settle_node(n) for n in nodes], S.BY_CHUNK_POS)
            read["nodes"] = [nodes[i] for i in kept]
            rebuild(read, raw[read["id"]])
    return new_ids


def correct_chunk_deletion(ds, sim_thr=None, stddev_of_error=None):
    assert all(r["nodes"] for r in ds["encoded_reads"])
    consensi = take_consensus_sequence(ds)
    pds = as_purge_ds(ds)
    num, length, status = PR.node_errors(pds)
    assert not any(status)
    fallback = sim_thr if sim_thr is not None else PR.error_quantile(num, length, TAKE_THR)
    fit = PR.estimate_error_rate(pds, num, length, fallback)
    stddev = stddev_of_error if stddev_of_error is not None else fit["median"]
    read_err = {r["id"]: fit["read_err"][i] for i, r in enumerate(ds["encoded_reads"])}
    state = [{"alive": True, "failed": set()} for _ in ds["encoded_reads"]]
    found = set()
    for _ in range(OUTER_LOOP):
        for st in state:
            st["alive"], st["failed"] = True, set()
        is_updated = True
        for i in range(INNER_LOOP):
            prev = sum(len(r["nodes"]) for r in ds["encoded_reads"])
            found.update(fill_round(ds, state, consensi, read_err, fit["chunk_err"], stddev))
            after = sum(len(r["nodes"]) for r in ds["encoded_reads"])
            if after == prev and i == 0:
                is_updated = False
                break
            if after == prev:
                break
        if not is_updated:
            break
    return sorted(found)


COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}


def original_seq(node):
    return node["seq"] if node["is_forward"] else "".join(COMPLEMENT[b] for b in reversed(node["seq"].upper()))


def remove(read, i):
    """EncodedRead::remove (definitions/src/lib.rs:540-603), on lists of characters as the reference works on Vec<u8>"""
    nodes, edges = read["nodes"], read["edges"]
    assert i < len(nodes) and len(nodes) == len(edges) + 1
    length = len(nodes)
    removed_node = nodes.pop(i)
    if not nodes:
        assert not edges
        read["leading_gap"] = read["leading_gap"] + original_seq(removed_node)
        return
    if i + 1 == length:
        removed_edge = edges.pop(i - 1)
        skip = -removed_edge["offset"] if removed_edge["offset"] < 0 else 0
        chain = list(removed_edge["label"]) + list(original_seq(removed_node)) + list(read["trailing_gap"])
        read["trailing_gap"] = "".join(chain[skip:])
    elif i == 0:
        removed_edge = edges.pop(i)
        gap = list(read["leading_gap"]) + list(original_seq(removed_node)) + list(removed_edge["label"])
        for _ in range(max(-removed_edge["offset"], 0)):
            if gap:
                gap.pop()
        read["leading_gap"] = "".join(gap)
    else:
        removed_edge = edges.pop(i)
        edge = list(edges[i - 1]["label"]) + list(original_seq(removed_node)) + list(removed_edge["label"])
        if edges[i - 1]["offset"] < 0:
            edge.reverse()
            for _ in range(-edges[i - 1]["offset"]):
                if edge:
                    edge.pop()
            edge.reverse()
        if removed_edge["offset"] < 0:
            for _ in range(-removed_edge["offset"]):
                if edge:
                    edge.pop()
        edges[i - 1]["to"] = removed_edge["to"]
        edges[i - 1]["label"] = "".join(edge)
        edges[i - 1]["offset"] += len(removed_node["seq"]) + removed_edge["offset"]
    assert len(nodes) == len(edges) + 1


def as_usize(x):
    return x % (1 << 64)


def purge_largeindel(ds, indel_size, occupy_fraction, compress):
    """purge_large_deletion_nodes + the retain of :52"""
    distr = {}
    copy_num = {c["id"]: c["copy_num"] for c in ds["selected_chunks"]}
    for read in ds["encoded_reads"]:
        for idx, node in enumerate(read["nodes"]):
            key = (node["chunk"], 0) if compress else (node["chunk"], node["cluster"])
            distr.setdefault(key, []).append((read["id"], idx, S.del_size(runs(node["cigar"]))))
    counts = {}                                                          # misc::update_coverage, misc.rs:394-407
    for read in ds["encoded_reads"]:
        for node in read["nodes"]:
            counts[node["chunk"]] = counts.get(node["chunk"], 0) + 1
    if not (isinstance(ds["coverage"], dict) and "Protected" in ds["coverage"]):
        cov = sorted(counts.values())
        ds["coverage"] = {"Estimated": cov[len(cov) // 2] / 2.0}
    hap_coverage = next(iter(ds["coverage"].values()))
    accept_size = int(math.ceil(indel_size * 0.5))
    kept = {}
    for (chunk, cluster), d in distr.items():
        if copy_num[chunk] <= 1:
            num = len([x for x in d if indel_size < x[2]])
            upper_thr = int(math.ceil(len(d) * (1.0 - occupy_fraction / 2.0)))
            ok = 1 <= num < upper_thr
        else:
            lower_thr = max(int(math.floor(hap_coverage * occupy_fraction)), 0)
            upper_thr = int(math.ceil(max(len(d) - float(lower_thr), 0.0)))
            min_remove = len([x for x in d if indel_size < x[2]])
            max_remove = len([x for x in d if accept_size < x[2]])
            ok = lower_thr < min_remove and max_remove < upper_thr
            assert not ok or max_remove != 0                              # sum / max_remove
        if ok:
            kept[chunk, cluster] = [x for x in d if accept_size < as_usize(x[2])]
    bucket = {}
    for (chunk, cluster), d in kept.items():
        for rid, idx, _ in d:
            bucket.setdefault(rid, []).append((chunk, cluster, idx))
    for read in ds["encoded_reads"]:
        for chunk, cluster, idx in sorted(bucket.get(read["id"], []), key=lambda x: -x[2]):
            node = read["nodes"][idx]
            assert chunk == node["chunk"] and (compress or cluster == node["cluster"])
            remove(read, idx)
    ds["encoded_reads"] = [r for r in ds["encoded_reads"] if r["nodes"]]
    return sorted({k[0] for k in kept})


def correct_deletion(ds, sim_thr=None, stddev_of_error=None):
    """-> (the data set afterwards, the chunk ids of find_new_chunks ascending, the ids after each of the three steps)"""
    ds = copy.deepcopy(ds)
    steps = [correct_chunk_deletion(ds, sim_thr, stddev_of_error)]
    steps.append(purge_largeindel(ds, MAX_ALLOWED_GAP, 0.5, False))
    steps.append(purge_largeindel(ds, MAX_ALLOWED_GAP, 0.5, True))
    return ds, sorted(set(steps[0]) | set(steps[1]) | set(steps[2])), steps
