"""An independent restatement, in plain Python, of what jtk_lc_node_errors / jtk_lc_error_quantile / jtk_lc_estimate_error_rate /
jtk_lc_purge_diverged compute, written from the behaviour of the reference (Node::recover, definitions/src/lib.rs:773-813;
calc_sim_thr, determine_chunks.rs:796-823; estimate_error_rate.rs:37-133; purge_diverged_nodes, purge_diverged.rs:238-322;
nodes_to_encoded_read, encode/mod.rs:94-119 with Edge::from_nodes, definitions/src/lib.rs:647-669).

A data set is the dict of the squish and correction tests -- reads = [dict(id, nodes = [dict(chunk, cluster, is_forward,
posterior)])], chunks = [dict(id, cluster_num, copy_num, score)] -- extended by each node's `seq`, `cigar` ("12M1D3I"; or `ops`, a
list of per-base codes 0 Match / 1 Mismatch / 2 Ins / 3 Del, where a test needs a code no cigar can hold) and
`position_from_start`, each read's raw `seq`, and each chunk's `seq`.

Every sum is an explicit left-to-right loop over Python floats: no builtin sum (compensated since Python 3.12), no math.fsum, no
numpy reduction (pairwise).  Where the reference panics, ReferencePanic is raised; it carries the status the entry points return
there."""
import math
import re
import struct

import numpy as np

INVALID_ARG, OPS_MISMATCH, CHUNK_FAILED = -1, -5, -6
NAN = struct.unpack("<d", struct.pack("<Q", 0x7ff8000000000000))[0]     # a read without nodes: 0 / 0
THR = 0.1                                                                # purge_diverged.rs:40
MAX_ITER = 100000
NODE_DT = np.dtype([("chunk", "<u8"), ("cluster", "<u8"), ("is_forward", "<u4"), ("post_len", "<u4"), ("post_off", "<u8")])
CHUNK_DT = np.dtype([("id", "<u8"), ("cluster_num", "<u4"), ("copy_num", "<u4"), ("score", "<f8")])


class ReferencePanic(Exception):
    def __init__(self, status, why):
        super().__init__(why)
        self.status = status


# ---- Node::recover, counted

def runs_of(node):
    """the node's cigar as [(code, length)]: from `cigar` (M -> 0, I -> 2, D -> 3) or from the per-base list `ops`"""
    if "ops" in node:
        out = []
        for code in node["ops"]:
            if out and out[-1][0] == code:
                out[-1][1] += 1
            else:
                out.append([int(code), 1])
        return [(c, n) for c, n in out]
    return [({"M": 0, "I": 2, "D": 3}[k], int(n)) for n, k in re.findall(r"(\d+)([MDI])", node["cigar"])]


def per_base_ops(node):
    return [c for c, n in runs_of(node) for _ in range(n)]


def query_length(node):
    n = 0
    for c, length in runs_of(node):
        if c in (0, 1, 2):
            n += length
    return n


def column_counts(node, chunk_seq):
    """(columns that are not '|', columns) of recover's alignment row; ReferencePanic where a slice runs past its sequence"""
    read, tmpl = node["seq"].upper(), chunk_seq.upper()
    q = r = errs = cols = 0
    for code, length in runs_of(node):
        if code > 3:
            raise ReferencePanic(INVALID_ARG, "no such op")
        if code in (0, 1):
            if q + length > len(read) or r + length > len(tmpl):
                raise ReferencePanic(OPS_MISMATCH, "Match past the end")
            for i in range(length):
                if read[q + i] != tmpl[r + i]:
                    errs += 1
            q += length
            r += length
        elif code == 3:
            if r + length > len(tmpl):
                raise ReferencePanic(OPS_MISMATCH, "Del past the end")
            errs += length
            r += length
        else:
            if q + length > len(read):
                raise ReferencePanic(OPS_MISMATCH, "Ins past the end")
            errs += length
            q += length
        cols += length
    if cols == 0:
        raise ReferencePanic(CHUNK_FAILED, "0 / 0")
    return errs, cols


def node_errors(ds):
    """(err_num, err_len, status) per node in read order, as jtk_lc_node_errors reports them"""
    seq_of = {c["id"]: c["seq"] for c in ds["chunks"]}
    num, length, status = [], [], []
    for read in ds["reads"]:
        for node in read["nodes"]:
            try:
                if node["chunk"] not in seq_of:
                    raise ReferencePanic(CHUNK_FAILED, "chunks[&node.chunk]")
                e, c = column_counts(node, seq_of[node["chunk"]])
                st = 0
            except ReferencePanic as p:
                e, c, st = 0, 0, p.status
            num.append(e)
            length.append(c)
            status.append(st)
    return num, length, status


# ---- calc_sim_thr

def error_quantile(num, length, q):
    if len(num) == 0 or not 0.0 <= q <= 1.0 or any(n == 0 for n in length):
        raise ReferencePanic(INVALID_ARG, "calc_sim_thr")
    rates = sorted(a / b for a, b in zip(num, length))
    return rates[min(int(math.floor(len(rates) * q)), len(rates) - 1)]


# ---- estimate_error_rate

def _residual(errors, read_err, chunk_err, ids, reverse):
    total = 0.0
    for r in (reversed(range(len(errors))) if reverse else range(len(errors))):
        data = 0.0
        for chunk, cluster, error in (reversed(errors[r]) if reverse else errors[r]):
            x = error - read_err[r] - chunk_err[chunk][cluster]
            data = data + x * x
        total = total + data
    reg = 0.0
    flat = [x for cid in ids for x in chunk_err[cid]]
    for x in (reversed(flat) if reverse else flat):
        reg = reg + x * x
    return total + reg


def estimate_error_rate(ds, num, length, fallback, reverse=False):
    """-> dict(read_err per read, chunk_err {chunk id: [rate per cluster]}, median, n_iter).  reverse=True adds every slot's
    and every residual's terms in the opposite order: not the reference, but what a test compares with to see that order shows"""
    if len(num) == 0 or any(n == 0 for n in length):
        raise ReferencePanic(INVALID_ARG, "the median of nothing / a rate of 0 / 0")
    k_of = {c["id"]: c["cluster_num"] for c in ds["chunks"]}
    ids = sorted(k_of)                                           # the reference's tables are indexed by chunk id
    errors, e = [], 0
    for read in ds["reads"]:
        row = []
        for node in read["nodes"]:
            if node["chunk"] not in k_of or not node["cluster"] < k_of[node["chunk"]]:
                raise ReferencePanic(CHUNK_FAILED, "counts[chunk][cluster]")
            row.append((node["chunk"], node["cluster"], num[e] / length[e]))
            e += 1
        errors.append(row)
    counts = {cid: [0] * k_of[cid] for cid in ids}
    for row in errors:
        for chunk, cluster, _ in row:
            counts[chunk][cluster] += 1
    read_err = [fallback] * len(errors)
    chunk_err = {cid: [0.0] * k_of[cid] for cid in ids}
    current = _residual(errors, read_err, chunk_err, ids, reverse)
    n_iter = 0
    while True:
        if n_iter == MAX_ITER:
            raise ReferencePanic(CHUNK_FAILED, "no convergence")
        n_iter += 1
        chunk_err = {cid: [0.0] * k_of[cid] for cid in ids}
        for r in (reversed(range(len(errors))) if reverse else range(len(errors))):
            for chunk, cluster, error in (reversed(errors[r]) if reverse else errors[r]):
                chunk_err[chunk][cluster] = chunk_err[chunk][cluster] + (error - read_err[r])
        for cid in ids:
            for cl in range(k_of[cid]):
                s = chunk_err[cid][cl]
                chunk_err[cid][cl] = (s if s > 0.0 else 0.0) / (counts[cid][cl] + 0.1)
        for r, row in enumerate(errors):
            s = 0.0
            for chunk, cluster, error in (reversed(row) if reverse else row):
                s = s + (error - chunk_err[chunk][cluster])
            read_err[r] = s / len(row) if row else NAN
        resid = _residual(errors, read_err, chunk_err, ids, reverse)
        if abs(current - resid) < 0.00001:
            break
        current = resid
    squares = []
    for r, row in enumerate(errors):
        for chunk, cluster, error in row:
            x = error - (chunk_err[chunk][cluster] + read_err[r])
            squares.append(x * x)
    squares.sort()
    return dict(read_err=read_err, chunk_err=chunk_err, median=math.sqrt(squares[len(squares) // 2]), n_iter=n_iter)


def flat_chunk_err(ds, chunk_err):
    """the rates in the entry points' layout: chunks[] order, with the offsets"""
    flat, off = [], [0]
    for c in ds["chunks"]:
        flat.extend(chunk_err[c["id"]])
        off.append(len(flat))
    return flat, off


# ---- purge_diverged_nodes

def purge(ds, thr=THR):
    """what jtk_lc_purge_diverged returns: dict(status, ...) with every output list in the entry point's layout"""
    try:
        n_nodes = 0
        for read in ds["reads"]:
            n_nodes += len(read["nodes"])
        if n_nodes == 0:
            raise ReferencePanic(INVALID_ARG, "calc_sim_thr on no node")
        num, length, status = node_errors(ds)
        if any(status):
            raise ReferencePanic(CHUNK_FAILED, "recover")
        fallback = error_quantile(num, length, 0.5)
        fit = estimate_error_rate(ds, num, length, fallback)
        k_of = {c["id"]: c["cluster_num"] for c in ds["chunks"]}
        flags = {}
        for cid, rates in fit["chunk_err"].items():
            xs = [thr < x for x in rates]
            flags[cid] = [False] * len(xs) if all(xs) else xs
        keep, cluster, touched, post_keep = [], [], [], []
        for read in ds["reads"]:
            for node in read["nodes"]:
                info = flags[node["chunk"]]
                kept = not info[node["cluster"]]
                hit = kept and any(info)
                if hit and len(node["posterior"]) > k_of[node["chunk"]]:
                    raise ReferencePanic(CHUNK_FAILED, "cluster_info[i - 1]")
                keep.append(int(kept))
                cluster.append(node["cluster"] - len([1 for x in info[:node["cluster"]] if x]) if kept else node["cluster"])
                touched.append(int(hit))
                post_keep.extend(int(not info[i]) if hit else 1 for i in range(len(node["posterior"])))
    except ReferencePanic as p:
        return dict(status=p.status)
    flat, off = flat_chunk_err(ds, fit["chunk_err"])
    return dict(status=0, fallback=fallback, diverged=[int(x) for c in ds["chunks"] for x in flags[c["id"]]], chunk_err_off=off,
                cluster_num=[c["cluster_num"] - len([1 for x in flags[c["id"]] if x]) for c in ds["chunks"]], keep=keep, cluster=cluster,
                touched=touched, post_keep=post_keep, purged=sorted(cid for cid, xs in flags.items() if any(xs)),
                read_err=fit["read_err"], chunk_err=flat, median=fit["median"], n_iter=fit["n_iter"])


def nodes_to_encoded_read(rid, nodes, seq):
    """encode::nodes_to_encoded_read with Edge::from_nodes: the gaps and edges of a read from its nodes and its raw sequence"""
    if not nodes:
        return None
    seq = seq.upper()
    last = nodes[-1]
    edges = []
    for a, b in zip(nodes, nodes[1:]):
        end, start = a["position_from_start"] + query_length(a), b["position_from_start"]
        edges.append({"from": a["chunk"], "to": b["chunk"], "offset": start - end, "label": "" if start <= end else seq[:start][end:]})
    return dict(id=rid, original_length=len(seq), leading_gap=seq[:nodes[0]["position_from_start"]],
                trailing_gap=seq[last["position_from_start"] + query_length(last):], edges=edges, nodes=nodes, seq=seq)


def written_back(ds, res):
    """the data set after purge_diverged_nodes: `res` (of `purge`, or an entry point's outputs under the same keys) applied as
    include/jtk_lc.h tells the caller to, the reads left without nodes dropped, every other read rebuilt from its nodes"""
    new_k = {c["id"]: int(k) for c, k in zip(ds["chunks"], res["cluster_num"])}
    out = dict(reads=[], chunks=[dict(c, cluster_num=new_k[c["id"]]) for c in ds["chunks"]], coverage=ds.get("coverage", 10.0))
    e = p = 0
    for read in ds["reads"]:
        nodes = []
        for n in read["nodes"]:
            m = len(n["posterior"])
            if res["keep"][e]:
                n = dict(n, cluster=int(res["cluster"][e]), posterior=[x for i, x in enumerate(n["posterior"]) if res["post_keep"][p + i]])
                nodes.append(n)
            e += 1
            p += m
        rebuilt = nodes_to_encoded_read(read["id"], nodes, read["seq"])
        if rebuilt is not None:
            out["reads"].append(rebuilt)
    return out


# ---- the flattened form of the entry points

def flatten(ds):
    nodes, node_off, n_post = [], [0], 0
    seq, seq_off, ops, ops_off, tmpl, tmpl_off = [], [0], [], [0], [], [0]
    for read in ds["reads"]:
        for n in read["nodes"]:
            nodes.append((n["chunk"], n["cluster"], 1 if n["is_forward"] else 0, len(n["posterior"]), n_post))
            n_post += len(n["posterior"])
            seq.append(n["seq"])
            seq_off.append(seq_off[-1] + len(n["seq"]))
            o = per_base_ops(n)
            ops.extend(o)
            ops_off.append(len(ops))
        node_off.append(len(nodes))
    for c in ds["chunks"]:
        tmpl.append(c["seq"])
        tmpl_off.append(tmpl_off[-1] + len(c["seq"]))
    u8 = lambda parts: np.frombuffer("".join(parts).encode("ascii"), dtype=np.uint8).copy()   # noqa: E731
    return dict(node_off=np.array(node_off, dtype=np.uint64), nodes=np.array(nodes, dtype=NODE_DT), n_post=n_post,
                chunks=np.array([(c["id"], c["cluster_num"], c["copy_num"], c["score"]) for c in ds["chunks"]], dtype=CHUNK_DT),
                seqs=(u8(seq), np.array(seq_off, dtype=np.uint64), np.array(ops, dtype=np.uint8), np.array(ops_off, dtype=np.uint64),
                      u8(tmpl), np.array(tmpl_off, dtype=np.uint64)))


def unflatten(node_off, nodes, n_post, chunks, seqs):
    """the data set behind the arrays of an entry point (posterior VALUES are not part of them: zeros of the right length)"""
    sb, so, ob, oo, tb, to = seqs
    text = lambda a, b, e: bytes(a[int(b):int(e)]).decode("ascii")                              # noqa: E731
    reads = []
    for r in range(len(node_off) - 1):
        ns = []
        for e in range(int(node_off[r]), int(node_off[r + 1])):
            n = nodes[e]
            ns.append(dict(chunk=int(n["chunk"]), cluster=int(n["cluster"]), is_forward=bool(n["is_forward"]),
                           posterior=[0.0] * int(n["post_len"]), seq=text(sb, so[e], so[e + 1]),
                           ops=[int(x) for x in ob[int(oo[e]):int(oo[e + 1])]]))
        reads.append(dict(id=r, nodes=ns))
    return dict(reads=reads, chunks=[dict(id=int(c["id"]), cluster_num=int(c["cluster_num"]), copy_num=int(c["copy_num"]),
                                          score=float(c["score"]), seq=text(tb, to[i], to[i + 1])) for i, c in enumerate(chunks)])
