"""File-level drop-in for the stage: `DataSet` JSON in, `DataSet` JSON out.

JTK passes ONE JSON object between its stages (definitions/src/lib.rs:6-35; `jtk ... > x.encoded.json`,
`jtk local_clustering < x.encoded.json > x.clustered.json`, cli/src/pipeline.rs:153-159).  This module reads that
object, runs `LocalClustering::local_clustering{,_selected}` (haplotyper/src/local_clustering/mod.rs:17-83) through
the C ABI and writes the object back; every field the stage does not touch is passed through as parsed.

    python -m jtk_amd.dataset in.encoded.json out.clustered.json [--chunks id,id,...] [--device 0]

Wire format of the fields the stage reads or writes (serde derives of definitions/src/lib.rs):
  coverage         "NotAvailable" | {"Protected": f64} | {"Estimated": f64}          (:46-55, externally tagged enum)
  read_type        "CCS" | "CLR" | "ONT" | "None"                                     (:156-162)
  model_param      {"forward": HMMParam, "reverse": HMMParam}; HMMParam = 9 transition fields + mat_emit[16] +
                   ins_emit[20]                                                        (:95-126)
  selected_chunks  [{"id", "seq": "ACGT..", "cluster_num", "copy_num", "score"}]       (:403-415, DNASeq as a string)
  encoded_reads    [{.., "nodes": [{"position_from_start", "chunk", "cluster", "seq": "ACGT..", "is_forward",
                   "cigar": "10M2D3I", "posterior": [f64]}]}]                          (:672-683, Ops as a string :825-877)

Both preambles run on the device: `update_models_on_both_strands` (mod.rs:58, model_tune.rs:96-156: training pile-ups
picked here, ten rounds of polish + Baum-Welch in `jtk_lc_fit_model`; `--no-refit` keeps `model_param` as found in the
file) and the gains calibration (mod.rs:60, `jtk_lc_estimate_gains`).  This is the same host logic as the C++ mirror `csrc/host/local_clustering.hpp`; the two
are tested against each other (tests/test_dataset_json.py)."""
import argparse
import ctypes as C
import json
import math
import re
import sys
import time

import numpy as np

from . import api, ffi
from .batch import pack, pileup_sort

BAND_FRAC = {"CCS": 0.01, "ONT": 0.03, "CLR": 0.05, "None": 0.05}   # definitions/src/lib.rs:173-175

# Field names of the serde derives of definitions/src/lib.rs (no #[serde(rename/default/skip)] anywhere in that file, so
# the wire names are the Rust names and every field is required on input): struct -> fields in declaration order.
SCHEMA = {
    "DataSet": ("input_file", "masked_kmers", "coverage", "raw_reads", "hic_pairs", "selected_chunks", "encoded_reads",
                "hic_edges", "read_type", "model_param", "error_rate", "processed_stages"),                 # :6-34
    "ProcessedStage": ("stage_name", "arg"),                                                               # :38-43
    "HMMParamOnStrands": ("forward", "reverse"),                                                           # :95-99
    "HMMParam": ("mat_mat", "mat_ins", "mat_del", "ins_mat", "ins_ins", "ins_del", "del_mat", "del_ins", "del_del",
                 "mat_emit", "ins_emit"),                                                                  # :101-126
    "MaskInfo": ("k", "thr"),
    "RawRead": ("name", "desc", "id", "seq"),
    "HiCPair": ("pair1", "pair2", "pair_id", "seq1", "seq2"),
    "Chunk": ("id", "seq", "cluster_num", "copy_num", "score"),                                            # :403-415
    "EncodedRead": ("id", "original_length", "leading_gap", "trailing_gap", "edges", "nodes"),
    "Edge": ("from", "to", "offset", "label"),
    "Node": ("position_from_start", "chunk", "cluster", "seq", "is_forward", "cigar", "posterior"),        # :672-683
    "HiCEdge": ("pair_id", "pair1", "pair2"),
    "ErrorRate": ("del", "del_sd", "ins", "ins_sd", "mismatch", "mism_sd", "total", "total_sd"),           # :900-909
}
READ_TYPES = ("CCS", "CLR", "ONT", "None")                                                                 # :156-162


def _need(obj, struct, where):
    if not isinstance(obj, dict):
        raise ValueError(f"{where}: expected a {struct} object")
    missing = [k for k in SCHEMA[struct] if k not in obj]
    if missing:   # serde: "missing field `x`"
        raise ValueError(f"{where}: {struct} is missing field(s) {missing}")


def validate(ds):
    """What serde_json would reject on the way into `DataSet` (definitions/src/lib.rs): missing fields, a coverage or
    read type that is not one of the enum's variants.  Unknown extra fields are ignored, as serde does by default."""
    _need(ds, "DataSet", "dataset")
    _need(ds["masked_kmers"], "MaskInfo", "masked_kmers")
    cov = ds["coverage"]
    if not (cov == "NotAvailable" or (isinstance(cov, dict) and len(cov) == 1 and next(iter(cov)) in ("Protected", "Estimated"))):
        raise ValueError("coverage: expected \"NotAvailable\", {\"Protected\": x} or {\"Estimated\": x}")
    if ds["read_type"] not in READ_TYPES:
        raise ValueError(f"read_type: unknown variant {ds['read_type']!r}")
    _need(ds["model_param"], "HMMParamOnStrands", "model_param")
    for strand in ("forward", "reverse"):
        _need(ds["model_param"][strand], "HMMParam", f"model_param.{strand}")
    _need(ds["error_rate"], "ErrorRate", "error_rate")
    for i, st in enumerate(ds["processed_stages"]):
        _need(st, "ProcessedStage", f"processed_stages[{i}]")
    for i, r in enumerate(ds["raw_reads"]):
        _need(r, "RawRead", f"raw_reads[{i}]")
    for i, h in enumerate(ds["hic_pairs"]):
        _need(h, "HiCPair", f"hic_pairs[{i}]")
    for i, h in enumerate(ds["hic_edges"]):
        _need(h, "HiCEdge", f"hic_edges[{i}]")
    for i, c in enumerate(ds["selected_chunks"]):
        _need(c, "Chunk", f"selected_chunks[{i}]")
    for i, r in enumerate(ds["encoded_reads"]):
        _need(r, "EncodedRead", f"encoded_reads[{i}]")
        for j, e in enumerate(r["edges"]):
            _need(e, "Edge", f"encoded_reads[{i}].edges[{j}]")
        for j, n in enumerate(r["nodes"]):
            _need(n, "Node", f"encoded_reads[{i}].nodes[{j}]")


_OP_RE = re.compile(r"(\d+)([MDI])")
_OP_CODE = {"M": ffi.OP_MATCH, "D": ffi.OP_DEL, "I": ffi.OP_INS}


def cigar_to_ops(cigar):
    """Ops::from_str (definitions/src/lib.rs:857-877) + ops_to_kiley (misc.rs:177-186): one op code per base."""
    out = []
    pos = 0
    for m in _OP_RE.finditer(cigar):
        if m.start() != pos:
            raise ValueError(f"bad cigar {cigar!r}")
        out.append(np.full(int(m.group(1)), _OP_CODE[m.group(2)], dtype=np.uint8))
        pos = m.end()
    if pos != len(cigar):
        raise ValueError(f"bad cigar {cigar!r}")
    return np.concatenate(out) if out else np.zeros(0, np.uint8)


def ops_to_cigar(ops):
    """kiley_op_to_ops (misc.rs:188-225; Match and Mismatch merge into one M run) + Display for Ops (:827-838)."""
    ops = np.asarray(ops, dtype=np.uint8)
    if len(ops) == 0:
        return ""
    kind = np.where(ops == ffi.OP_DEL, 1, np.where(ops == ffi.OP_INS, 2, 0))
    cut = np.flatnonzero(np.diff(kind)) + 1
    starts = np.concatenate([[0], cut])
    ends = np.concatenate([cut, [len(kind)]])
    return "".join(f"{e - s}{'MDI'[kind[s]]}" for s, e in zip(starts.tolist(), ends.tolist()))


def coverage_of(ds):
    cov = ds["coverage"]
    if isinstance(cov, dict):
        (tag, value), = cov.items()
        return tag, float(value)
    return cov, None


def update_coverage(ds):
    """misc.rs:394-407: unless protected, haploid coverage = median node count per chunk / 2."""
    tag, _ = coverage_of(ds)
    if tag == "Protected":
        return
    counts = {}
    for read in ds["encoded_reads"]:
        for node in read["nodes"]:
            counts[node["chunk"]] = counts.get(node["chunk"], 0) + 1
    if not counts:
        raise ValueError("update_coverage: no nodes")
    c = sorted(counts.values())
    ds["coverage"] = {"Estimated": c[len(c) // 2] / 2.0}


def _hmm(d):
    h = ffi.Hmm()
    for name in ("mat_mat", "mat_ins", "mat_del", "ins_mat", "ins_ins", "ins_del", "del_mat", "del_ins", "del_del"):
        setattr(h, name, float(d[name]))
    if len(d["mat_emit"]) != 16 or len(d["ins_emit"]) != 20:
        raise ValueError("HMMParam: mat_emit must have 16 and ins_emit 20 entries")
    for i, v in enumerate(d["mat_emit"]):
        h.mat_emit[i] = float(v)
    for i, v in enumerate(d["ins_emit"]):
        h.ins_emit[i] = float(v)
    return h


def _seq(s):
    return np.frombuffer(s.encode("ascii"), dtype=np.uint8)


def training_pileup_ids(piles, chunk_of):
    """truncate_bucket + the filter_map of estimate_model_parameters_on_both_strands (model_tune.rs:99-133): pile-ups whose
    coverage lies within 2 of the median, sorted by chunk id, the first TRAIN_UNIT_SIZE = 5 of them, and only THEN without
    those whose chunk is not among the selected chunks (a stray node can cost a training pile-up)."""
    covs = sorted(len(v) for v in piles.values())
    cov = covs[len(covs) // 2]                                       # select_nth_unstable(len / 2)
    first = sorted(cid for cid, v in piles.items() if max(cov, 2) - 2 <= len(v) < cov + 2)[:5]
    return [cid for cid in first if cid in chunk_of]


def update_models_on_both_strands(ds, device=0):
    """ModelFit::update_models_on_both_strands (model_tune.rs:20-25, :96-156): pick the training pile-ups (:99-118) and
    refit the model on both strands with jtk_lc_fit_model (TRAIN_ROUND = 10)."""
    piles = {c["id"]: [] for c in ds["selected_chunks"]}
    chunk_of = {c["id"]: c for c in ds["selected_chunks"]}
    for read in ds["encoded_reads"]:
        for node in read["nodes"]:
            piles.setdefault(node["chunk"], []).append(node)
    if not piles:
        raise ValueError("update_models_on_both_strands: no pile-up")
    ids = training_pileup_ids(piles, chunk_of)
    pile = [(cid, int(chunk_of[cid]["copy_num"]), _seq(chunk_of[cid]["seq"]), [_seq(n["seq"]) for n in piles[cid]],
             [cigar_to_ops(n["cigar"]) for n in piles[cid]], [1 if n["is_forward"] else 0 for n in piles[cid]], None)
            for cid in ids]
    if not pile or not any(p[3] for p in pile):
        raise ValueError("update_models_on_both_strands: no training pile-up")     # assert!, model_tune.rs:135
    params = ffi.Params()
    params.forward = _hmm(ds["model_param"]["forward"])
    params.reverse = _hmm(ds["model_param"]["reverse"])
    params.band_frac = BAND_FRAC[ds["read_type"]]
    f, r = api.fit_model(params, pack(pile), rounds=10, device=device)
    for name, h in (("forward", f), ("reverse", r)):
        d = {k: float(getattr(h, k)) for k in ("mat_mat", "mat_ins", "mat_del", "ins_mat", "ins_ins", "ins_del", "del_mat",
                                               "del_ins", "del_del")}
        d["mat_emit"] = [float(v) for v in h.mat_emit]
        d["ins_emit"] = [float(v) for v in h.ins_emit]
        ds["model_param"][name] = d


def normalize_local_clustering(ds):
    """normalize.rs:6-51 over every node of the dataset: clusters relabelled by descending size, posteriors permuted."""
    L = ffi.lib()
    piles = {}
    for read in ds["encoded_reads"]:
        for node in read["nodes"]:
            piles.setdefault(node["chunk"], []).append(node)
    cluster_num = {c["id"]: c["cluster_num"] for c in ds["selected_chunks"]}
    for cid, nodes in piles.items():
        if cid not in cluster_num:
            raise ValueError("normalize_local_clustering: node on an unknown chunk")
        k = cluster_num[cid]
        if any(len(n["posterior"]) != k for n in nodes):   # assert_eq!, normalize.rs:27-29
            raise ValueError("normalize_local_clustering: posterior length != cluster_num")
        if k == 0:
            continue
        label = np.array([n["cluster"] for n in nodes], dtype=np.uint32)
        post = np.array([n["posterior"] for n in nodes], dtype=np.float64).reshape(len(nodes), k)
        ffi.check(L.jtk_lc_normalize_pileup(len(nodes), k, ffi.u32p(label), ffi.f64p(post), k))
        for i, n in enumerate(nodes):
            n["cluster"] = int(label[i])
            n["posterior"] = post[i].tolist()


def local_clustering_selected(ds, selection, gains=None, device=0, failed=None, refit=True, record=None, trace=None):
    """mod.rs:56-83 on the parsed JSON object `ds` (modified in place).

    The reference panics when a chunk hits one of its asserts; here such a chunk (and a chunk of a shape this build does
    not take) comes back with a status.  With `failed` = a list, those chunks are left exactly as they were, their
    (chunk id, status) pairs are appended to it and every other chunk is written back; with `failed` = None the call
    raises like the reference, before touching `ds`.  `record` = a list: the reference's per-chunk RECORD lines (mod.rs:121,
    `debug!`) of the chunks that were written back are appended to it (api.record_rows).  `trace` = a list: the reference's
    trace! rows of every clustered chunk of copy number < 8 (TOTAL / CAND / PICK / DUMP / RANGE / LK / COUNTS,
    pseudo_mcmc.rs:122-127,236,250-262,467-472,539), chunk after chunk in chunk-id order (api.Session.trace: those chunks once
    more through a resident session -- a debugging aid, like the log level it mirrors)."""
    validate(ds)
    update_coverage(ds)                                                       # mod.rs:57
    if refit:
        update_models_on_both_strands(ds, device=device)                      # mod.rs:58
    params = ffi.Params()
    params.forward = _hmm(ds["model_param"]["forward"])                       # mod.rs:59
    params.reverse = _hmm(ds["model_param"]["reverse"])
    params.gains = gains if gains is not None else api.estimate_gains(params.forward, params.reverse, device=device)
    params.haploid_coverage = coverage_of(ds)[1]
    params.band_frac = BAND_FRAC[ds["read_type"]]
    # pileup_nodes (mod.rs:33-53): nodes of the selected chunks in order of appearance, then a stable sort by the
    # number of non-'|' alignment columns against the unpolished chunk sequence
    selection = set(selection)
    chunk_of = {c["id"]: c for c in ds["selected_chunks"] if c["id"] in selection}
    piles = {cid: [] for cid in chunk_of}
    for read in ds["encoded_reads"]:
        for node in read["nodes"]:
            if node["chunk"] in piles:
                piles[node["chunk"]].append(node)
    order = sorted(cid for cid, nodes in piles.items() if nodes)
    pileups = []
    for cid in order:
        chunk, nodes = chunk_of[cid], piles[cid]
        tmpl = _seq(chunk["seq"])
        reads = [_seq(n["seq"]) for n in nodes]
        ops = [cigar_to_ops(n["cigar"]) for n in nodes]
        perm = pileup_sort(tmpl, reads, ops)
        piles[cid] = [nodes[i] for i in perm]
        pileups.append((cid, int(chunk["copy_num"]), tmpl, [reads[i] for i in perm], [ops[i] for i in perm],
                        [1 if nodes[i]["is_forward"] else 0 for i in perm], None))
    batch = pack(pileups)
    out = api.cluster_chunks(params, batch, device=device,                    # the hot loop of mod.rs:64-72
                             raise_on_chunk_failure=failed is None)
    # update_by_clusterings (mod.rs:244-260) and the chunk write-back (mod.rs:74-81)
    for c, cid in enumerate(order):
        if int(out["result"][c]["status"]) != 0:
            failed.append((cid, int(out["result"][c]["status"])))
            continue
        k = int(out["result"][c]["cluster_num"])
        for r, node in zip(batch.chunk_reads(c), piles[cid]):
            node["posterior"] = out["log_post"][r, :k].tolist()
            node["cluster"] = int(out["label"][r])
            node["cigar"] = ops_to_cigar(out["ops_out"][int(out["ops_out_off"][r]):int(out["ops_out_off"][r + 1])])
        chunk = chunk_of[cid]
        chunk["seq"] = bytes(out["cons"][int(out["cons_off"][c]):int(out["cons_off"][c + 1])]).decode("ascii")
        chunk["score"] = float(out["result"][c]["score"])
        chunk["cluster_num"] = k
    if record is not None:                                                    # mod.rs:121
        rows = api.record_rows(batch.chunks["chunk_id"], batch.chunks["n_reads"], batch.chunks["tmpl_len"],
                               [int(batch.read_off[batch.chunk_reads(c).stop] - batch.read_off[batch.chunk_reads(c).start])
                                for c in range(batch.n_chunks)], batch.chunks["copy_num"], out["result"],
                               np.diff(out["cons_off"]).astype(np.int64), api.last_timing())
        record.extend(r for c, r in enumerate(rows) if int(out["result"][c]["status"]) == 0)
    if trace is not None:
        keep = [c for c in range(batch.n_chunks) if int(out["result"][c]["status"]) == 0 and int(batch.chunks["copy_num"][c]) < 8]
        if keep:
            with api.Session(params, batch.subset(keep), device=device) as sess:
                sess.run()
                for i in range(len(keep)):
                    trace.extend(sess.trace(i))
    normalize_local_clustering(ds)                                            # mod.rs:82
    return ds


def realign_selected(ds, selection, device=0):
    """What PolishChunk::consensus_chunk does per node once a chunk has its sequence (polish_chunks.rs:114-120): every node of
    the selected chunks is aligned globally to chunk.seq (jtk_lc_align_reads) and its cigar replaced.  For a file whose
    cigars no longer fit their chunks (a chunk was re-polished, a consensus written back)."""
    validate(ds)
    selection = set(selection)
    chunk_of = {c["id"]: c for c in ds["selected_chunks"] if c["id"] in selection}
    piles = {cid: [] for cid in chunk_of}
    for read in ds["encoded_reads"]:
        for node in read["nodes"]:
            if node["chunk"] in piles:
                piles[node["chunk"]].append(node)
    order = sorted(cid for cid, nodes in piles.items() if nodes)
    none = np.zeros(0, dtype=np.uint8)
    batch = pack([(cid, int(chunk_of[cid]["copy_num"]), _seq(chunk_of[cid]["seq"]), [_seq(n["seq"]) for n in piles[cid]],
                   [none] * len(piles[cid]), [1 if n["is_forward"] else 0 for n in piles[cid]], None) for cid in order])
    out = api.align_reads(batch, device=device)
    for c, cid in enumerate(order):
        for r, node in zip(batch.chunk_reads(c), piles[cid]):
            node["cigar"] = ops_to_cigar(out["ops"][int(out["ops_off"][r]):int(out["ops_off"][r + 1])])
    return ds


def local_clustering(ds, gains=None, device=0, failed=None, refit=True, record=None, trace=None):
    """mod.rs:23-26: every selected chunk."""
    validate(ds)
    return local_clustering_selected(ds, [c["id"] for c in ds["selected_chunks"]], gains=gains, device=device,
                                     failed=failed, refit=refit, record=record, trace=trace)


def correct_clustering_selected(ds, selection, device=0, min_gain=None):
    """AlignmentCorrection::correct_clustering_selected (phmm_likelihood_correction.rs:32-97) on the parsed JSON object `ds`
    (modified in place): jtk_lc_correct_clustering on the flattened nodes, then the write-back of :80-96.  min_gain defaults
    to estimate_minimum_gain(model) x PROTECT_FACTOR (:118) computed on the device."""
    tag, cov = coverage_of(ds)
    if cov is None:
        raise ValueError("correct_clustering: coverage is NotAvailable (the reference unwraps it, :154)")
    if min_gain is None:
        min_gain = api.estimate_minimum_gain(_hmm(ds["model_param"]["forward"]), _hmm(ds["model_param"]["reverse"]),
                                             device=device) * 1.0
    n_nodes = sum(len(r["nodes"]) for r in ds["encoded_reads"])
    nodes = np.zeros(n_nodes, dtype=ffi.CC_NODE_DT)
    node_off = np.zeros(len(ds["encoded_reads"]) + 1, dtype=np.uint64)
    read_id = np.zeros(len(ds["encoded_reads"]), dtype=np.uint64)
    post = []
    e = 0
    for r, read in enumerate(ds["encoded_reads"]):
        read_id[r] = read["id"]
        for node in read["nodes"]:
            nodes[e] = (node["chunk"], node["cluster"], 1 if node["is_forward"] else 0, len(node["posterior"]), len(post))
            post.extend(float(x) for x in node["posterior"])
            e += 1
        node_off[r + 1] = e
    chunks = np.zeros(len(ds["selected_chunks"]), dtype=ffi.CC_CHUNK_DT)
    for i, c in enumerate(ds["selected_chunks"]):
        chunks[i] = (c["id"], c["cluster_num"], c["copy_num"], c["score"])
    cluster, touched = api.correct_clustering(read_id, node_off, nodes, np.array(post, dtype=np.float64), chunks,
                                              sorted(int(x) for x in selection), cov, min_gain, device=device)
    cluster_num = {}
    for i, c in enumerate(ds["selected_chunks"]):
        c["cluster_num"] = int(chunks["cluster_num"][i])
        cluster_num[c["id"]] = c["cluster_num"]
    e = 0
    for read in ds["encoded_reads"]:
        for node in read["nodes"]:
            if touched[e]:                                           # :85-93
                node["cluster"] = int(cluster[e])
                node["posterior"] = [-10000.0] * cluster_num[node["chunk"]]
                node["posterior"][node["cluster"]] = 0.0
            e += 1


def squish_erroneous_clusters(ds, config=None, device=0):
    """SquishErroneousClusters::squish_erroneous_clusters (squish_erroneous_clusters.rs:44-60) on the parsed JSON object `ds`
    (modified in place): jtk_lc_squish_clusters on the flattened nodes, then the write-back of :47-58 -- a suspicious chunk
    gets cluster_num 1, its nodes cluster 0 and the posterior [0.0].  Returns the class per chunk id (ffi.REL_*)."""
    n_nodes = sum(len(r["nodes"]) for r in ds["encoded_reads"])
    nodes = np.zeros(n_nodes, dtype=ffi.CC_NODE_DT)
    node_off = np.zeros(len(ds["encoded_reads"]) + 1, dtype=np.uint64)
    post = []
    e = 0
    for r, read in enumerate(ds["encoded_reads"]):
        for node in read["nodes"]:
            nodes[e] = (node["chunk"], node["cluster"], 1 if node["is_forward"] else 0, len(node["posterior"]), len(post))
            post.extend(float(x) for x in node["posterior"])
            e += 1
        node_off[r + 1] = e
    chunks = np.zeros(len(ds["selected_chunks"]), dtype=ffi.CC_CHUNK_DT)
    for i, c in enumerate(ds["selected_chunks"]):
        chunks[i] = (c["id"], c["cluster_num"], c["copy_num"], c["score"])
    out = api.squish_clusters(node_off, nodes, np.array(post, dtype=np.float64), chunks, config=config, device=device)
    for i, c in enumerate(ds["selected_chunks"]):
        c["cluster_num"] = int(chunks["cluster_num"][i])
    e = 0
    for read in ds["encoded_reads"]:
        for node in read["nodes"]:
            if out["touched"][e]:                                    # :55-58
                node["cluster"] = int(out["cluster"][e])
                node["posterior"] = [0.0]
            e += 1
    return {c["id"]: int(k) for c, k in zip(ds["selected_chunks"], out["classes"])}


def query_length(node):
    """Node::query_length (definitions/src/lib.rs:754-762): the read bases the node's cigar consumes"""
    return sum(int(n) for n, k in _OP_RE.findall(node["cigar"]) if k in "MI")


def nodes_to_encoded_read(read, raw_seq):
    """encode::nodes_to_encoded_read (encode/mod.rs:94-119) with Edge::from_nodes (definitions/src/lib.rs:647-669): the read's
    gaps and edges rebuilt, in place, from its nodes and its raw read (upper-cased)."""
    seq, nodes = raw_seq.upper(), read["nodes"]
    last = nodes[-1]
    read["original_length"] = len(seq)
    read["leading_gap"] = seq[:nodes[0]["position_from_start"]]
    read["trailing_gap"] = seq[last["position_from_start"] + query_length(last):]
    read["edges"] = []
    for a, b in zip(nodes, nodes[1:]):
        end, start = a["position_from_start"] + query_length(a), b["position_from_start"]
        read["edges"].append({"from": a["chunk"], "to": b["chunk"], "offset": start - end,
                              "label": "" if start <= end else seq[:start][end:]})


def _flat_nodes(ds):
    """The data set as jtk_lc_node_errors / jtk_lc_purge_diverged take it: node_off, nodes (ffi.CC_NODE_DT), the length of the
    flat posterior array, chunks (ffi.CC_CHUNK_DT) and the sequences (node seqs, their offsets, per-base ops, their offsets, chunk
    seqs, their offsets)."""
    n_nodes = sum(len(r["nodes"]) for r in ds["encoded_reads"])
    nodes = np.zeros(n_nodes, dtype=ffi.CC_NODE_DT)
    node_off = np.zeros(len(ds["encoded_reads"]) + 1, dtype=np.uint64)
    seq_off, ops_off = np.zeros(n_nodes + 1, dtype=np.uint64), np.zeros(n_nodes + 1, dtype=np.uint64)
    seqs, ops = [], []
    e = n_post = 0
    for r, read in enumerate(ds["encoded_reads"]):
        for node in read["nodes"]:
            nodes[e] = (node["chunk"], node["cluster"], 1 if node["is_forward"] else 0, len(node["posterior"]), n_post)
            n_post += len(node["posterior"])
            seqs.append(_seq(node["seq"]))
            ops.append(cigar_to_ops(node["cigar"]))
            seq_off[e + 1] = seq_off[e] + len(seqs[-1])
            ops_off[e + 1] = ops_off[e] + len(ops[-1])
            e += 1
        node_off[r + 1] = e
    chunks = np.zeros(len(ds["selected_chunks"]), dtype=ffi.CC_CHUNK_DT)
    tmpls = [_seq(c["seq"]) for c in ds["selected_chunks"]]
    tmpl_off = np.zeros(len(tmpls) + 1, dtype=np.uint64)
    for i, c in enumerate(ds["selected_chunks"]):
        chunks[i] = (c["id"], c["cluster_num"], c["copy_num"], c["score"])
        tmpl_off[i + 1] = tmpl_off[i] + len(tmpls[i])
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.uint8)   # noqa: E731
    return node_off, nodes, n_post, chunks, (cat(seqs), seq_off, cat(ops), ops_off, cat(tmpls), tmpl_off)


def purge_diverged_nodes(ds, device=0, thr=0.1):
    """purge_diverged_nodes (purge_diverged.rs:238-322) on the parsed JSON object `ds` (modified in place):
    jtk_lc_purge_diverged on the flattened nodes with their sequences, then the write-back -- the flagged clusters' nodes go
    (:271-272), the other nodes of those chunks are renumbered and lose the flagged posterior entries (:311-322), reads left
    without nodes are dropped (:283), every other read gets its gaps and edges rebuilt from its raw read (:284-290).  Returns
    the ids of the chunks that lost a cluster, ascending: what `purge` (:42-48) hands to re_cluster, whose copy-number
    estimation (estimate_multiplicity, :210-212) is not part of this library."""
    node_off, nodes, n_post, chunks, seqs = _flat_nodes(ds)
    out = api.purge_diverged(node_off, nodes, n_post, chunks, seqs, thr=thr, device=device)
    for i, c in enumerate(ds["selected_chunks"]):
        c["cluster_num"] = int(chunks["cluster_num"][i])                     # :261-265
    raw = {r["id"]: r["seq"] for r in ds["raw_reads"]}
    e = p = 0
    reads = []
    for read in ds["encoded_reads"]:
        kept = []
        for node in read["nodes"]:
            m = len(node["posterior"])
            if out["keep"][e]:
                if out["touched"][e]:                                        # remove_diverged :311-322
                    node["cluster"] = int(out["cluster"][e])
                    node["posterior"] = [x for i, x in enumerate(node["posterior"]) if out["post_keep"][p + i]]
                kept.append(node)
            e += 1
            p += m
        if kept:                                                             # :283
            read["nodes"] = kept
            nodes_to_encoded_read(read, raw[read["id"]])                     # :284-290
            reads.append(read)
    ds["encoded_reads"] = reads
    return [int(x) for x in out["purged"]]


_COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}


def fill_candidates(ds, alive=None, device=0):
    """The candidate search of correct_deletion (encode/deletion_fill.rs:301-337: get_pileup, ins_thr, check_insertion_head /
    _tail) on encoded_reads[*].nodes, query_length taken from the cigar as Node::query_length does.  alive: None, or the ids of
    the reads to compute (the reference's `is_alive` filter).  Returns a list, one entry per computed read with a node, in read
    order: {"id", "ins_thr", "coverage": [n + 1], "candidates": [{"slot", "side": "head" | "tail", "chunk", "cluster",
    "is_forward", "count", "position"}]}.  What the reference does with a candidate (encode_node with kiley's infix_guided,
    remove_slippy_alignment, remove_overlapping_encoding) is not part of this: the data set is not changed."""
    reads = ds["encoded_reads"]
    node_off = np.zeros(len(reads) + 1, dtype=np.uint64)
    flat = []
    for r, read in enumerate(reads):
        flat += [(n["chunk"], n["cluster"], int(bool(n["is_forward"])), query_length(n), n["position_from_start"]) for n in read["nodes"]]
        node_off[r + 1] = len(flat)
    nodes = np.array(flat, dtype=ffi.FILL_NODE_DT) if flat else np.zeros(0, dtype=ffi.FILL_NODE_DT)
    ids = None if alive is None else set(alive)
    target = None if ids is None else np.array([read["id"] in ids for read in reads], dtype=np.uint8)
    out = api.fill_candidates(node_off, nodes, target=target, device=device)
    report = []
    for r, read in enumerate(reads):
        if not read["nodes"] or (target is not None and not target[r]):
            continue
        b = int(node_off[r]) + r
        cands = out["cands"][int(out["cand_off"][r]):int(out["cand_off"][r + 1])]
        report.append({"id": read["id"], "ins_thr": int(out["ins_thr"][r]),
                       "coverage": [int(x) for x in out["coverage"][b:b + len(read["nodes"]) + 1]],
                       "candidates": [{"slot": int(c["slot"]), "side": "tail" if c["side"] else "head", "chunk": int(c["chunk"]),
                                       "cluster": int(c["cluster"]), "is_forward": bool(c["is_forward"]), "count": int(c["count"]),
                                       "position": int(c["position"])} for c in cands]})
    return report


def take_consensus_sequence(ds, device=0):
    """take_consensus_sequence (encode/deletion_fill.rs:260-285): the consensus of every (chunk, cluster) that a node carries --
    the chunk's own sequence for cluster 0, otherwise the guided polish of the chunk's sequence with the nodes' sequences, band =
    read_type.band_width(len).  -> {(chunk, cluster): str}; the data set is not changed.  The polish is this build's own
    specification ("Guided polishing"): parity with kiley's polish_until_converge is not pinned."""
    chunk_seqs = {c["id"]: _seq(c["seq"].upper()) for c in ds["selected_chunks"]}
    nodes = [n for read in ds["encoded_reads"] for n in read["nodes"]]
    out = api.take_consensus(chunk_seqs, [n["chunk"] for n in nodes], [n["cluster"] for n in nodes], [_seq(n["seq"].upper()) for n in nodes],
                             BAND_FRAC[ds["read_type"]], device=device)
    return {key: bytes(seq).decode("ascii") for key, seq in out.items()}


def recover_raw_read(read):
    """EncodedRead::recover_raw_read (definitions/src/lib.rs:604-619): leading gap, then every node's original sequence
    (Node::original_seq :737-753: reverse complement of a reverse node; anything but ACGT panics) with the overlap of a
    negative edge offset popped and the edge label appended, the last node, the trailing gap."""
    def original(node):
        if node["is_forward"]:
            return node["seq"]
        try:
            return "".join(_COMPLEMENT[b] for b in reversed(node["seq"].upper()))
        except KeyError:
            raise ValueError("sanity_check: a reverse node holds a base outside ACGT (Node::original_seq panics)") from None
    out = list(read["leading_gap"])
    for node, edge in zip(read["nodes"], read["edges"]):
        if node["chunk"] != edge["from"]:
            raise ValueError(f"sanity_check: read {read['id']}: edge.from {edge['from']} after node of chunk {node['chunk']}")
        out.extend(original(node))
        drop = max(-int(edge["offset"]), 0)
        if drop:
            del out[max(len(out) - drop, 0):]
        out.extend(edge["label"])
    if read["nodes"]:
        out.extend(original(read["nodes"][-1]))
    out.extend(read["trailing_gap"])
    return "".join(out)


def sanity_check(ds):
    """DataSet::sanity_check (definitions/src/lib.rs:296-327 + encoded_reads_can_be_recovered :328-358), which
    correct_clustering ends with (phmm_likelihood_correction.rs:29).  Where the reference panics this raises ValueError."""
    ids = [c["id"] for c in ds["selected_chunks"]]
    chunks = set(ids)
    for read in ds["encoded_reads"]:
        for node in read["nodes"]:
            if node["chunk"] not in chunks:
                raise ValueError(f"sanity_check: read {read['id']} has a node on chunk {node['chunk']}, which is not selected")
    raw = {r["id"]: r["seq"] for r in ds["raw_reads"]}
    for read in ds["encoded_reads"]:
        if read["id"] not in raw:
            raise ValueError(f"sanity_check: encoded read {read['id']} has no raw read")
        orig, rec = raw[read["id"]].upper(), recover_raw_read(read).upper()
        if len(orig) != len(rec) or len(orig) != read["original_length"] or orig != rec:
            raise ValueError(f"sanity_check: encoded read {read['id']} does not recover its raw read "
                             f"({len(rec)} bases recovered, {len(orig)} raw, original_length {read['original_length']})")
    if len(chunks) != len(ids):
        raise ValueError("sanity_check: a chunk id occurs twice in selected_chunks")
    for c in ds["selected_chunks"]:
        if not c["cluster_num"] <= c["copy_num"]:
            raise ValueError(f"sanity_check: chunk {c['id']}: cluster_num {c['cluster_num']} > copy_num {c['copy_num']}")
    max_cl = {c["id"]: c["cluster_num"] for c in ds["selected_chunks"]}
    for read in ds["encoded_reads"]:
        for node in read["nodes"]:
            if not node["cluster"] <= max_cl[node["chunk"]]:
                raise ValueError(f"sanity_check: a node of chunk {node['chunk']} carries cluster {node['cluster']} of "
                                 f"{max_cl[node['chunk']]}")


def correct_clustering(ds, device=0, min_gain=None):
    """AlignmentCorrection::correct_clustering (phmm_likelihood_correction.rs:14-30): chunks no read visits are dropped,
    every chunk with more than one cluster is corrected, and the data set has to pass DataSet::sanity_check afterwards."""
    present = {n["chunk"] for r in ds["encoded_reads"] for n in r["nodes"]}
    ds["selected_chunks"] = [c for c in ds["selected_chunks"] if c["id"] in present]
    correct_clustering_selected(ds, [c["id"] for c in ds["selected_chunks"] if 1 < c["cluster_num"]], device=device,
                                min_gain=min_gain)
    sanity_check(ds)


OUTER_LOOP, INNER_LOOP = 3, 12     # encode/deletion_fill.rs:137,172
FILL_THR = 10.0                    # :369: the stddevs a trial's error rate may lie above its expectation
TAKE_THR = 0.999                   # determine_chunks.rs:29
MAX_ALLOWED_GAP = 100              # haplotyper/src/lib.rs:43
OCCUPY_FRACTION = 0.5              # deletion_fill.rs:39
ACCEPT_RATE = 0.5                  # purge_diverged.rs:63


_stage_timing = None     # scripts/settle_timing.py sets a dict here: wall seconds per primitive are added into it


class _Clock:
    """the wall time of one primitive's call, added into _stage_timing where that is a dict"""
    def __init__(self, key):
        self.key = key

    def __enter__(self):
        self.t0 = time.perf_counter()

    def __exit__(self, *exc):
        if _stage_timing is not None:
            _stage_timing[self.key] = _stage_timing.get(self.key, 0.0) + (time.perf_counter() - self.t0)


def _settle_arrays(reads):
    """api.settle_nodes' arrays for a list of node lists (JSON nodes)"""
    node_off = np.zeros(len(reads) + 1, dtype=np.uint64)
    flat = [n for nodes in reads for n in nodes]
    node_off[1:] = np.cumsum([len(nodes) for nodes in reads])
    rec = np.array([(n["chunk"], n["position_from_start"], 1 if n["is_forward"] else 0, query_length(n)) for n in flat],
                   dtype=ffi.SETTLE_NODE_DT) if flat else np.zeros(0, dtype=ffi.SETTLE_NODE_DT)
    ops = [cigar_to_ops(n["cigar"]) for n in flat]
    ops_off = np.zeros(len(flat) + 1, dtype=np.uint64)
    ops_off[1:] = np.cumsum([len(o) for o in ops])
    return node_off, rec, (np.concatenate(ops) if ops else np.zeros(0, np.uint8)), ops_off


def _fill_round(ds, state, consensi, read_err, chunk_err, stddev, device):
    """One pass of filling_until's loop body (deletion_fill.rs:192-204): correct_deletion_error (:301-367) for every live read,
    with one device call per primitive.  The reference goes through a read slot by slot, head before tail, and a slot's head
    candidates that fail are in `failed_trials` (:325) before the same slot's tail candidates are filtered (:328): the trials of
    every group are made and encoded at once here, and the pick then goes through the groups in that order and drops from a tail
    group what its head group has just failed.  Returns the chunk ids of the nodes that were inserted."""
    reads = ds["encoded_reads"]
    raw = {r["id"]: r["seq"] for r in ds["raw_reads"]}
    chunk_of = {c["id"]: c for c in ds["selected_chunks"]}
    live = [r for r, read in enumerate(reads) if read["nodes"] and state[r]["alive"]]                 # :196
    node_off = np.zeros(len(reads) + 1, dtype=np.uint64)
    flat = []
    for r, read in enumerate(reads):
        flat += [(n["chunk"], n["cluster"], int(bool(n["is_forward"])), query_length(n), n["position_from_start"]) for n in read["nodes"]]
        node_off[r + 1] = len(flat)
    target = np.zeros(len(reads), dtype=np.uint8)
    target[live] = 1
    with _Clock("fill_candidates"):
        found = api.fill_candidates(node_off, np.array(flat, dtype=ffi.FILL_NODE_DT) if flat else np.zeros(0, dtype=ffi.FILL_NODE_DT),
                                    target=target, device=device)
    # ---- the trials of every (read, slot, side): try_encoding_head / _tail up to encode_node (:370-446)
    cons_at, chunk_at, read_at = {}, {}, {}              # where a sequence lies in its flat buffer: key -> (offset, length)
    cons_parts, chunk_parts, read_parts = [], [], []

    def place(table, parts, key, text):
        if key not in table:
            last = table[next(reversed(table))] if table else (0, 0)
            table[key] = (last[0] + last[1], len(text))
            parts.append(_seq(text))
        return table[key]

    def cons_len_of(chunk, cluster):
        return len(consensi[chunk, cluster]) if chunk in chunk_of and (chunk, cluster) in consensi else None

    groups, trials, keys = [], [], []   # group: (read, slot, the candidates left after the failed-trial filter, first trial, trials)
    cand_of = []                        # per trial: its candidate's index in the group's list
    for r in live:
        read, nodes = reads[r], reads[r]["nodes"]
        seq = raw[read["id"]]
        by_slot = {}
        for c in found["cands"][int(found["cand_off"][r]):int(found["cand_off"][r + 1])]:
            by_slot.setdefault((int(c["slot"]), int(c["side"])), []).append(
                (int(c["chunk"]), int(c["cluster"]), bool(c["is_forward"]), int(c["position"])))
        for slot in range(len(nodes) + 1):
            for side in (0, 1):                                                                      # head, then tail (:317-336)
                left = [c for c in by_slot.get((slot, side), []) if (slot, c[:3]) not in state[r]["failed"]]   # :318, :328
                nxt = (nodes[slot]["chunk"], nodes[slot]["position_from_start"]) if slot < len(nodes) else None
                first = len(trials)
                for k, start, end in api.fill_trials(side, left, len(seq), nxt, cons_len_of):
                    chunk, cluster, forward, _ = left[k]
                    bound = (read_err[read["id"]] + chunk_err[chunk, cluster]) + FILL_THR * stddev   # :399-400, :441-442
                    cons_off, cons_len = place(cons_at, cons_parts, (chunk, cluster), consensi[chunk, cluster])
                    chunk_off, chunk_len = place(chunk_at, chunk_parts, chunk, chunk_of[chunk]["seq"].upper())
                    read_off, _ = place(read_at, read_parts, read["id"], seq)
                    trials.append((read_off, start, end, 1 if forward else 0, cons_len, cons_off, chunk_off, chunk_len, 0, bound))
                    keys.append((chunk, cluster))
                    cand_of.append(k)
                groups.append((r, slot, left, first, len(trials) - first))
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.uint8)   # noqa: E731
    read_bases = cat(read_parts)
    enc = None
    if trials:
        with _Clock("encode_nodes"):
            enc = api.encode_nodes(np.array(trials, dtype=ffi.ENCODE_TRIAL_DT), read_bases, cat(cons_parts), cat(chunk_parts), device=device,
                                   raise_on_trial_failure=False)
    # ---- the pick (:405, :445), the failed trials (:325, :335), the append (:344)
    inserts = {r: [] for r in live}
    for r, slot, left, first, n in groups:                 # per read in (slot, head, tail) order, as :316-337 goes
        gone = {k for k, c in enumerate(left) if (slot, c[:3]) in state[r]["failed"]}   # failed by this slot's head group (:325, :328)
        best = None
        for t in range(first, first + n):
            res = enc["result"][t]
            if cand_of[t] in gone or int(res["status"]) != 0 or int(res["verdict"]) != ffi.ENCODE_ACCEPTED:
                continue                                   # (a trial the device refuses is a trial that fails: encode_node's None)
            if best is None or int(enc["result"][best]["score"]) <= int(res["score"]):
                best = t                                   # max_by_key: of equal scores the last in candidate order
        if best is None:
            state[r]["failed"].update((slot, c[:3]) for k, c in enumerate(left) if k not in gone)
            continue
        res, trial = enc["result"][best], trials[best]
        window = api._oriented_window(read_bases, trial[0], trial[1], trial[2], trial[3])
        query = window[int(res["trim_head"]):len(window) - int(res["trim_tail"])]
        chunk, cluster = keys[best]
        k = int(chunk_of[chunk]["cluster_num"])
        inserts[r].append({"position_from_start": int(res["position_from_start"]), "chunk": chunk, "cluster": cluster,
                           "seq": query.decode("ascii"), "is_forward": bool(trial[3]),
                           "cigar": ops_to_cigar(enc["ops"][int(enc["ops_off"][best]):int(enc["ops_off"][best + 1])]),
                           "posterior": [math.log(1.0 / max(k, 1))] * k})                           # Node::new, lib.rs:723-731
    new_ids, changed = [], []
    for r in live:
        state[r]["alive"] = bool(inserts[r])                                                         # :341
        if inserts[r]:
            state[r]["failed"].clear()                                                               # revive, :343
            new_ids += [n["chunk"] for n in inserts[r]]
            reads[r]["nodes"].extend(inserts[r])
            changed.append(r)
    # ---- the settle step (:349-361), every changed read in one call
    if changed:
        node_off, rec, ops, ops_off = _settle_arrays([reads[r]["nodes"] for r in changed])
        with _Clock("settle_nodes"):
            out = api.settle_nodes(node_off, rec, ops, ops_off, mode=ffi.SETTLE_BY_CHUNK_POS, device=device)
        if out["rc"] != 0:
            raise ValueError("correct_deletion: a node without ops (the reference divides 0 by 0 in remove_overlapping_encoding)")
        for i, r in enumerate(changed):
            reads[r]["nodes"] = [reads[r]["nodes"][int(k)] for k in out["order"][i]]
            nodes_to_encoded_read(reads[r], raw[reads[r]["id"]])
    return new_ids


def correct_chunk_deletion(ds, sim_thr=None, stddev_of_error=None, device=0):
    """correct_chunk_deletion (encode/deletion_fill.rs:136-231, 301-367) on the parsed JSON object `ds` (modified in place): up
    to 3 x 12 rounds in which every live read gets the nodes the other reads say it lacks.  One round = jtk_lc_fill_candidates
    on the live reads, the candidates a read has already failed taken out, the windows of try_encoding_head / _tail
    (api.fill_trials) with sim_thr = read error + (chunk, cluster) error + 10 stddev, one jtk_lc_encode_nodes call, per (read,
    slot, side) the accepted trial of highest score, the new nodes appended, one jtk_lc_settle_nodes call on the reads that
    changed, and their gaps and edges rebuilt (nodes_to_encoded_read).  The consensus sequences (take_consensus_sequence) and
    the error rates (jtk_lc_node_errors, jtk_lc_error_quantile unless sim_thr is given, jtk_lc_estimate_error_rate) are taken
    once, before the first round.  Returns the ids of the chunks that gained a node, ascending.
    This build's own decisions: the guided passes of encode_node and the polish behind the consensus follow DESIGN.md section 4
    (parity with kiley is not pinned), and among trials of equal score the last in the order jtk_lc_fill_candidates returns wins,
    where the reference takes the last in the order of its HashMap.  A read without nodes in `ds` raises ValueError: the
    reference fails its assert_eq of :190.  A trial that jtk_lc_encode_nodes refuses (a sequence above 32,000 bases, a band row
    above 4,096 cells) counts as a trial that failed, as encode_node's None does."""
    reads = ds["encoded_reads"]
    if any(not r["nodes"] for r in reads):
        raise ValueError("correct_deletion: an encoded read without nodes (the reference's assert_eq of deletion_fill.rs:190 fails)")
    with _Clock("take_consensus"):
        consensi = take_consensus_sequence(ds, device=device)                                        # :139
    node_off, nodes, _, chunks, seqs = _flat_nodes(ds)
    with _Clock("node_errors"):
        errs = api.node_errors(node_off, nodes, chunks, seqs, device=device)
        fallback = float(sim_thr) if sim_thr is not None else api.error_quantile(errs["err_num"], errs["err_len"], TAKE_THR, device=device)
    with _Clock("estimate_error_rate"):
        fit = api.estimate_error_rate(node_off, nodes, errs["err_num"], errs["err_len"], chunks, fallback, device=device)   # :144
    stddev = float(stddev_of_error) if stddev_of_error is not None else fit["median_of_sqrt_err"]    # :145
    read_err = {read["id"]: float(fit["read_err"][r]) for r, read in enumerate(reads)}
    chunk_err = {}
    for i, c in enumerate(ds["selected_chunks"]):
        for cl in range(int(c["cluster_num"])):
            chunk_err[c["id"], cl] = float(fit["chunk_err"][int(fit["chunk_err_off"][i]) + cl])
    state = [{"alive": True, "failed": set()} for _ in reads]
    found = set()
    for _ in range(OUTER_LOOP):
        for st in state:                                                                             # :181
            st["alive"] = True
            st["failed"].clear()
        updated = True
        for i in range(INNER_LOOP):
            prev = sum(len(r["nodes"]) for r in reads)
            found.update(_fill_round(ds, state, consensi, read_err, chunk_err, stddev, device))
            after = sum(len(r["nodes"]) for r in reads)
            if after == prev:                                                                        # :207-211
                updated = i != 0
                break
        if not updated:                                                                              # :165
            break
    return sorted(found)


def _original_seq(node):
    """Node::original_seq (definitions/src/lib.rs:737-753)"""
    if node["is_forward"]:
        return node["seq"]
    try:
        return "".join(_COMPLEMENT[b] for b in reversed(node["seq"].upper()))
    except KeyError:
        raise ValueError("a reverse node holds a base outside ACGT (Node::original_seq panics)") from None


def remove_node(read, i):
    """EncodedRead::remove (definitions/src/lib.rs:540-603): node i goes, and its bases join the gap or the edge beside it.  Not
    nodes_to_encoded_read: nothing is taken from the raw read, and an overlap (a negative edge offset) is cut as the reference
    cuts it."""
    nodes, edges = read["nodes"], read["edges"]
    if not (0 <= i < len(nodes)) or len(nodes) != len(edges) + 1:
        raise ValueError("EncodedRead::remove: index or edge count (the reference asserts)")
    n = len(nodes)
    gone = nodes.pop(i)
    if not nodes:
        read["leading_gap"] += _original_seq(gone)
    elif i + 1 == n:
        edge = edges.pop(i - 1)
        skip = -edge["offset"] if edge["offset"] < 0 else 0
        read["trailing_gap"] = (edge["label"] + _original_seq(gone) + read["trailing_gap"])[skip:]
    elif i == 0:
        edge = edges.pop(0)
        lead = read["leading_gap"] + _original_seq(gone) + edge["label"]
        read["leading_gap"] = lead[:max(len(lead) + edge["offset"], 0)] if edge["offset"] < 0 else lead
    else:
        edge, before = edges.pop(i), edges[i - 1]
        label = before["label"] + _original_seq(gone) + edge["label"]
        if before["offset"] < 0:
            label = label[-before["offset"]:]
        if edge["offset"] < 0:
            label = label[:max(len(label) + edge["offset"], 0)]
        before["to"] = edge["to"]
        before["label"] = label
        before["offset"] += len(gone["seq"]) + edge["offset"]


def _filter_indel_sizes(distr, copy_num, hap_coverage, indel_size, occupy_fraction):
    """filter_single_copy / filter_multi_copy (purge_diverged.rs:130-187) on one key's [(read id, node index, del_size)]:
    None where the key is dropped, else the entries that are removed.  `accept_size < size as usize` is restated: a negative
    del_size wraps to a huge usize and passes."""
    accept_size = int(math.ceil(indel_size * ACCEPT_RATE))
    passes = lambda size: size < 0 or accept_size < size   # noqa: E731
    if copy_num <= 1:
        num = sum(indel_size < d[2] for d in distr)
        upper_thr = int(math.ceil(len(distr) * (1.0 - occupy_fraction / 2.0)))
        if not 1 <= num < upper_thr:
            return None
        return [d for d in distr if passes(d[2])]
    lower_thr = max(int(math.floor(hap_coverage * occupy_fraction)), 0)
    upper_thr = int(math.ceil(max(float(len(distr)) - float(lower_thr), 0.0)))
    min_remove = sum(indel_size < d[2] for d in distr)
    max_remove = sum(accept_size < d[2] for d in distr)
    if not (lower_thr < min_remove and max_remove < upper_thr):
        return None
    # (the reference's sum / max_remove of :179 cannot divide by zero here: accept_size <= indel_size, so max_remove >= min_remove
    # > lower_thr >= 0)
    return [d for d in distr if passes(d[2])]


def purge_largeindel(ds, indel_size, occupy_fraction, compress, device=0):
    """PurgeDivergent::purge_largeindel (purge_diverged.rs:49-187) on the parsed JSON object `ds` (modified in place).  del_size
    of every node comes from jtk_lc_settle_nodes in mode STATS_ONLY; the nodes are grouped by (chunk, cluster) -- by chunk where
    `compress` -- the coverage is updated (misc::update_coverage), filter_single_copy / filter_multi_copy decide per group by the
    chunk's copy number, the nodes they name are taken out with EncodedRead::remove (remove_node) from the highest index of a read
    down, and reads left without nodes are dropped.  Returns the chunk ids of the groups that passed, ascending."""
    reads = ds["encoded_reads"]
    copy_num = {c["id"]: int(c["copy_num"]) for c in ds["selected_chunks"]}
    node_off, rec, ops, ops_off = _settle_arrays([r["nodes"] for r in reads])
    with _Clock("settle_nodes"):
        out = api.settle_nodes(node_off, rec, ops, ops_off, mode=ffi.SETTLE_STATS_ONLY, device=device)
    distr = {}
    e = 0
    for r, read in enumerate(reads):
        for idx, node in enumerate(read["nodes"]):
            if not node["cigar"]:
                raise ValueError("purge_largeindel: a node without ops (max_region of nothing is i64::MIN)")
            key = (node["chunk"], 0 if compress else node["cluster"])
            distr.setdefault(key, []).append((r, idx, int(out["stats"]["del_size"][e])))
            e += 1
    update_coverage(ds)                                                                              # :91
    hap_coverage = coverage_of(ds)[1]
    buckets, purged = {}, set()
    for (chunk, cluster), entries in distr.items():
        if chunk not in copy_num:
            raise ValueError(f"purge_largeindel: a node of chunk {chunk}, which is not selected (copy_num[&chunk] panics)")
        removed = _filter_indel_sizes(entries, copy_num[chunk], hap_coverage, indel_size, occupy_fraction)
        if removed is None:
            continue
        purged.add(chunk)
        for r, idx, _ in removed:
            buckets.setdefault(r, []).append(idx)
    for r, idxs in buckets.items():
        for idx in sorted(idxs, reverse=True):                                                       # :111
            remove_node(reads[r], idx)
    ds["encoded_reads"] = [r for r in reads if r["nodes"]]                                           # :52
    return sorted(purged)


def correct_deletion(ds, re_clustering=False, sim_thr=None, stddev_of_error=None, device=0):
    """CorrectDeletion::correct_deletion (encode/deletion_fill.rs:36-90) on the parsed JSON object `ds` (modified in place):
    correct_chunk_deletion, then purge_largeindel(MAX_ALLOWED_GAP, 0.5) by (chunk, cluster) and once more by chunk.  Returns the
    ids of the chunks that gained a node or had a group purged, ascending -- the reference's find_new_chunks."""
    if re_clustering:
        raise NotImplementedError("re_clustering=True needs estimate_multiplicity, which is another subsystem")
    found = set(correct_chunk_deletion(ds, sim_thr=sim_thr, stddev_of_error=stddev_of_error, device=device))
    found.update(purge_largeindel(ds, MAX_ALLOWED_GAP, OCCUPY_FRACTION, False, device=device))
    found.update(purge_largeindel(ds, MAX_ALLOWED_GAP, OCCUPY_FRACTION, True, device=device))
    return sorted(found)


def mask_repeat(ds, k=12, freq=0.001, min_count=10, device=0, record=None):
    """RepeatMask::mask_repeat (repeat_masking.rs:135-158) on the parsed JSON object `ds` (modified in place): raw_reads[*].seq is
    rewritten -- upper case, lower case where a masked k-mer covers the base -- and masked_kmers.k is set; masked_kmers.thr stays
    as it was (the reference computes thr and drops it).  The defaults are example.toml's.  record: a list that receives the
    reference's three debug rows.  Where the reference panics (no k-mer is counted twice, or freq is too small to matter) this
    raises ffi.JtkError with status -6 and leaves `ds` alone.  Returns the report of api.mask_repeats."""
    reads = ds["raw_reads"]
    masked, report, mask = api.mask_repeats([r["seq"].encode("latin-1") for r in reads], k, freq, min_count, device=device)
    if report["rc"] != 0:
        raise ffi.JtkError(report["rc"], "mask_repeat: no k-mer at the percentile (create_mask's counts[percentile] panics)")
    ds["masked_kmers"]["k"] = int(k)
    for r, seq in zip(reads, masked):
        r["seq"] = seq.decode("latin-1")
    if record is not None:
        record.append("MASKREPEAT\tMaskLen\t%d\t%d" % (k, len(mask)))
        record.append("MASKREPEAT\tTotalMask\t%d\t%d" % (report["n_lower"], report["n_bases"]))
        record.append("MASKREPEAT\tMaskedKmers\t%d\t%d" % (len(mask), k))
    return report


def get_repetitive_kmer(ds, device=0):
    """RepeatMask::get_repetitive_kmer (repeat_masking.rs:109-134): the RepeatAnnot of a masked data set, dict(k, kmers) with the
    k-mers of every all-lower-case window of the raw reads, ascending"""
    k = int(ds["masked_kmers"]["k"])
    return dict(k=k, kmers=api.repetitive_kmers([r["seq"].encode("latin-1") for r in ds["raw_reads"]], k, device=device))


def repetitiveness(ds_or_kmers, seqs, device=0):
    """RepeatAnnot::repetitiveness (repeat_masking.rs:90-105) of every sequence of `seqs` (str or bytes) as np.float64;
    ds_or_kmers is a data set or what get_repetitive_kmer returned for one"""
    annot = get_repetitive_kmer(ds_or_kmers, device=device) if "raw_reads" in ds_or_kmers else ds_or_kmers
    seqs = [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in seqs]
    return api.repetitiveness(seqs, annot["k"], annot["kmers"], device=device)


def encode_by_map(ds, sim_thr, device=0, **map_params):
    """The counterpart of encode_by_mm2 + encode_by (encode/mod.rs:41-139) on the parsed JSON object `ds` (modified in place: only
    encoded_reads is written).  Where the reference pipes every raw read through minimap2 and makes a node of every PAF line whose
    alignment reaches within 25 bases of the chunk's ends at an identity above 1 - sim_thr, this
      1. maps every raw read against selected_chunks (api.map_reads; map_params are its k, w, max_occ, max_gap, min_seeds),
      2. turns every placement into a window of the read (api.map_trials) with cons = the chunk's own sequence,
      3. runs all windows through one api.encode_nodes call (encode_node, deletion_fill.rs:451-566: the alignment, the identity
         and edge tests against sim_thr, the trimmed query, the ops against the chunk),
      4. makes a Node (cluster 0) of every accepted trial,
      5. keeps, where two accepted trials of one read and chunk overlap by more than half the chunk, the better score (of equal
         scores the first in placement order),
      6. settles every read's nodes in one api.settle_nodes call in mode SETTLE_BY_CHUNK (the sorts and remove_slippy_alignment of
         encode_read_to_nodes_by_paf, :133-138, followed by remove_overlapping_encoding as that entry point always does),
      7. rebuilds gaps and edges (nodes_to_encoded_read); reads without a node are dropped (:75-79).
    The mapper and the guided passes follow this build's own specifications: parity with minimap2's
    alignments is not pinned.  Returns the number of trials that were tried."""
    chunks, reads = ds["selected_chunks"], ds["raw_reads"]
    chunk_seqs = [c["seq"].upper().encode("latin-1") for c in chunks]
    read_seqs = [r["seq"].encode("latin-1") for r in reads]
    with _Clock("map_reads"):
        placed = api.map_reads(chunk_seqs, read_seqs, device=device, **map_params)
    picks = api.map_trials(placed, [len(s) for s in read_seqs], [len(s) for s in chunk_seqs], sim_thr)
    ds["encoded_reads"] = []
    if not picks:
        return 0
    read_off = np.zeros(len(read_seqs) + 1, dtype=np.int64)
    read_off[1:] = np.cumsum([len(s) for s in read_seqs])
    chunk_off = np.zeros(len(chunk_seqs) + 1, dtype=np.int64)
    chunk_off[1:] = np.cumsum([len(s) for s in chunk_seqs])
    read_bases = np.frombuffer(b"".join(read_seqs), dtype=np.uint8)
    chunk_bases = np.frombuffer(b"".join(chunk_seqs), dtype=np.uint8)
    trials = np.zeros(len(picks), dtype=ffi.ENCODE_TRIAL_DT)
    for t, (i, start, end, forward, thr) in enumerate(picks):
        r, c = int(placed[i]["query"]), int(placed[i]["target"])
        trials[t] = (read_off[r], start, end, forward, len(chunk_seqs[c]), chunk_off[c], chunk_off[c], len(chunk_seqs[c]), 0, thr)
    with _Clock("encode_nodes"):
        enc = api.encode_nodes(trials, read_bases, chunk_bases, chunk_bases, device=device, raise_on_trial_failure=False)
    per_read = {}
    for t, (i, start, end, forward, _) in enumerate(picks):
        res = enc["result"][t]
        if int(res["status"]) != 0 or int(res["verdict"]) != ffi.ENCODE_ACCEPTED:
            continue                                       # (a trial the device refuses is a trial that fails: encode_node's None)
        r, c = int(placed[i]["query"]), int(placed[i]["target"])
        window = api._oriented_window(read_bases, int(read_off[r]), start, end, forward)
        query = window[int(res["trim_head"]):len(window) - int(res["trim_tail"])]
        k = int(chunks[c]["cluster_num"])
        node = {"position_from_start": int(res["position_from_start"]), "chunk": chunks[c]["id"], "cluster": 0, "seq": query.decode("ascii"),
                "is_forward": bool(forward), "cigar": ops_to_cigar(enc["ops"][int(enc["ops_off"][t]):int(enc["ops_off"][t + 1])]),
                "posterior": [math.log(1.0 / max(k, 1))] * k}                                        # Node::new, lib.rs:723-731
        per_read.setdefault(r, []).append((node, int(res["score"]), len(chunk_seqs[c])))
    kept = {r: _drop_overlapping_trials(found) for r, found in per_read.items()}
    order = sorted(kept)
    node_off, rec, ops, ops_off = _settle_arrays([kept[r] for r in order])
    with _Clock("settle_nodes"):
        out = api.settle_nodes(node_off, rec, ops, ops_off, mode=ffi.SETTLE_BY_CHUNK, device=device)
    if out["rc"] != 0:
        raise ValueError("encode_by_map: a node without ops")
    for i, r in enumerate(order):
        read = {"id": reads[r]["id"], "nodes": [kept[r][int(j)] for j in out["order"][i]]}
        nodes_to_encoded_read(read, reads[r]["seq"])
        ds["encoded_reads"].append({key: read[key] for key in ("id", "original_length", "leading_gap", "trailing_gap", "edges", "nodes")})
    return len(picks)


def _drop_overlapping_trials(found):
    """found: (node, score, chunk length) of a read's accepted trials, in placement order.  Of two nodes of one chunk whose spans in
    the read overlap by more than half the chunk, the better score stays (the first where they are equal); -> the nodes left"""
    kept = []
    for node, score, chunk_len in found:
        start, end = node["position_from_start"], node["position_from_start"] + len(node["seq"])
        rival = None
        for j, (other, other_score, _) in enumerate(kept):
            lo, hi = max(start, other["position_from_start"]), min(end, other["position_from_start"] + len(other["seq"]))
            if other["chunk"] == node["chunk"] and 2 * (hi - lo) > chunk_len:
                rival = j
                break
        if rival is None:
            kept.append((node, score, chunk_len))
        elif kept[rival][1] < score:
            kept[rival] = (node, score, chunk_len)
    return [k[0] for k in kept]


def is_uppercase(read):
    """encode::is_uppercase (encode/mod.rs:357-367)"""
    upper = lambda s: all("A" <= c <= "Z" for c in s)   # noqa: E731
    return all(upper(n["seq"]) for n in read["nodes"]) and all(upper(e["label"]) for e in read["edges"])


def encode(ds, sim_thr, sd_of_error, device=0, **map_params):
    """Encode::encode (encode/mod.rs:19-39) on the parsed JSON object `ds` (modified in place): encode_by_map in the place of
    encode_by_mm2, correct_chunk_deletion with sim_thr and sd_of_error, and the reference's assertion that every node and edge
    label is upper case.  Returns the ids of the chunks that gained a node in the second step."""
    encode_by_map(ds, sim_thr, device=device, **map_params)
    found = correct_chunk_deletion(ds, sim_thr=sim_thr, stddev_of_error=sd_of_error, device=device) if ds["encoded_reads"] else []
    if not all(is_uppercase(r) for r in ds["encoded_reads"]):
        raise ValueError("encode: a node or an edge label that is not upper case (the reference asserts)")
    return found


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--stage", default="local_clustering", choices=("local_clustering", "correct_clustering", "squish_erroneous_clusters", "corrected", "realign", "purge_diverged_nodes", "fill_candidates", "consensus_sequences", "correct_deletion", "mask_repeat", "encode"),
                    help="which JTK stage to run on the file (jtk local_clustering / jtk correct_clustering); "
                         "squish_erroneous_clusters: the step JTK runs in front of the correction, with its default "
                         "configuration; corrected: that step, then correct_clustering (cli/src/pipeline.rs:174-175); realign: "
                         "replace every node's cigar by its global alignment to the chunk sequence; purge_diverged_nodes: the first "
                         "half of `ds.purge` (purge_diverged.rs:238-322), the purged chunk ids go to stderr; fill_candidates: the "
                         "candidate search of correct_deletion (deletion_fill.rs:301-337) -- the output is a REPORT, a JSON list "
                         "keyed by read id with coverage, ins_thr and the head / tail candidates, not a DataSet: testing a "
                         "candidate against the sequence (encode_node, kiley's infix_guided) is JTK's; consensus_sequences: "
                         "take_consensus_sequence (deletion_fill.rs:260-285) -- also a REPORT, {\"chunk,cluster\": \"ACGT...\"}, made with "
                         "this build's guided polish (parity with kiley's polish_until_converge is not pinned); correct_deletion: "
                         "`ds.correct_deletion` without re-clustering (deletion_fill.rs:36-44: the filling rounds, then purge_largeindel "
                         "twice), the chunk ids that changed go to stderr; the guided passes and the polish are this build's own; "
                         "mask_repeat: `ds.mask_repeat` (repeat_masking.rs:135-158, the pipeline's first step) with --kmersize, "
                         "--top-freq and --min-count; -v writes its three MASKREPEAT rows; encode: `ds.encode` (encode/mod.rs:19-39) "
                         "with --sim-thr and --sd-of-error: the reads are mapped onto selected_chunks by this build's own minimizer "
                         "mapper in the place of minimap2 (--map-k, --map-w; parity with minimap2 is not pinned), encoded, and "
                         "correct_chunk_deletion fills in what the mapping missed")
    ap.add_argument("input", help="DataSet JSON ('-' = stdin)")
    ap.add_argument("output", help="DataSet JSON ('-' = stdout)")
    ap.add_argument("--chunks", default="", help="comma-separated chunk ids (local_clustering_selected); default: all")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--kmersize", type=int, default=12, help="mask_repeat: k (example.toml: 12)")
    ap.add_argument("--top-freq", type=float, default=0.001, help="mask_repeat: the fraction of the repeated k-mers to mask (0.001)")
    ap.add_argument("--min-count", type=int, default=10, help="mask_repeat: k-mers counted this often or less are not masked (10)")
    ap.add_argument("--sim-thr", type=float, default=None, help="encode: the error rate a node may have (required there)")
    ap.add_argument("--sd-of-error", type=float, default=None,
                    help="encode: the standard deviation of the error rate (default: the median correct_chunk_deletion estimates)")
    ap.add_argument("--map-k", type=int, default=15, help="encode: the mapper's k-mer size (15)")
    ap.add_argument("--map-w", type=int, default=10, help="encode: the mapper's minimizer window (10)")
    ap.add_argument("--no-refit", action="store_true",
                    help="skip update_models_on_both_strands (mod.rs:58): cluster with model_param as found in the file")
    ap.add_argument("--recluster", action="store_true",
                    help="after purge_diverged_nodes: local_clustering_selected on the purged chunks with the copy numbers as they "
                         "stand (re_cluster, purge_diverged.rs:189-236, without its estimate_multiplicity)")
    ap.add_argument("--keep-going", action="store_true",
                    help="a chunk that fails (where the reference would panic, or an unsupported shape) is left untouched "
                         "and listed on stderr instead of aborting the stage")
    ap.add_argument("-v", "--verbose", action="store_true",
                    help="write the reference's per-chunk RECORD lines (mod.rs:121, its debug! level) to stderr")
    ap.add_argument("--trace", action="store_true",
                    help="write the reference's trace! rows of every clustered chunk (TOTAL / CAND / PICK / DUMP / RANGE / LK / "
                         "COUNTS; its -vvv) to stderr")
    args = ap.parse_args(argv)
    ds = json.load(sys.stdin if args.input == "-" else open(args.input))
    failed = [] if args.keep_going else None
    record = [] if args.verbose else None
    trace = [] if args.trace else None
    if args.stage in ("squish_erroneous_clusters", "corrected"):
        validate(ds)
        squish_erroneous_clusters(ds, device=args.device)
        if args.stage == "corrected":
            correct_clustering(ds, device=args.device)
    elif args.stage == "purge_diverged_nodes":
        validate(ds)
        purged = purge_diverged_nodes(ds, device=args.device)
        sys.stderr.write("PD\tPurged\t%s\n" % ",".join(str(x) for x in purged))
        if args.recluster and purged:
            local_clustering_selected(ds, purged, device=args.device, failed=failed, refit=not args.no_refit, record=record, trace=trace)
    elif args.stage == "correct_deletion":
        validate(ds)
        changed = correct_deletion(ds, device=args.device)
        sys.stderr.write("CD\tChanged\t%s\n" % ",".join(str(x) for x in changed))
    elif args.stage == "mask_repeat":
        validate(ds)
        mask_repeat(ds, k=args.kmersize, freq=args.top_freq, min_count=args.min_count, device=args.device, record=record)
    elif args.stage == "encode":
        validate(ds)
        if args.sim_thr is None:
            ap.error("--stage encode needs --sim-thr")
        encode(ds, args.sim_thr, args.sd_of_error, device=args.device, k=args.map_k, w=args.map_w)
        sys.stderr.write("ENCODE\tEncoded\t%d\t%d\n" % (len(ds["encoded_reads"]), len(ds["raw_reads"])))
    elif args.stage == "fill_candidates":
        ds = fill_candidates(ds, device=args.device)   # the report takes the data set's place in the output
    elif args.stage == "consensus_sequences":
        validate(ds)
        ds = {"%d,%d" % key: seq for key, seq in take_consensus_sequence(ds, device=args.device).items()}   # a report as well
    elif args.stage == "correct_clustering":
        validate(ds)
        if args.chunks:
            correct_clustering_selected(ds, [int(x) for x in args.chunks.split(",")], device=args.device)
        else:
            correct_clustering(ds, device=args.device)
    elif args.stage == "realign":
        validate(ds)
        realign_selected(ds, [int(x) for x in args.chunks.split(",")] if args.chunks else [c["id"] for c in ds["selected_chunks"]],
                         device=args.device)
    elif args.chunks:
        local_clustering_selected(ds, [int(x) for x in args.chunks.split(",")], device=args.device, failed=failed,
                                  refit=not args.no_refit, record=record, trace=trace)
    else:
        local_clustering(ds, device=args.device, failed=failed, refit=not args.no_refit, record=record, trace=trace)
    for row in (trace or []) + (record or []):
        sys.stderr.write(row + "\n")
    for cid, status in failed or []:
        sys.stderr.write(f"LC\tFAILED\t{cid}\t{status}\t{ffi.lib().jtk_lc_strerror(status).decode()}\n")
    api.trim_cache(args.device)
    text = json.dumps(ds)
    if args.output == "-":
        sys.stdout.write(text + "\n")
    else:
        with open(args.output, "w") as f:
            f.write(text + "\n")
    return 3 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
