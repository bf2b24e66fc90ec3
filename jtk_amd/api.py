"""Thin numpy wrappers over the C-ABI (include/jtk_lc.h).  Every compute function runs on the GPU through
libjtk_lc.so; there is no fallback path."""
import ctypes as C

import numpy as np

from . import ffi
from .ffi import check, f64p, u8p, u32p, u64p


def _outputs(batch):
    n_chunks, n_reads, stride = batch.n_chunks, batch.n_reads, batch.post_stride
    label = np.zeros(n_reads, dtype=np.uint32)
    post = np.zeros((n_reads, stride), dtype=np.float64)
    result = np.zeros(n_chunks, dtype=ffi.RESULT_DT)
    cons_cap = int(batch.chunks["tmpl_len"].sum()) * 2 + 64 * n_chunks + 64
    ops_cap = int(len(batch.ops)) * 2 + 64 * n_reads + 64
    cons = np.zeros(cons_cap, dtype=np.uint8)
    cons_off = np.zeros(n_chunks + 1, dtype=np.uint64)
    ops_out = np.zeros(ops_cap, dtype=np.uint8)
    ops_out_off = np.zeros(n_reads + 1, dtype=np.uint64)
    return dict(label=label, log_post=post, result=result, cons=cons, cons_off=cons_off, ops_out=ops_out,
                ops_out_off=ops_out_off)


def cluster_chunks(params, batch, device=0, raise_on_chunk_failure=True, devices=None, out=None):
    """jtk_lc_cluster_chunks: polish + variant search + clustering for every chunk of `batch`;
    devices=[...]: jtk_lc_cluster_chunks_multi over that list of GPUs; out = the output arrays of an earlier call on a batch of
    this shape, to be overwritten (a host that enters the stage several times keeps its buffers)."""
    L = ffi.lib()
    o = out if out is not None else _outputs(batch)
    args = (C.byref(params), batch.n_chunks, batch.chunks.ctypes.data, u8p(batch.tmpl_bases),
            u8p(batch.read_bases), u64p(batch.read_off), u8p(batch.ops), u64p(batch.ops_off),
            u8p(batch.strand), u32p(o["label"]), f64p(o["log_post"]), batch.post_stride,
            o["result"].ctypes.data, u8p(o["cons"]), u64p(o["cons_off"]), len(o["cons"]),
            u8p(o["ops_out"]), u64p(o["ops_out_off"]), len(o["ops_out"]))
    if devices is None:
        rc = L.jtk_lc_cluster_chunks(*args, device)
    else:
        dev = (C.c_int * len(devices))(*devices)
        rc = L.jtk_lc_cluster_chunks_multi(*args, dev, len(devices))
    if rc != 0 and (raise_on_chunk_failure or rc != -6):
        check(rc)
    o["rc"] = rc
    return o


def cluster_polished(params, batch, device=0, raise_on_chunk_failure=True):
    """jtk_lc_cluster_polished: the template is already the polished consensus (pseudo_mcmc::clustering)."""
    L = ffi.lib()
    o = _outputs(batch)
    rc = L.jtk_lc_cluster_polished(C.byref(params), batch.n_chunks, batch.chunks.ctypes.data,
                                   u8p(batch.tmpl_bases), u8p(batch.read_bases), u64p(batch.read_off), u8p(batch.ops),
                                   u64p(batch.ops_off), u8p(batch.strand), u32p(o["label"]), f64p(o["log_post"]),
                                   batch.post_stride, o["result"].ctypes.data, device)
    if rc != 0 and (raise_on_chunk_failure or rc != -6):
        check(rc)
    o["rc"] = rc
    return o


def polish_chunks(params, batch, radius=0, take_num=0, ignore_edge=0, device=0, raise_on_chunk_failure=True):
    """jtk_lc_polish_chunks: polish_until_converge_antidiagonal on every window of `batch` (no clustering)."""
    L = ffi.lib()
    o = _outputs(batch)
    rc = L.jtk_lc_polish_chunks(C.byref(params), batch.n_chunks, batch.chunks.ctypes.data, u8p(batch.tmpl_bases),
                                u8p(batch.read_bases), u64p(batch.read_off), u8p(batch.ops), u64p(batch.ops_off),
                                u8p(batch.strand), radius, take_num, ignore_edge, u8p(o["cons"]), u64p(o["cons_off"]),
                                len(o["cons"]), u8p(o["ops_out"]), u64p(o["ops_out_off"]), len(o["ops_out"]),
                                o["result"].ctypes.data, device)
    if rc != 0 and (raise_on_chunk_failure or rc != -6):
        check(rc)
    o["rc"] = rc
    return o


ALIGN_MODES = {"global": 0, "infix": 1, "prefix": 2}     # enum jtk_align_mode
ALIGN_FREE = {"template": 0, "read": 1}                  # enum jtk_align_free


def align_reads(batch, max_dist=0, device=0, raise_on_read_failure=True, mode="global", free="template"):
    """jtk_lc_align_reads: global unit-cost alignment of every read of `batch` to its chunk's template (the batch's own ops
    are not looked at).  -> dict(ops, ops_off, dist, status, rc); `batch.with_ops(out["ops"], out["ops_off"])` carries them
    into polish_chunks / cluster_chunks.
    mode="infix" / "prefix": jtk_lc_align_reads_mode with the `free` sequence ("template" or "read") consumed only on
    [start, end); the dict gains `start` and `end` (see `semiglobal` for ops that consume both sequences whole)."""
    L = ffi.lib()
    n = batch.n_reads
    cap = int(len(batch.read_bases)) + int((batch.chunks["tmpl_len"] * batch.chunks["n_reads"]).sum()) + 64
    ops = np.zeros(cap, dtype=np.uint8)
    ops_off = np.zeros(n + 1, dtype=np.uint64)
    dist = np.zeros(n, dtype=np.uint32)
    status = np.zeros(n, dtype=np.int32)
    if mode not in ALIGN_MODES or free not in ALIGN_FREE:
        raise ValueError("mode is one of %s, free one of %s" % (sorted(ALIGN_MODES), sorted(ALIGN_FREE)))
    extra = {}
    if mode == "global":
        rc = L.jtk_lc_align_reads(batch.n_chunks, batch.chunks.ctypes.data, u8p(batch.tmpl_bases), u8p(batch.read_bases),
                                  u64p(batch.read_off), int(max_dist), u8p(ops), u64p(ops_off), cap, u32p(dist),
                                  status.ctypes.data_as(C.POINTER(C.c_int32)), device)
    else:
        extra = dict(start=np.zeros(n, dtype=np.uint32), end=np.zeros(n, dtype=np.uint32))
        rc = L.jtk_lc_align_reads_mode(batch.n_chunks, batch.chunks.ctypes.data, u8p(batch.tmpl_bases), u8p(batch.read_bases),
                                       u64p(batch.read_off), ALIGN_MODES[mode], ALIGN_FREE[free], int(max_dist), u8p(ops),
                                       u64p(ops_off), cap, u32p(dist), u32p(extra["start"]), u32p(extra["end"]),
                                       status.ctypes.data_as(C.POINTER(C.c_int32)), device)
    if rc != 0 and (raise_on_read_failure or rc != -6):
        check(rc)
    return dict(ops=ops[:int(ops_off[n])] if rc in (0, -6) else ops[:0], ops_off=ops_off, dist=dist, status=status, rc=rc, **extra)


def semiglobal(batch, max_dist=0, device=0):
    """`semiglobal` (encode/mod.rs:227-246) for every read of `batch`: the template is placed inside the read (infix, the read
    free) and the read's bases in front of `start` and behind `end` become Ins, so the ops consume both sequences whole.
    -> dict(ops, ops_off, dist, start, end, status, rc), ready for `batch.with_ops(out["ops"], out["ops_off"])`."""
    o = align_reads(batch, max_dist=max_dist, device=device, mode="infix", free="read")
    rl = np.diff(batch.read_off.astype(np.int64))
    n_in = np.diff(o["ops_off"].astype(np.int64))
    lead = o["start"].astype(np.int64)
    trail = rl - o["end"].astype(np.int64)
    # the reference's guards come out of the same sums: an empty template gives the read as Ins (no ops, start = end = 0)
    off = np.zeros(batch.n_reads + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lead + n_in + trail)
    ops = np.full(int(off[-1]), 2, dtype=np.uint8)                       # JTK_OP_INS; the aligned stretches are copied in
    for r in range(batch.n_reads):
        a = int(off[r]) + int(lead[r])
        ops[a:a + int(n_in[r])] = o["ops"][int(o["ops_off"][r]):int(o["ops_off"][r + 1])]
    return dict(ops=ops, ops_off=off, dist=o["dist"], start=o["start"], end=o["end"], status=o["status"], rc=o["rc"])


def modification_table(params, tmpl, reads, ops, strands, device=0):
    """jtk_lc_modification_table for one pile-up -> (table [n, 14*(L+1)] minus lk, lk [n])."""
    L = ffi.lib()
    n = len(reads)
    rb = np.concatenate(reads).astype(np.uint8) if n else np.zeros(0, np.uint8)
    ob = np.concatenate(ops).astype(np.uint8) if n else np.zeros(0, np.uint8)
    ro = np.zeros(n + 1, dtype=np.uint64)
    oo = np.zeros(n + 1, dtype=np.uint64)
    ro[1:] = np.cumsum([len(r) for r in reads])
    oo[1:] = np.cumsum([len(o) for o in ops])
    st = np.array([1 if s else 0 for s in strands], dtype=np.uint8)
    tmpl = np.ascontiguousarray(tmpl, dtype=np.uint8)
    table = np.zeros((n, ffi.NUM_ROW * (len(tmpl) + 1)), dtype=np.float64)
    lk = np.zeros(n, dtype=np.float64)
    check(L.jtk_lc_modification_table(C.byref(params), u8p(tmpl), len(tmpl), n, u8p(rb), u64p(ro), u8p(ob), u64p(oo),
                                      u8p(st), f64p(table), f64p(lk), device))
    return table, lk


def estimate_gains(hmm_forward, hmm_reverse, seed=309423, seq_len=100, band=10, homop_len=3, device=0):
    """jtk_lc_estimate_gains; the defaults are estimate_gain_default's (likelihood_gains.rs:186-192)."""
    out = ffi.Gains()
    check(ffi.lib().jtk_lc_estimate_gains(C.byref(hmm_forward), C.byref(hmm_reverse), seed, seq_len, band, homop_len,
                                          C.byref(out), device))
    return out


def estimate_minimum_gain(hmm_forward, hmm_reverse, seed=23908, sample_num=1000, seq_num=500, seq_len=100, band=25, device=0):
    """jtk_lc_estimate_minimum_gain; the defaults are the reference's constants (likelihood_gains.rs:7-11)."""
    out = C.c_double(0.0)
    check(ffi.lib().jtk_lc_estimate_minimum_gain(C.byref(hmm_forward), C.byref(hmm_reverse), seed, sample_num, seq_num, seq_len,
                                                 band, C.byref(out), device))
    return out.value


def gains_batches():
    """what jtk_lc_debug_gains_batch (include/jtk_lc_debug.h) kept of this thread's last estimate_gains / estimate_minimum_gain
    call: one dict per device batch with tmpl / tmpl_off, reads / read_off, ops [pairs, 512] / ops_len as edit_ops_kernel wrote
    them, and lk [pairs].  Empty unless the switch was on during the call."""
    L = ffi.lib()
    out = []
    for b in range(L.jtk_lc_debug_gains_batches()):
        sizes = np.zeros(4, dtype=np.uint64)
        check(L.jtk_lc_debug_gains_batch_sizes(b, u64p(sizes)))
        n_tmpl, tmpl_bytes, pairs, read_bytes = (int(v) for v in sizes)
        k = dict(tmpl=np.zeros(tmpl_bytes, np.uint8), tmpl_off=np.zeros(n_tmpl + 1, np.uint64), reads=np.zeros(read_bytes, np.uint8),
                 read_off=np.zeros(pairs + 1, np.uint64), ops=np.zeros((pairs, ffi.DEBUG_GAINS_OPS_STRIDE), np.uint8),
                 ops_len=np.zeros(pairs, np.uint32), lk=np.zeros(pairs))
        check(L.jtk_lc_debug_gains_batch(b, u8p(k["tmpl"]), u64p(k["tmpl_off"]), u8p(k["reads"]), u64p(k["read_off"]), u8p(k["ops"]),
                                         u32p(k["ops_len"]), f64p(k["lk"])))
        out.append(k)
    return out


def with_gains_batches(call, *args, **kw):
    """call(*args, **kw) -- estimate_gains or estimate_minimum_gain -- with the diagnostic keep switch on: returns (its result, or
    the JtkError it raised; gains_batches()).  A test hook: the switch is off again, and nothing is kept, when this returns."""
    L = ffi.lib()
    L.jtk_lc_debug_gains_keep(1)
    try:
        try:
            res = call(*args, **kw)
        except ffi.JtkError as e:
            res = e
        return res, gains_batches()
    finally:
        L.jtk_lc_debug_gains_keep(0)


def fit_model(params, batch, rounds=10, device=0):
    """jtk_lc_fit_model: the model refit of the stage preamble (model_tune.rs:119-152) on the training pile-ups `batch`;
    returns (forward, reverse)."""
    f, r = ffi.Hmm(), ffi.Hmm()
    check(ffi.lib().jtk_lc_fit_model(C.byref(params), batch.n_chunks, batch.chunks.ctypes.data, u8p(batch.tmpl_bases),
                                     u8p(batch.read_bases), u64p(batch.read_off), u8p(batch.ops), u64p(batch.ops_off),
                                     u8p(batch.strand), rounds, C.byref(f), C.byref(r), device))
    return f, r


def correct_clustering(read_id, node_off, nodes, posteriors, chunks, selection, haploid_coverage, min_gain, device=0):
    """jtk_lc_correct_clustering: AlignmentCorrection::correct_clustering_selected (phmm_likelihood_correction.rs:32-97).
    `nodes` (ffi.CC_NODE_DT) are the reads' nodes flattened by `node_off`; `chunks` (ffi.CC_CHUNK_DT) is updated in place
    (cluster_num).  Returns (cluster, touched) per node."""
    nodes = np.ascontiguousarray(nodes, dtype=ffi.CC_NODE_DT)
    posteriors = np.ascontiguousarray(posteriors, dtype=np.float64)
    read_id = np.ascontiguousarray(read_id, dtype=np.uint64)
    node_off = np.ascontiguousarray(node_off, dtype=np.uint64)
    selection = np.ascontiguousarray(selection, dtype=np.uint64)
    if chunks.dtype != ffi.CC_CHUNK_DT or not chunks.flags.c_contiguous:
        raise ValueError("chunks must be a contiguous array of ffi.CC_CHUNK_DT (it is updated in place)")
    cluster = np.zeros(len(nodes), dtype=np.uint64)
    touched = np.zeros(len(nodes), dtype=np.uint8)
    check(ffi.lib().jtk_lc_correct_clustering(len(read_id), u64p(read_id), u64p(node_off), nodes.ctypes.data, f64p(posteriors),
                                              len(chunks), chunks.ctypes.data, len(selection), u64p(selection),
                                              float(haploid_coverage), float(min_gain), u64p(cluster), u8p(touched), device))
    return cluster, touched


def squish_clusters(node_off, nodes, posteriors, chunks, config=None, device=0):
    """jtk_lc_squish_clusters: SquishErroneousClusters::squish_erroneous_clusters (squish_erroneous_clusters.rs:44-60) on the
    flattened data set of correct_clustering.  `chunks` (ffi.CC_CHUNK_DT) is updated in place (cluster_num = 1 where
    suspicious).  Returns dict(classes, cluster, touched, pair_u1, pair_u2, pair_ari, pair_count): the class per chunk
    (ffi.REL_*), the cluster and the rewritten flag per node (a rewritten node's posterior is [0.0]) and the surviving chunk
    pairs ascending by (u1, u2)."""
    nodes = np.ascontiguousarray(nodes, dtype=ffi.CC_NODE_DT)
    posteriors = np.ascontiguousarray(posteriors, dtype=np.float64)
    node_off = np.ascontiguousarray(node_off, dtype=np.uint64)
    if chunks.dtype != ffi.CC_CHUNK_DT or not chunks.flags.c_contiguous:
        raise ValueError("chunks must be a contiguous array of ffi.CC_CHUNK_DT (it is updated in place)")
    cfg = config if config is not None else ffi.SquishConfig()
    # every surviving pair has count_thr < count, and the counts add up to at most sum n (n - 1) / 2 over the reads
    lens = np.diff(node_off).astype(object)
    total = int(sum(n * (n - 1) // 2 for n in lens))
    k = int((chunks["cluster_num"] > 1).sum())
    cap = min(total // (int(cfg.count_thr) + 1), k * (k + 1) // 2)
    u1, u2 = np.zeros(cap + 1, dtype=np.uint64), np.zeros(cap + 1, dtype=np.uint64)
    ari, count = np.zeros(cap + 1, dtype=np.float64), np.zeros(cap + 1, dtype=np.uint64)
    classes = np.zeros(len(chunks) + 1, dtype=np.uint8)
    cluster = np.zeros(len(nodes) + 1, dtype=np.uint64)
    touched = np.zeros(len(nodes) + 1, dtype=np.uint8)
    n_pairs = C.c_size_t(0)
    check(ffi.lib().jtk_lc_squish_clusters(len(node_off) - 1, u64p(node_off), nodes.ctypes.data, f64p(posteriors), len(chunks),
                                           chunks.ctypes.data, C.byref(cfg), u8p(classes), u64p(cluster), u8p(touched), u64p(u1),
                                           u64p(u2), f64p(ari), u64p(count), cap, C.byref(n_pairs), device))
    n = n_pairs.value
    return dict(classes=classes[:len(chunks)], cluster=cluster[:len(nodes)], touched=touched[:len(nodes)], pair_u1=u1[:n],
                pair_u2=u2[:n], pair_ari=ari[:n], pair_count=count[:n])


def squish_classify(u1, u2, ari, count, config=None):
    """jtk_lc_squish_classify (host only): classify (squish_erroneous_clusters.rs:254-365) on a pair list in the order given.
    Returns (ids, stiff): the chunk ids in first-appearance order and their labels."""
    u1 = np.ascontiguousarray(u1, dtype=np.uint64)
    u2 = np.ascontiguousarray(u2, dtype=np.uint64)
    ari = np.ascontiguousarray(ari, dtype=np.float64)
    count = np.ascontiguousarray(count, dtype=np.uint64)
    if not len(u1) == len(u2) == len(ari) == len(count):
        raise ValueError("the four pair arrays differ in length")
    cfg = config if config is not None else ffi.SquishConfig()
    cap = 2 * len(u1)
    ids, stiff = np.zeros(cap + 1, dtype=np.uint64), np.zeros(cap + 1, dtype=np.uint8)
    n_ids = C.c_size_t(0)
    check(ffi.lib().jtk_lc_squish_classify(len(u1), u64p(u1), u64p(u2), f64p(ari), u64p(count), C.byref(cfg), u64p(ids), u8p(stiff),
                                           cap, C.byref(n_ids)))
    return ids[:n_ids.value], stiff[:n_ids.value]


def _sequences(seqs):
    """(bases, off, ops, ops_off, tmpl, tmpl_off) of the purge entry points as contiguous arrays of the ABI's types"""
    kinds = (np.uint8, np.uint64, np.uint8, np.uint64, np.uint8, np.uint64)
    return tuple(np.ascontiguousarray(a, dtype=k) for a, k in zip(seqs, kinds))


def _flat_chunks(chunks):
    if chunks.dtype != ffi.CC_CHUNK_DT or not chunks.flags.c_contiguous:
        raise ValueError("chunks must be a contiguous array of ffi.CC_CHUNK_DT")


def node_errors(node_off, nodes, chunks, seqs, device=0, raise_on_node_failure=True):
    """jtk_lc_node_errors: per node the alignment columns against its chunk (Node::recover, definitions/src/lib.rs:773-813)
    that are not '|' and their number; a node's error rate is err_num / err_len (determine_chunks.rs:796-803).
    `seqs` = (seq_bases, seq_off, ops, ops_off, tmpl_bases, tmpl_off): the nodes' sequences and per-base ops, the chunks'
    sequences in `chunks` order.  Returns dict(err_num, err_len, status, rc); rc is -6 when a node failed (status per node)."""
    nodes = np.ascontiguousarray(nodes, dtype=ffi.CC_NODE_DT)
    node_off = np.ascontiguousarray(node_off, dtype=np.uint64)
    _flat_chunks(chunks)
    sb, so, ob, oo, tb, to = _sequences(seqs)
    n = len(nodes)
    num, length = np.zeros(n + 1, dtype=np.uint32), np.zeros(n + 1, dtype=np.uint32)
    status = np.zeros(n + 1, dtype=np.int32)
    rc = ffi.lib().jtk_lc_node_errors(len(node_off) - 1, u64p(node_off), nodes.ctypes.data, len(chunks), chunks.ctypes.data, u8p(sb),
                                      u64p(so), u8p(ob), u64p(oo), u8p(tb), u64p(to), u32p(num), u32p(length),
                                      status.ctypes.data_as(C.POINTER(C.c_int32)), device)
    if rc != 0 and (raise_on_node_failure or rc != -6):
        check(rc)
    return dict(err_num=num[:n], err_len=length[:n], status=status[:n], rc=rc)


def error_quantile(err_num, err_len, quantile, device=0):
    """jtk_lc_error_quantile: calc_sim_thr (determine_chunks.rs:806-823) on the nodes' error counts."""
    err_num = np.ascontiguousarray(err_num, dtype=np.uint32)
    err_len = np.ascontiguousarray(err_len, dtype=np.uint32)
    if len(err_num) != len(err_len):
        raise ValueError("err_num and err_len differ in length")
    out = C.c_double(0.0)
    check(ffi.lib().jtk_lc_error_quantile(len(err_num), u32p(err_num), u32p(err_len), float(quantile), C.byref(out), device))
    return out.value


def estimate_error_rate(node_off, nodes, err_num, err_len, chunks, fallback, device=0):
    """jtk_lc_estimate_error_rate: estimate_error_rate (estimate_error_rate.rs:37-133).  Returns dict(read_err, chunk_err,
    chunk_err_off, median_of_sqrt_err, n_iter): one rate per read, one per (chunk, cluster) flat in `chunks` order."""
    nodes = np.ascontiguousarray(nodes, dtype=ffi.CC_NODE_DT)
    node_off = np.ascontiguousarray(node_off, dtype=np.uint64)
    err_num = np.ascontiguousarray(err_num, dtype=np.uint32)
    err_len = np.ascontiguousarray(err_len, dtype=np.uint32)
    _flat_chunks(chunks)
    if not len(err_num) == len(err_len) == len(nodes):
        raise ValueError("err_num / err_len need one entry per node")
    n_reads, cap = len(node_off) - 1, int(chunks["cluster_num"].astype(np.uint64).sum())
    read_err, chunk_err = np.zeros(n_reads + 1, dtype=np.float64), np.zeros(cap + 1, dtype=np.float64)
    off = np.zeros(len(chunks) + 1, dtype=np.uint64)
    median, n_iter = C.c_double(0.0), C.c_uint32(0)
    check(ffi.lib().jtk_lc_estimate_error_rate(n_reads, u64p(node_off), nodes.ctypes.data, u32p(err_num), u32p(err_len), len(chunks),
                                               chunks.ctypes.data, float(fallback), f64p(read_err), f64p(chunk_err), u64p(off), cap,
                                               C.byref(median), C.byref(n_iter), device))
    return dict(read_err=read_err[:n_reads], chunk_err=chunk_err[:cap], chunk_err_off=off, median_of_sqrt_err=median.value,
                n_iter=n_iter.value)


def purge_diverged(node_off, nodes, n_post, chunks, seqs, thr=0.1, device=0):
    """jtk_lc_purge_diverged: purge_diverged_nodes (purge_diverged.rs:238-322) on the flattened data set of correct_clustering
    plus `seqs` (see node_errors); thr defaults to the reference's THR.  `chunks` (ffi.CC_CHUNK_DT) is updated in place
    (cluster_num).  Returns dict(diverged, chunk_err_off, keep, cluster, touched, post_keep, purged, read_err, chunk_err,
    median_of_sqrt_err): the flag per (chunk, cluster) flat in `chunks` order, per node whether it stays, its new cluster and
    whether it is rewritten, per posterior entry whether it stays, and the ids of the chunks that lost a cluster."""
    nodes = np.ascontiguousarray(nodes, dtype=ffi.CC_NODE_DT)
    node_off = np.ascontiguousarray(node_off, dtype=np.uint64)
    _flat_chunks(chunks)
    sb, so, ob, oo, tb, to = _sequences(seqs)
    n, n_reads, m, n_post = len(nodes), len(node_off) - 1, len(chunks), int(n_post)
    cap = int(chunks["cluster_num"].astype(np.uint64).sum())
    diverged, off = np.zeros(cap + 1, dtype=np.uint8), np.zeros(m + 1, dtype=np.uint64)
    keep, cluster, touched = np.zeros(n + 1, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint8)
    post_keep, purged = np.zeros(n_post + 1, dtype=np.uint8), np.zeros(m + 1, dtype=np.uint64)
    read_err, chunk_err = np.zeros(n_reads + 1, dtype=np.float64), np.zeros(cap + 1, dtype=np.float64)
    n_purged, median = C.c_size_t(0), C.c_double(0.0)
    check(ffi.lib().jtk_lc_purge_diverged(n_reads, u64p(node_off), nodes.ctypes.data, n_post, m, chunks.ctypes.data, u8p(sb), u64p(so),
                                          u8p(ob), u64p(oo), u8p(tb), u64p(to), float(thr), u8p(diverged), u64p(off), cap, u8p(keep),
                                          u64p(cluster), u8p(touched), u8p(post_keep), u64p(purged), m, C.byref(n_purged),
                                          f64p(read_err), f64p(chunk_err), C.byref(median), device))
    return dict(diverged=diverged[:cap], chunk_err_off=off, keep=keep[:n], cluster=cluster[:n], touched=touched[:n],
                post_keep=post_keep[:n_post], purged=purged[:n_purged.value], read_err=read_err[:n_reads], chunk_err=chunk_err[:cap],
                median_of_sqrt_err=median.value)


def purge_timing():
    """jtk_lc_debug_purge_timing (include/jtk_lc_debug.h): upload ms, column-walk ms, device ms and fit passes of the last call"""
    f = ffi.lib().jtk_lc_debug_purge_timing
    f.restype, f.argtypes = None, [C.POINTER(C.c_double)]
    out = (C.c_double * 4)()
    f(out)
    return dict(upload_ms=out[0], walk_ms=out[1], device_ms=out[2], n_iter=int(out[3]))


def settle_nodes(node_off, nodes, ops, ops_off, mode=ffi.SETTLE_BY_CHUNK_POS, device=0):
    """jtk_lc_settle_nodes: the node statistics and, unless mode is ffi.SETTLE_STATS_ONLY, the list surgery of
    correct_deletion_error (encode/deletion_fill.rs:349-361): a stable sort by (chunk, position) -- ffi.SETTLE_BY_CHUNK: by chunk
    alone, as re_encode_read does -- remove_slippy_alignment, a stable sort by position, remove_slippy_alignment,
    remove_overlapping_encoding.  nodes (ffi.SETTLE_NODE_DT) lists read r's nodes at node_off[r] .. node_off[r+1]; ops holds node
    e's per-base cigar at ops_off[e] .. ops_off[e+1].  Returns dict(stats, keep, order, n_kept, status, rc): stats
    (ffi.NODE_STATS_DT) and keep per node, order = per read the indices (inside the read) of its surviving nodes in their final
    order, n_kept and status per read.  rc is 0, or -6 where a read was left as it came (status[r] != 0: a node without ops or
    whose ops do not take query_len bases); every other failure raises."""
    nodes = np.ascontiguousarray(nodes, dtype=ffi.SETTLE_NODE_DT)
    node_off = np.ascontiguousarray(node_off, dtype=np.uint64)
    ops, ops_off = np.ascontiguousarray(ops, dtype=np.uint8), np.ascontiguousarray(ops_off, dtype=np.uint64)
    if len(node_off) == 0 or int(node_off[-1]) != len(nodes):
        raise ValueError("node_off must hold n_reads + 1 offsets that end at len(nodes)")
    if len(ops_off) != len(nodes) + 1 or int(ops_off[-1]) != len(ops):
        raise ValueError("ops_off must hold one offset per node and one more, ending at len(ops)")
    n_reads, n = len(node_off) - 1, len(nodes)
    stats, keep = np.zeros(n + 1, dtype=ffi.NODE_STATS_DT), np.zeros(n + 1, dtype=np.uint8)
    order, n_kept = np.zeros(n + 1, dtype=np.uint32), np.zeros(n_reads + 1, dtype=np.uint32)
    status = np.zeros(n_reads + 1, dtype=np.int32)
    rc = ffi.lib().jtk_lc_settle_nodes(n_reads, u64p(node_off), nodes.ctypes.data, u8p(ops), u64p(ops_off), int(mode), stats.ctypes.data,
                                       u32p(n_kept), u32p(order), u8p(keep), status.ctypes.data_as(C.POINTER(C.c_int32)), device)
    if rc != 0 and rc != -6:
        check(rc)
    per_read = [order[int(node_off[r]):int(node_off[r]) + int(n_kept[r])].copy() for r in range(n_reads)]
    return dict(stats=stats[:n], keep=keep[:n], order=per_read, n_kept=n_kept[:n_reads], status=status[:n_reads], rc=rc)


def settle_timing():
    """jtk_lc_debug_settle_timing (include/jtk_lc_debug.h): reads, reads whose work area lay in global memory, kernel ms and ms
    of the whole call on its stream, of the last settle_nodes call"""
    out = (C.c_double * 4)()
    ffi.lib().jtk_lc_debug_settle_timing(out)
    return dict(n_reads=int(out[0]), n_global=int(out[1]), kernel_ms=out[2], call_ms=out[3])


def _flat_seqs(seqs):
    """bytes back to back and their n + 1 offsets"""
    seqs = [bytes(s) for s in seqs]
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    if seqs:
        off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    bases = np.frombuffer(b"".join(seqs), dtype=np.uint8).copy() if int(off[-1]) else np.zeros(0, dtype=np.uint8)
    return seqs, bases, off


def mask_repeats(reads, k, freq, min_count, device=0, mask_cap=None):
    """jtk_lc_mask_repeats, `ds.mask_repeat` (repeat_masking.rs:135-158), on a list of bytes: every read upper-cased, the
    canonical k-mers of all reads counted, create_mask's percentile over the counts, and every base that a masked k-mer covers
    lower-cased.  Returns (the masked reads, the report, the mask's k-mers ascending): the report is a dict of
    ffi.MASK_REPORT_DT's fields and rc -- 0, or -6 where the reference panics (no k-mer counted twice, or 1.0 - freq == 1.0): the
    reads are then upper-cased and no more.  mask_cap: the capacity offered for the mask first (default 1,024; a mask that does
    not fit is fetched with a second call); every other failure raises."""
    seqs, bases, off = _flat_seqs(reads)
    masked = np.zeros(max(len(bases), 1), dtype=np.uint8)
    report = np.zeros(1, dtype=ffi.MASK_REPORT_DT)
    cap = 1024 if mask_cap is None else int(mask_cap)
    while True:
        kmers = np.zeros(max(cap, 1), dtype=np.uint64)
        rc = ffi.lib().jtk_lc_mask_repeats(len(seqs), u8p(bases), u64p(off), int(k), float(freq), int(min_count), u8p(masked), u64p(kmers), cap,
                                           report.ctypes.data, device)
        need = int(report["n_masked_kmers"][0])
        if rc == -1 and need > cap:
            cap = need
            continue
        break
    if rc != 0 and rc != -6:
        check(rc)
    out = dict((name, int(report[name][0])) for name in ffi.MASK_REPORT_DT.names)
    out["rc"] = rc
    raw = masked.tobytes()
    return [raw[int(off[i]):int(off[i + 1])] for i in range(len(seqs))], out, kmers[:need].copy()


def mask_timing():
    """jtk_lc_debug_mask_timing (include/jtk_lc_debug.h): HIP-event ms of the last mask_repeats call's four phases"""
    out = (C.c_double * 4)()
    ffi.lib().jtk_lc_debug_mask_timing(out)
    return dict(emit_ms=out[0], sort_ms=out[1], select_ms=out[2], apply_ms=out[3])


def repetitive_kmers(reads, k, device=0, cap=None):
    """jtk_lc_repetitive_kmers, get_repetitive_kmer (repeat_masking.rs:109-134): the k-mers of every window of `reads` (bytes, as
    given) whose bytes are all ASCII lower case, ascending and unique (np.uint64)"""
    seqs, bases, off = _flat_seqs(reads)
    cap = 1024 if cap is None else int(cap)
    n = C.c_uint64(0)
    while True:
        kmers = np.zeros(max(cap, 1), dtype=np.uint64)
        rc = ffi.lib().jtk_lc_repetitive_kmers(len(seqs), u8p(bases), u64p(off), int(k), u64p(kmers), cap, C.byref(n), device)
        if rc == -1 and n.value > cap:
            cap = n.value
            continue
        break
    check(rc)
    return kmers[:n.value].copy()


def repetitiveness(seqs, k, kmers, device=0, parts=False):
    """jtk_lc_repetitiveness, RepeatAnnot::repetitiveness (repeat_masking.rs:90-105) of every sequence (bytes) against the
    ascending, unique k-mers `kmers`: np.float64 rep_num / rep_den; parts=True: (rep_num, rep_den) as np.uint32.  A call of the
    library takes as many sequences as have an index that fits above the k-mer in 64 bits (four at k = 31): more go in several."""
    seqs = [bytes(s) for s in seqs]
    kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
    num, den = np.zeros(len(seqs), dtype=np.uint32), np.zeros(len(seqs), dtype=np.uint32)
    per_call = 1 << (64 - 2 * int(k)) if 16 < int(k) <= ffi.MASK_MAX_K else max(len(seqs), 1)
    for first in range(0, max(len(seqs), 1), per_call):
        part, bases, off = _flat_seqs(seqs[first:first + per_call])
        n, d = np.zeros(len(part) + 1, dtype=np.uint32), np.zeros(len(part) + 1, dtype=np.uint32)
        check(ffi.lib().jtk_lc_repetitiveness(len(part), u8p(bases), u64p(off), int(k), u64p(kmers), len(kmers), u32p(n), u32p(d), device))
        num[first:first + len(part)], den[first:first + len(part)] = n[:len(part)], d[:len(part)]
    return (num, den) if parts else num.astype(np.float64) / den.astype(np.float64)


def sketch(seqs, k=15, w=10, device=0, cap=None):
    """jtk_lc_sketch: the minimizers of every sequence (bytes) by DESIGN.md section 4 "Seeding and chaining" -- canonical k-mers,
    the invertible hash, windows of w positions, every position that attains a window's minimum -- ascending by (seq, pos).
    -> dict(hash (np.uint64), seq, pos (np.uint32), strand (np.uint8)).  Own specification: parity with minimap2's seeds is not
    pinned."""
    seqs, bases, off = _flat_seqs(seqs)
    cap = 1024 if cap is None else int(cap)
    n = C.c_uint64(0)
    while True:
        size = max(cap, 1)
        h, s, p, st = np.zeros(size, np.uint64), np.zeros(size, np.uint32), np.zeros(size, np.uint32), np.zeros(size, np.uint8)
        rc = ffi.lib().jtk_lc_sketch(len(seqs), u8p(bases), u64p(off), int(k), int(w), u64p(h), u32p(s), u32p(p), u8p(st), cap, C.byref(n), device)
        if rc == -1 and n.value > cap:
            cap = n.value
            continue
        break
    check(rc)
    m = n.value
    return dict(hash=h[:m].copy(), seq=s[:m].copy(), pos=p[:m].copy(), strand=st[:m].copy())


def map_reads(targets, queries, k=15, w=10, max_occ=200, max_gap=100, min_seeds=4, skip_self=False, device=0, cap=None):
    """jtk_lc_map_reads: where every target (a chunk; bytes) lies in every query (a read; bytes) -- what the reference asks an
    external minimap2 process (encode/mod.rs:41-64, :315-355).  Minimizers of both sides (sketch), hits of equal hash (hashes that
    occur more than max_occ times among the targets are not used), diag = q' - tpos on the oriented query, single-linkage
    clusters along the diagonal (a gap above max_gap starts a new one), one placement per cluster of at least min_seeds distinct
    target positions.  skip_self: query i against target i yields nothing (minimap2's -X).
    -> np.ndarray of ffi.MAP_PLACEMENT_DT in the order (query, target, reverse after forward, diag_lo).  cap: the capacity offered
    first (default 1,024; more placements are fetched with a second call).  A placement is a seed cluster, not an alignment:
    map_trials and encode_nodes make a node of it.  Own specification: parity with minimap2's choice of
    seeds and chains is not pinned."""
    _, tb, toff = _flat_seqs(targets)
    _, qb, qoff = _flat_seqs(queries)
    params = np.array([(int(k), int(w), int(max_occ), int(max_gap), int(min_seeds), 1 if skip_self else 0)], dtype=ffi.MAP_PARAMS_DT)
    cap = 1024 if cap is None else int(cap)
    n = C.c_uint64(0)
    while True:
        out = np.zeros(max(cap, 1), dtype=ffi.MAP_PLACEMENT_DT)
        rc = ffi.lib().jtk_lc_map_reads(len(toff) - 1, u8p(tb), u64p(toff), len(qoff) - 1, u8p(qb), u64p(qoff), params.ctypes.data, out.ctypes.data,
                                        cap, C.byref(n), device)
        if rc == -1 and n.value > cap:
            cap = n.value
            continue
        break
    check(rc)
    return out[:n.value].copy()


def map_timing():
    """jtk_lc_debug_map_timing (include/jtk_lc_debug.h): HIP-event ms of the last map_reads call's six phases, two counts, and
    the ms of the two sketch kernels alone (the sketch phase also holds the upload and a wait)"""
    out = (C.c_double * 10)()
    ffi.lib().jtk_lc_debug_map_timing(out)
    return dict(sketch_ms=out[0], index_ms=out[1], hits_ms=out[2], order_ms=out[3], chain_ms=out[4], compact_ms=out[5],
                n_minimizers=int(out[6]), n_hits=int(out[7]), sketch_kernel_ms=out[8])


ALLOWED_END_GAP = 25     # encode/mod.rs:14


def map_trials(placements, query_lens, target_lens, sim_thr):
    """The window of a read that encode_node is tried on for every placement of map_reads; pure host arithmetic, no GPU.  The
    chunk's ends are projected along the placement onto the oriented read: est_start = oq_start - tstart, est_end = oq_end +
    (tlen - tend).  A placement whose estimate leaves the read by more than ALLOWED_END_GAP bases at either end is dropped -- the
    reference's filter `tstart < 25 && tlen - tend < 25` (encode/mod.rs:46) asks the aligner to have reached the chunk's ends,
    a seed cluster cannot, so the question becomes whether the read holds the whole chunk.  The estimate is widened by
    ceil(OFFSET_FACTOR * tlen) per side (as fill_trials does), clipped to the read and turned into forward coordinates, as
    jtk_encode_trial_t wants them.  -> list of (index of the placement, start, end, is_forward, sim_thr)."""
    import math
    out = []
    for i, p in enumerate(placements):
        qlen, tlen = int(query_lens[int(p["query"])]), int(target_lens[int(p["target"])])
        est_start = int(p["oq_start"]) - int(p["tstart"])
        est_end = int(p["oq_end"]) + (tlen - int(p["tend"]))
        if est_start < -ALLOWED_END_GAP or est_end > qlen + ALLOWED_END_GAP:
            continue
        offset = math.ceil(OFFSET_FACTOR * float(tlen))
        start, end = max(est_start - offset, 0), min(est_end + offset, qlen)
        if not start < end:
            continue
        forward = bool(p["is_forward"])
        if not forward:
            start, end = qlen - end, qlen - start
        out.append((i, start, end, 1 if forward else 0, float(sim_thr)))
    return out


def _fill_reads(node_off, nodes):
    nodes = np.ascontiguousarray(nodes, dtype=ffi.FILL_NODE_DT)
    node_off = np.ascontiguousarray(node_off, dtype=np.uint64)
    if len(node_off) == 0 or int(node_off[-1]) != len(nodes):
        raise ValueError("node_off must hold n_reads + 1 offsets that end at len(nodes)")
    return node_off, nodes


def fill_candidates(node_off, nodes, target=None, device=0, cand_cap=None):
    """jtk_lc_fill_candidates: get_pileup, ins_thr and check_insertion_head / _tail of correct_deletion
    (encode/deletion_fill.rs:301-337, 642-698, 883-981) for the reads nodes[node_off[r] .. node_off[r+1]) (ffi.FILL_NODE_DT).
    target: None, or per read 1 = compute it.  Returns dict(coverage, ins_thr, cand_off, cands): coverage flat with read r's
    n + 1 slots at node_off[r] + r, cands (ffi.FILL_CAND_DT) in (read, slot, side, chunk, cluster, is_forward) order.  The
    candidate array is grown once on the capacity reply (cand_cap: its first size, default one per node)."""
    node_off, nodes = _fill_reads(node_off, nodes)
    n_reads, n = len(node_off) - 1, len(nodes)
    tgt = None
    if target is not None:
        tgt = np.ascontiguousarray(target, dtype=np.uint8)
        if len(tgt) != n_reads:
            raise ValueError("target must hold one entry per read")
    coverage, ins_thr = np.zeros(n + n_reads + 1, dtype=np.uint32), np.zeros(n_reads + 1, dtype=np.uint32)
    cand_off = np.zeros(n_reads + 1, dtype=np.uint64)
    cap = n if cand_cap is None else int(cand_cap)
    need = C.c_size_t(0)
    L = ffi.lib()
    for attempt in range(2):
        cands = np.zeros(cap + 1, dtype=ffi.FILL_CAND_DT)
        rc = L.jtk_lc_fill_candidates(n_reads, u64p(node_off), nodes.ctypes.data, None if tgt is None else u8p(tgt), u32p(coverage),
                                      u32p(ins_thr), u64p(cand_off), cands.ctypes.data, cap, C.byref(need), device)
        if rc == -1 and attempt == 0 and need.value > cap:
            cap = need.value
            continue
        check(rc)
        break
    return dict(coverage=coverage[:n + n_reads], ins_thr=ins_thr[:n_reads], cand_off=cand_off, cands=cands[:need.value])


def fill_pairs(node_off, nodes, pair_target, pair_query, device=0):
    """jtk_lc_debug_fill_pairs (include/jtk_lc_debug.h): per (target, query) pair the direction (1 forward, 0 reverse, -1 = the
    pre-filter rejects it), the score, the pass flag and the compressed ops as a list of (code, length)."""
    node_off, nodes = _fill_reads(node_off, nodes)
    pt, pq = np.ascontiguousarray(pair_target, dtype=np.uint32), np.ascontiguousarray(pair_query, dtype=np.uint32)
    n_pairs = len(pt)
    length = np.diff(node_off.astype(np.int64))
    cap = int(sum(int(length[t]) + int(length[q]) + 2 for t, q in zip(pt, pq) if t < len(length) and q < len(length)))
    direction, score = np.zeros(n_pairs + 1, dtype=np.int32), np.zeros(n_pairs + 1, dtype=np.int32)
    passed, ops_off, ops = np.zeros(n_pairs + 1, dtype=np.uint8), np.zeros(n_pairs + 1, dtype=np.uint64), np.zeros(cap + 1, dtype=np.uint32)
    n_ops = C.c_size_t(0)
    check(ffi.lib().jtk_lc_debug_fill_pairs(len(node_off) - 1, u64p(node_off), nodes.ctypes.data, n_pairs, u32p(pt), u32p(pq),
                                            direction.ctypes.data_as(C.POINTER(C.c_int32)), score.ctypes.data_as(C.POINTER(C.c_int32)),
                                            u8p(passed), u64p(ops_off), u32p(ops), cap, C.byref(n_ops), device))
    runs = [[(int(o) & 3, int(o) >> 2) for o in ops[int(ops_off[p]):int(ops_off[p + 1])]] for p in range(n_pairs)]
    return dict(dir=direction[:n_pairs], score=score[:n_pairs], passed=passed[:n_pairs], ops=runs)


def fill_timing():
    """jtk_lc_debug_fill_timing (include/jtk_lc_debug.h): pairs aligned, insertion records, device ms and pair-kernel ms of the
    last fill_candidates call"""
    out = (C.c_double * 4)()
    ffi.lib().jtk_lc_debug_fill_timing(out)
    return dict(n_pairs=int(out[0]), n_records=int(out[1]), device_ms=out[2], pair_ms=out[3])


ALN_PARAMETER = (2, -6, -5, -1)     # (match, mismatch, open, ext): haplotyper's ALN_PARAMETER


def _flat(seqs, dtype=np.uint8):
    """sequences (bytes / arrays) back to back -> (buffer, offsets)"""
    arrs = [np.frombuffer(s, dtype=np.uint8) if isinstance(s, (bytes, bytearray)) else np.asarray(s, dtype=dtype) for s in seqs]
    off = np.zeros(len(arrs) + 1, dtype=np.uint64)
    if arrs:
        off[1:] = np.cumsum([len(a) for a in arrs])
    buf = np.concatenate(arrs).astype(dtype) if arrs else np.zeros(0, dtype)
    return np.ascontiguousarray(np.append(buf, dtype(0))), off      # one spare byte: never a null pointer


def align_guided(pairs, x_bases, y_bases, guide_ops, mode="global", scores=ALN_PARAMETER, device=0, raise_on_pair_failure=True):
    """jtk_lc_align_guided: banded affine-gap alignment of every pair (ffi.GUIDED_PAIR_DT: offsets and lengths into x_bases,
    y_bases, guide_ops, and a radius) along its guide, mode "global" or "infix" (both ends of x free).
    -> dict(score, start, end, status, ops, ops_off, rc).  The aligner is this build's own specification:
    parity with kiley's guided alignment is not pinned."""
    if mode not in ("global", "infix"):
        raise ValueError("mode is global or infix")
    pairs = np.ascontiguousarray(pairs, dtype=ffi.GUIDED_PAIR_DT)
    n = len(pairs)
    xb, yb, gb = (np.ascontiguousarray(np.append(np.asarray(a, dtype=np.uint8), np.uint8(0))) for a in (x_bases, y_bases, guide_ops))
    cap = int(pairs["x_len"].astype(np.int64).sum() + pairs["y_len"].astype(np.int64).sum()) + 1
    ops, ops_off = np.zeros(cap, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64)
    score, status = np.zeros(n + 1, dtype=np.int32), np.zeros(n + 1, dtype=np.int32)
    start, end = np.zeros(n + 1, dtype=np.uint32), np.zeros(n + 1, dtype=np.uint32)
    PI32 = C.POINTER(C.c_int32)
    rc = ffi.lib().jtk_lc_align_guided(n, pairs.ctypes.data, u8p(xb), u8p(yb), u8p(gb), ALIGN_MODES[mode], *[int(s) for s in scores],
                                       u8p(ops), u64p(ops_off), cap, score.ctypes.data_as(PI32), u32p(start), u32p(end),
                                       status.ctypes.data_as(PI32), device)
    if rc != 0 and (raise_on_pair_failure or rc != -6):
        check(rc)
    return dict(score=score[:n], start=start[:n], end=end[:n], status=status[:n], ops=ops[:int(ops_off[n])], ops_off=ops_off, rc=rc)


def align_guided_seqs(items, mode="global", scores=ALN_PARAMETER, device=0, raise_on_pair_failure=True):
    """align_guided for a list of (x, y, guide, radius) with sequences as bytes: every pair gets buffers of its own."""
    xb, xo = _flat([it[0] for it in items])
    yb, yo = _flat([it[1] for it in items])
    gb, go = _flat([it[2] for it in items])
    pairs = np.zeros(len(items), dtype=ffi.GUIDED_PAIR_DT)
    for p, it in enumerate(items):
        pairs[p] = (xo[p], yo[p], go[p], len(it[0]), len(it[1]), len(it[2]), it[3])
    return align_guided(pairs, xb, yb, gb, mode=mode, scores=scores, device=device, raise_on_pair_failure=raise_on_pair_failure)


def guided_scratch_cap(n_bytes):
    """jtk_lc_debug_guided_scratch_cap (include/jtk_lc_debug.h): the work-area budget of the guided aligner on this thread; 0
    restores the default.  A test hook: a small budget cuts a small batch into several slices."""
    ffi.lib().jtk_lc_debug_guided_scratch_cap(int(n_bytes))


def guided_timing():
    """jtk_lc_debug_guided_timing: pairs, cells filled, kernel ms and slices of the last align_guided call"""
    out = (C.c_double * 4)()
    ffi.lib().jtk_lc_debug_guided_timing(out)
    return dict(n_pairs=int(out[0]), cells=int(out[1]), kernel_ms=out[2], slices=int(out[3]))


def polish_guided(batch, radius, take_num=0, ignore_edge=0, max_rounds=0, device=0, raise_on_chunk_failure=True):
    """jtk_lc_polish_guided: the consensus polish that votes with banded edit distances (what the reference gets from kiley's
    `bialignment::guided::polish_until_converge`), on every pile-up of `batch`; strands, copy numbers and ids play no part.
    radius: one band radius for all pile-ups or one per pile-up; take_num = 0: every read votes; max_rounds = 0: 20.
    -> dict(cons, cons_off, ops_out, ops_out_off, dist, result, rc).  The polish is this build's own specification (DESIGN.md
    section 4, "Guided polishing"): parity with kiley's polish is not pinned."""
    n_chunks, n_reads = batch.n_chunks, len(batch.read_off) - 1
    rad = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.uint32), (n_chunks,)))
    result = np.zeros(n_chunks + 1, dtype=ffi.RESULT_DT)
    tl = batch.chunks["tmpl_len"].astype(np.int64)
    cons_cap = int((tl + 64 + tl // 8).sum()) + 1
    rl = np.diff(batch.read_off.astype(np.int64))
    ops_cap = int((np.repeat(tl + 64 + tl // 8, batch.chunks["n_reads"].astype(np.int64))).sum() + rl.sum()) + 1
    cons, cons_off = np.zeros(cons_cap, dtype=np.uint8), np.zeros(n_chunks + 1, dtype=np.uint64)
    ops_out, ops_out_off = np.zeros(ops_cap, dtype=np.uint8), np.zeros(n_reads + 1, dtype=np.uint64)
    dist = np.zeros(n_reads + 1, dtype=np.uint32)
    tb, rb, ob = (np.ascontiguousarray(np.append(np.asarray(a, dtype=np.uint8), np.uint8(0))) for a in (batch.tmpl_bases, batch.read_bases, batch.ops))
    rc = ffi.lib().jtk_lc_polish_guided(n_chunks, batch.chunks.ctypes.data, u8p(tb), u8p(rb), u64p(batch.read_off), u8p(ob), u64p(batch.ops_off),
                                        u32p(np.append(rad, np.uint32(0))), int(take_num), int(ignore_edge), int(max_rounds), u8p(cons),
                                        u64p(cons_off), cons_cap, u8p(ops_out), u64p(ops_out_off), ops_cap, u32p(dist), result.ctypes.data, device)
    if rc != 0 and (raise_on_chunk_failure or rc != -6):
        check(rc)
    return dict(cons=cons, cons_off=cons_off, ops_out=ops_out, ops_out_off=ops_out_off, dist=dist[:n_reads], result=result[:n_chunks], rc=rc)


def guided_table(tmpl, reads, opss, radius, device=0):
    """jtk_lc_debug_guided_table (include/jtk_lc_debug.h): one round's fill of polish_guided for one pile-up, nothing applied.
    -> (dist [n_reads] uint32, table [n_reads, len(tmpl) + 1, 14] uint32 with 0xFFFFFFFF for a dead entry).  A test hook."""
    tmpl = np.frombuffer(tmpl, dtype=np.uint8) if isinstance(tmpl, (bytes, bytearray)) else np.asarray(tmpl, dtype=np.uint8)
    rb, ro = _flat(reads)
    ob, oo = _flat(opss)
    n, nr = len(tmpl), len(reads)
    dist = np.zeros(nr + 1, dtype=np.uint32)
    table = np.zeros((nr, n + 1, ffi.NUM_ROW), dtype=np.uint32)
    tb = np.ascontiguousarray(np.append(tmpl, np.uint8(0)))
    check(ffi.lib().jtk_lc_debug_guided_table(u8p(tb), n, nr, u8p(rb), u64p(ro), u8p(ob), u64p(oo), int(radius), u32p(dist), u32p(table),
                                              (n + 1) * ffi.NUM_ROW, device))
    return dist[:nr], table


def filter_stage(params, chunks, mode, device=0):
    """jtk_lc_debug_filter (include/jtk_lc_debug.h): the variant filter of a clustering pass on planted input.  A test hook.
    chunks: dicts with `tmpl` (ASCII bases), `strands` (one per read), `copy_num` and, for mode ffi.DEBUG_FILTER_TABLE, `table`
    [n, 14 (L + 1)] (minus lk); for the two row-sum modes `rows` [n, L + 1, 16], `exps` [n, L + 1] and `lk` [n].
    -> per chunk dict(cand [14 (L + 1)], dim, pos [dim], vtype [dim, 2], feat [n, dim], n_cand, order [picks]: the picked
    candidates' indices among the candidates in pick order)"""
    rows = mode != ffi.DEBUG_FILTER_TABLE
    rec = np.zeros(len(chunks) + 1, dtype=ffi.CHUNK_DT)
    tmpl, strand, values, exps, lk = [], [], [], [], []
    n_reads = n_bases = 0
    for c, ch in enumerate(chunks):
        t = np.frombuffer(ch["tmpl"], dtype=np.uint8) if isinstance(ch["tmpl"], (bytes, bytearray)) else np.asarray(ch["tmpl"], dtype=np.uint8)
        n, L = len(ch["strands"]), len(t)
        rec[c] = (c, ch["copy_num"], n, n_bases, L, n_reads)
        tmpl.append(t)
        strand.append(np.asarray(ch["strands"], dtype=np.uint8))
        if rows:
            assert np.shape(ch["rows"]) == (n, L + 1, 16) and np.shape(ch["exps"]) == (n, L + 1) and np.shape(ch["lk"]) == (n,)
            values.append(np.asarray(ch["rows"], dtype=np.float64).ravel())
            exps.append(np.asarray(ch["exps"], dtype=np.int32).ravel())
            lk.append(np.asarray(ch["lk"], dtype=np.float64))
        else:
            assert np.shape(ch["table"]) == (n, ffi.NUM_ROW * (L + 1))
            values.append(np.asarray(ch["table"], dtype=np.float64).ravel())
        n_reads, n_bases = n_reads + n, n_bases + L
    cat = lambda xs, dt: np.ascontiguousarray(np.concatenate(xs + [np.zeros(1, dtype=dt)]))  # noqa: E731
    tb, st, va = cat(tmpl, np.uint8), cat(strand, np.uint8), cat(values, np.float64)
    ex, lks = cat(exps, np.int32), cat(lk, np.float64)
    n_chunks, W = len(chunks), ffi.DEBUG_FILTER_TRACE_WORDS
    cand = np.zeros(ffi.NUM_ROW * (n_bases + n_chunks) + 1)
    dim, pos, vtype = np.zeros(n_chunks + 1, dtype=np.uint32), np.zeros((n_chunks + 1, ffi.MAX_DIM), dtype=np.uint32), np.zeros((n_chunks + 1, ffi.MAX_DIM, 2), dtype=np.uint32)
    feat, trace = np.zeros(n_reads * ffi.MAX_DIM + 1), np.zeros((n_chunks + 1, W), dtype=np.uint32)
    check(ffi.lib().jtk_lc_debug_filter(C.byref(params), n_chunks, rec.ctypes.data, u8p(tb), u8p(st), int(mode), f64p(va),
                                        ex.ctypes.data_as(C.POINTER(C.c_int32)) if rows else None, f64p(lks) if rows else None, f64p(cand),
                                        u32p(dim), u32p(pos), u32p(vtype), f64p(feat), u32p(trace), device))
    out, co = [], 0
    for c, ch in enumerate(chunks):
        n, L, first, d = int(rec["n_reads"][c]), int(rec["tmpl_len"][c]), int(rec["read_first"][c]), int(dim[c])
        cols = ffi.NUM_ROW * (L + 1)
        out.append(dict(cand=cand[co:co + cols].copy(), dim=d, pos=pos[c, :d].copy(), vtype=vtype[c, :d].copy(),
                        feat=feat[ffi.MAX_DIM * first:ffi.MAX_DIM * first + n * d].reshape(n, d).copy(), n_cand=int(trace[c, 0]),
                        order=trace[c, 2:2 + int(trace[c, 1])].copy()))
        co += cols
    return out


def gpolish_timing():
    """jtk_lc_debug_gpolish_timing: of the last polish_guided call, pile-ups, reads, rounds enqueued, band cells filled forward,
    kernel ms, the slices of the work area and the bytes all reads take of it by the host's bound"""
    out = (C.c_double * 8)()
    ffi.lib().jtk_lc_debug_gpolish_timing(out)
    return dict(n_chunks=int(out[0]), n_reads=int(out[1]), rounds=int(out[2]), cells=int(out[3]), kernel_ms=out[4], slices=int(out[5]),
                work_bytes=int(out[6]), vote_cells=int(out[7]))


def take_consensus(chunk_seqs, node_chunk, node_cluster, node_seqs, band_frac, device=0):
    """`take_consensus_sequence` (encode/deletion_fill.rs:260-285) for flat node arrays: the nodes are bucketed by (chunk, cluster)
    in the order given (that of encoded_reads); cluster 0 stands for the chunk's own sequence; any other bucket is polished from
    the chunk's sequence with its nodes' sequences -- global ops from align_reads, then polish_guided with radius =
    ReadType::band_width(len) = ceil(len * band_frac) (definitions/src/lib.rs:201-210).
    chunk_seqs: {chunk id: uint8 array}; band_frac: dataset.BAND_FRAC of the read type.
    -> {(chunk, cluster): uint8 array}, in bucket order: the cons_bases that the trials of encode_nodes take.  The polish is this
    build's own specification: parity with kiley's polish is not pinned."""
    import math
    from .batch import pack
    bucket = {}
    for cid, cl, seq in zip(node_chunk, node_cluster, node_seqs):
        bucket.setdefault((int(cid), int(cl)), []).append(np.asarray(seq, dtype=np.uint8))
    for cid, _ in bucket:
        if cid not in chunk_seqs:
            raise KeyError("take_consensus: a node of chunk %d, which has no sequence" % cid)
    todo = [key for key in bucket if key[1] != 0]
    polished = {}
    if todo:
        none = np.zeros(0, dtype=np.uint8)
        batch = pack([(key[0], 1, chunk_seqs[key[0]], bucket[key], [none] * len(bucket[key]), [1] * len(bucket[key]), None) for key in todo])
        aligned = align_reads(batch, device=device)
        radius = [max(1, math.ceil(len(chunk_seqs[key[0]]) * band_frac)) for key in todo]
        out = polish_guided(batch.with_ops(aligned["ops"], aligned["ops_off"]), radius, device=device)
        for c, key in enumerate(todo):
            polished[key] = out["cons"][int(out["cons_off"][c]):int(out["cons_off"][c + 1])].copy()
    return {key: (np.asarray(chunk_seqs[key[0]], dtype=np.uint8) if key[1] == 0 else polished[key]) for key in bucket}


def encode_nodes(trials, read_bases, cons_bases, chunk_bases, device=0, raise_on_trial_failure=True):
    """jtk_lc_encode_nodes: `encode_node` (encode/deletion_fill.rs:451-566) for every trial (ffi.ENCODE_TRIAL_DT).
    -> dict(result (ffi.ENCODE_RESULT_DT), ops, ops_off, rc); the caller runs kiley_op_to_ops on a trial's ops, takes seq from the
    window and keeps the best score among a slot's accepted trials."""
    trials = np.ascontiguousarray(trials, dtype=ffi.ENCODE_TRIAL_DT)
    n = len(trials)
    rb, cb, kb = (np.ascontiguousarray(np.append(np.asarray(a, dtype=np.uint8), np.uint8(0))) for a in (read_bases, cons_bases, chunk_bases))
    cap = int(trials["chunk_len"].astype(np.int64).sum() + (trials["end"].astype(np.int64) - trials["start"].astype(np.int64)).clip(0).sum()) + 1
    result = np.zeros(n + 1, dtype=ffi.ENCODE_RESULT_DT)
    ops, ops_off = np.zeros(cap, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64)
    rc = ffi.lib().jtk_lc_encode_nodes(n, trials.ctypes.data, u8p(rb), u8p(cb), u8p(kb), result.ctypes.data, u8p(ops), u64p(ops_off), cap, device)
    if rc != 0 and (raise_on_trial_failure or rc != -6):
        check(rc)
    return dict(result=result[:n], ops=ops[:int(ops_off[n])], ops_off=ops_off, rc=rc)


def encode_timing():
    """jtk_lc_debug_encode_timing: of the last encode_nodes call, the trials past the filter, kernel ms and cells of the three
    guided passes, host ms of the infix alignment"""
    out = (C.c_double * 8)()
    ffi.lib().jtk_lc_debug_encode_timing(out)
    return dict(n_live=int(out[0]), pass_ms=[out[1], out[2], out[3]], pass_cells=[int(out[4]), int(out[5]), int(out[6])], infix_host_ms=out[7])


OFFSET_FACTOR = 0.1     # deletion_fill.rs:293


def fill_trials(side, candidates, seq_len, next_node, cons_len_of):
    """The trial windows try_encoding_head / _tail (encode/deletion_fill.rs:370-446) make from a slot's candidates; pure host
    arithmetic, no GPU.
    side: 0 = head (the position is a start), 1 = tail (it is an end); candidates: (chunk, cluster, is_forward, position) each,
    position as jtk_lc_fill_candidates returns it (a negative head position is the reference's wrapped usize: rejected by
    `start_position < seq.len()`; a tail position is never negative there, and one that is raises ValueError, where the
    reference's wrapped value fails `assert!(start_position < end_position)`); seq_len: the raw read's length; next_node: None or (chunk, position_from_start) of
    nodes.get(idx); cons_len_of(chunk, cluster) -> the consensus length or None (no such chunk or consensus: skipped).
    -> list of (candidate index, start, end): the windows encode_node is tried on."""
    import math
    out = []
    for k, (chunk, cluster, _fw, position) in enumerate(candidates):
        if side == 0 and not (0 <= position < seq_len):
            continue
        if position < 0:
            raise ValueError("a negative tail position (jtk_lc_fill_candidates clamps them at 0; the reference's wrapped usize fails its assert)")
        cons_len = cons_len_of(chunk, cluster)
        if cons_len is None:
            continue
        offset = math.ceil(OFFSET_FACTOR * float(cons_len))
        if side == 0:
            end = min(position + cons_len + offset, seq_len)
            start = max(position - offset, 0)
        else:
            start = max(min(position, seq_len) - (offset + cons_len), 0)
            end = min(position + offset, seq_len)
        if not start < end:
            raise ValueError("start_position < end_position does not hold (the reference asserts)")
        if next_node is not None and next_node[0] == chunk and abs(next_node[1] - start) < cons_len:
            continue     # is_the_same_encode
        out.append((k, start, end))
    return out


_REVCMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def _as_bytes(s):
    return bytes(s) if isinstance(s, (bytes, bytearray)) else bytes(np.asarray(s, dtype=np.uint8))


def _oriented_window(read_bases, read_off, start, end, is_forward):
    """the window as tune_position takes it (dense_encoding.rs:722-727)"""
    w = bytes(np.asarray(read_bases[read_off + start:read_off + end], dtype=np.uint8)).upper()
    return w if is_forward else w.translate(_REVCMP)[::-1]


def encode_edges(trials, read_bases, contig_bases, break_points, device=0, raise_on_trial_failure=True):
    """jtk_lc_encode_edges: `encode_edge` with `tune_position` (dense_encoding.rs:627-759) for every trial (ffi.EDGE_TRIAL_DT).
    -> dict(result (ffi.EDGE_RESULT_DT, per trial), nodes (ffi.EDGE_NODE_DT, per slot: trial t's chunk k at node_off[t] + k),
    node_off, ops, ops_off (per slot), accepted, rc).  accepted[t] is what encode_edge returns for trial t: its accepted nodes as
    dict(chunk (index in the trial), position_from_start, seq, ops, mat_num, ops_len), reversed for a reverse trial (:693-695);
    the caller runs kiley_op_to_ops on the ops.  Both infix alignments and the guided pass are this build's own specification
    (DESIGN.md section 4): parity with edlib's choice among equal placements and with kiley is not pinned."""
    trials = np.ascontiguousarray(trials, dtype=ffi.EDGE_TRIAL_DT)
    n = len(trials)
    rb, cb = (np.ascontiguousarray(np.append(np.asarray(a, dtype=np.uint8), np.uint8(0))) for a in (read_bases, contig_bases))
    bp = np.ascontiguousarray(np.append(np.asarray(break_points, dtype=np.uint32), np.uint32(0)))
    node_off = np.zeros(n + 1, dtype=np.uint64)
    node_off[1:] = np.cumsum(trials["n_chunks"].astype(np.uint64))
    n_nodes = int(node_off[n])
    cap = int(trials["contig_len"].astype(np.int64).sum() + (trials["end"].astype(np.int64) - trials["start"].astype(np.int64)).clip(0).sum())
    result = np.zeros(n + 1, dtype=ffi.EDGE_RESULT_DT)
    nodes = np.zeros(n_nodes + 1, dtype=ffi.EDGE_NODE_DT)
    ops, ops_off = np.zeros(cap + 1, dtype=np.uint8), np.zeros(n_nodes + 1, dtype=np.uint64)
    rc = ffi.lib().jtk_lc_encode_edges(n, trials.ctypes.data, u8p(rb), u8p(cb), u32p(bp), u64p(node_off), result.ctypes.data, nodes.ctypes.data,
                                       u8p(ops), u64p(ops_off), cap, device)
    if rc != 0 and (raise_on_trial_failure or rc != -6):
        check(rc)
    accepted = []
    for t in range(n):
        tr, got = trials[t], []
        window = None
        for k in range(int(tr["n_chunks"])):
            e = int(node_off[t]) + k
            nd = nodes[e]
            if int(result[t]["status"]) != 0 or int(nd["verdict"]) != ffi.EDGE_ACCEPTED:
                continue
            if window is None:
                window = _oriented_window(rb, int(tr["read_off"]), int(tr["start"]), int(tr["end"]), bool(tr["is_forward"]))
            q = int(nd["query_off"])
            got.append(dict(chunk=k, position_from_start=int(nd["position_from_start"]), seq=window[q:q + int(nd["query_len"])],
                            ops=ops[int(ops_off[e]):int(ops_off[e + 1])].copy(), mat_num=int(nd["mat_num"]), ops_len=int(nd["ops_len"])))
        accepted.append(got if tr["is_forward"] else got[::-1])
    return dict(result=result[:n], nodes=nodes[:n_nodes], node_off=node_off, ops=ops[:int(ops_off[n_nodes])], ops_off=ops_off, accepted=accepted, rc=rc)


def edges_timing():
    """jtk_lc_debug_edges_timing: of the last encode_edges call, the trials, kernel ms, cells and slices of the guided pass, host ms
    of the two infix alignments, kernel ms of the cut and the pack"""
    out = (C.c_double * 8)()
    ffi.lib().jtk_lc_debug_edges_timing(out)
    return dict(n_trials=int(out[0]), pass_ms=out[1], pass_cells=int(out[2]), slices=int(out[3]), infix_host_ms=[out[4], out[5]], cut_ms=out[6])


def pack_edge_trials(items):
    """items: dict(read, start, end, is_forward, chunks (the edge's chunk sequences, in order), radius, sim_thr) each; sequences
    are bytes or uint8 arrays.  Every item gets buffers of its own.  -> (trials (ffi.EDGE_TRIAL_DT), read_bases, contig_bases,
    break_points): the arguments of encode_edges; the contig and its break points are merge_chunks' (dense_encoding.rs:595-609)."""
    reads = _flat([it["read"] for it in items])
    contigs = _flat([b"".join(_as_bytes(c) for c in it["chunks"])
                     for it in items])
    arr = np.zeros(len(items), dtype=ffi.EDGE_TRIAL_DT)
    breaks = []
    for k, it in enumerate(items):
        ends = np.cumsum([len(c) for c in it["chunks"]], dtype=np.int64)
        arr[k] = (reads[1][k], it["start"], it["end"], int(bool(it["is_forward"])), it["radius"], contigs[1][k], int(ends[-1]) if len(ends) else 0,
                  len(ends), len(breaks), it["sim_thr"])
        breaks.extend(int(e) for e in ends)
    return arr, reads[0], contigs[0], np.asarray(breaks, dtype=np.uint32)


EDGE_MARGIN = 25     # dense_encoding.rs:209


def edge_trials(nodes, seq_len, edges, tips, band_width_of, sim_thr):
    """`fill_edges_by_new_chunks` (dense_encoding.rs:202-293) up to its calls of encode_edge; pure host arithmetic, no GPU.
    nodes: the read's nodes in order, (chunk, cluster, is_forward, position_from_start, seq length) each; seq_len: the raw read's
    length; edges: {((chunk, cluster, is_forward), (chunk, cluster, is_forward)): [chunk sequence, ...]}; tips: {(chunk, cluster,
    is_forward, is_tail): [[chunk sequence, ...], ...]}, both keyed as the reference's EdgeAndUnit and TipAndUnit;
    band_width_of(contig_len) -> the radius (read_type.band_width); sim_thr: read_type.sim_thr().
    Covered: the head tip with both keys (the second one, which the reference marks "Here is a bug", as it stands), every
    windows(2) gap with MARGIN = 25, the forward key before the reverse key, and the `end <= start` skip, the tail tip with both
    keys.  -> list of dict(insert_at, start, end, is_forward, chunks, radius, sim_thr) in the reference's order (pack_edge_trials
    takes them once `read` is added); insert_at is the index the trial's nodes get in `inserts`: 0, idx + 1, len + 1."""
    out = []

    def trial(insert_at, start, end, direction, chunks):
        contig_len = sum(len(c) for c in chunks)
        out.append(dict(insert_at=insert_at, start=start, end=end, is_forward=direction, chunks=chunks, radius=int(band_width_of(contig_len)),
                        sim_thr=sim_thr))

    if len(nodes):
        chunk, cluster, forward, position, _ = nodes[0]
        start, end = 0, min(position + EDGE_MARGIN, seq_len)
        for chunks in tips.get((chunk, cluster, bool(forward), False), ()):
            trial(0, start, end, True, chunks)
        for chunks in tips.get((chunk, cluster, not forward, True), ()):
            trial(0, start, end, False, chunks)
    for idx in range(len(nodes) - 1):
        a, b = nodes[idx], nodes[idx + 1]
        start = min(max(a[3] + a[4], EDGE_MARGIN) - EDGE_MARGIN, seq_len)
        end = min(b[3] + EDGE_MARGIN, seq_len)
        forward_key = ((a[0], a[1], bool(a[2])), (b[0], b[1], bool(b[2])))
        reverse_key = ((b[0], b[1], not b[2]), (a[0], a[1], not a[2]))
        if forward_key in edges:
            chunks, direction = edges[forward_key], True
        elif reverse_key in edges:
            chunks, direction = edges[reverse_key], False
        else:
            continue
        if end <= start:     # "TooNear"
            continue
        trial(idx + 1, start, end, direction, chunks)
    if len(nodes):
        chunk, cluster, forward, position, length = nodes[-1]
        start = max(min(position + length, seq_len) - EDGE_MARGIN, 0)
        end = min(seq_len + EDGE_MARGIN, seq_len)
        for chunks in tips.get((chunk, cluster, bool(forward), True), ()):
            trial(len(nodes) + 1, start, end, True, chunks)
        for chunks in tips.get((chunk, cluster, not forward, False), ()):
            trial(len(nodes) + 1, start, end, False, chunks)
    return out


CONS_MIN_LENGTH, CONS_MAX_LENGTH = 400, 10_000     # dense_encoding.rs:7-8


def edge_consensus_plan(seqs, cov_thr):
    """the host part of `consensus` (dense_encoding.rs:548-561, :572-573) -> None or (the kept sequences, the draft first, and the
    band).  Own decision where select_nth_unstable leaves the order open: the sequences keep their input order, the median is the
    element at index len / 2 of the ascending lengths, and the draft is the first sequence in input order of that length."""
    seqs = [_as_bytes(s) for s in seqs]
    median = sorted(len(s) for s in seqs)[len(seqs) // 2]
    upper, lower = 2 * median, max(median, CONS_MIN_LENGTH) // 2
    if upper <= lower or CONS_MAX_LENGTH < median:
        return None
    idx = next(k for k, s in enumerate(seqs) if len(s) == median)
    seqs[0], seqs[idx] = seqs[idx], seqs[0]
    seqs = [s for s in seqs if lower <= len(s) < upper]
    if len(seqs) <= cov_thr:
        return None
    mean_len = sum(len(s) for s in seqs) // len(seqs)
    return seqs, min(max(mean_len // 20, 10), 50)


def edge_consensus(seqs, cov_thr, device=0):
    """`consensus` (dense_encoding.rs:548-579): the edge's sequences of median-like length, aligned to the draft with align_reads
    (global), then two polish_guided calls that share the ops.  -> the consensus (uint8 array), or None where the reference
    returns None: 2 median <= max(median, 400) / 2, a median above 10,000, at most cov_thr sequences inside the length window
    [max(median, 400) / 2, 2 median), a result that is not longer than 400.  The polish is this build's own specification."""
    from .batch import pack
    plan = edge_consensus_plan(seqs, cov_thr)
    if plan is None:
        return None
    seqs, band = plan
    reads = [np.frombuffer(s, dtype=np.uint8) for s in seqs]
    none = np.zeros(0, dtype=np.uint8)
    batch = pack([(0, 1, reads[0], reads, [none] * len(reads), [1] * len(reads), None)])
    aligned = align_reads(batch, device=device)
    ops, ops_off = aligned["ops"], aligned["ops_off"]
    cons = reads[0]
    for _ in range(2):      # :574-577
        batch = pack([(0, 1, cons, reads, [ops[int(ops_off[r]):int(ops_off[r + 1])] for r in range(len(reads))], [1] * len(reads), None)])
        out = polish_guided(batch, band, device=device)
        cons = out["cons"][int(out["cons_off"][0]):int(out["cons_off"][1])].copy()
        ops, ops_off = out["ops_out"], out["ops_out_off"]
    return cons if CONS_MIN_LENGTH < len(cons) else None


def correct_clustering_with_sims(*args, **kw):
    """correct_clustering with the diagnostic switch of include/jtk_lc_debug.h on: returns (cluster, touched, sims), sims = the
    raw similarity matrix (before filter_similarity) of every corrected chunk, in selected_chunks order.  A test hook: the
    matrices are kept on the calling thread only while the switch is on, and it is off again when this returns."""
    L = ffi.lib()
    L.jtk_lc_debug_cc_keep_sims.argtypes = [C.c_int]
    L.jtk_lc_debug_cc_keep_sims.restype = None
    L.jtk_lc_debug_cc_sims_count.argtypes = []
    L.jtk_lc_debug_cc_sims_count.restype = C.c_size_t
    L.jtk_lc_debug_cc_sims.argtypes = [C.c_size_t, C.POINTER(C.c_double), C.c_size_t]
    L.jtk_lc_debug_cc_sims.restype = C.c_size_t
    L.jtk_lc_debug_cc_keep_sims(1)
    try:
        cluster, touched = correct_clustering(*args, **kw)
        sims = []
        for job in range(L.jtk_lc_debug_cc_sims_count()):
            size = L.jtk_lc_debug_cc_sims(job, None, 0)
            n = int(round(size ** 0.5))
            m = np.zeros((n, n))
            assert n * n == size and L.jtk_lc_debug_cc_sims(job, f64p(m), m.size) == size
            sims.append(m)
    finally:
        L.jtk_lc_debug_cc_keep_sims(0)
    return cluster, touched, sims


def cluster_features(params, feature_chunks, variants, variant_type, post_stride, device=0,
                     raise_on_chunk_failure=True):
    """jtk_lc_cluster_features: cluster_filtered_variants + posterior on caller-supplied feature matrices."""
    L = ffi.lib()
    n_reads = int(feature_chunks["n_reads"].sum())
    label = np.zeros(n_reads, dtype=np.uint32)
    post = np.zeros((n_reads, post_stride), dtype=np.float64)
    result = np.zeros(len(feature_chunks), dtype=ffi.RESULT_DT)
    variants = np.ascontiguousarray(variants, dtype=np.float64)
    variant_type = np.ascontiguousarray(variant_type, dtype=np.uint32)
    rc = L.jtk_lc_cluster_features(C.byref(params), len(feature_chunks), feature_chunks.ctypes.data, f64p(variants),
                                   u32p(variant_type), u32p(label), f64p(post), post_stride, result.ctypes.data, device)
    if rc != 0 and (raise_on_chunk_failure or rc != -6):
        check(rc)
    return dict(rc=rc, label=label, log_post=post, result=result)


def trim_cache(device=0):
    """jtk_lc_trim_cache: hand the pooled device blocks of finished calls back to the driver."""
    check(ffi.lib().jtk_lc_trim_cache(device))


def last_timing():
    t = ffi.Timing()
    check(ffi.lib().jtk_lc_last_timing(C.byref(t)))
    return dict(total_ms=t.total_ms, h2d_ms=t.h2d_ms, d2h_ms=t.d2h_ms,
                kernel_ms={n: t.kernel_ms[i] for i, n in enumerate(ffi.KERNEL_NAMES)},
                kernel_launches={n: int(t.kernel_launches[i]) for i, n in enumerate(ffi.KERNEL_NAMES)},
                chain_lds_bytes=[int(t.chain_lds_bytes[0]), int(t.chain_lds_bytes[1])])


class Session:
    """Resident-batch session: inputs uploaded once, `run()` = one pass of the hot path on the device."""

    def __init__(self, params, batch, device=0):
        self._lib = ffi.lib()
        self._h = C.c_void_p()
        self.batch = batch
        self.params = params
        check(self._lib.jtk_lc_session_create(C.byref(params), batch.n_chunks, batch.chunks.ctypes.data,
                                              u8p(batch.tmpl_bases), u8p(batch.read_bases), u64p(batch.read_off),
                                              u8p(batch.ops), u64p(batch.ops_off), u8p(batch.strand),
                                              batch.post_stride, device, C.byref(self._h)))

    def run(self, skip_polish=False):
        check(self._lib.jtk_lc_session_run(self._h, int(skip_polish)))

    def fetch(self, raise_on_chunk_failure=True, out=None):
        """every output of the stage call: labels, log-posteriors, per-chunk records, consensus and re-threaded ops (out = the
        arrays of an earlier fetch, overwritten)"""
        o = out if out is not None else _outputs(self.batch)
        rc = self._lib.jtk_lc_session_fetch(self._h, u32p(o["label"]), f64p(o["log_post"]), o["result"].ctypes.data,
                                            u8p(o["cons"]), u64p(o["cons_off"]), len(o["cons"]), u8p(o["ops_out"]),
                                            u64p(o["ops_out_off"]), len(o["ops_out"]))
        if rc != 0 and (raise_on_chunk_failure or rc != -6):
            check(rc)
        o["rc"] = rc
        return o

    def fetch_results(self, raise_on_chunk_failure=True):
        """labels, log-posteriors and the per-chunk records only (no consensus / ops): the payload of the label gather"""
        b = self.batch
        label = np.zeros(b.n_reads, dtype=np.uint32)
        post = np.zeros((b.n_reads, b.post_stride), dtype=np.float64)
        result = np.zeros(b.n_chunks, dtype=ffi.RESULT_DT)
        rc = self._lib.jtk_lc_session_fetch(self._h, u32p(label), f64p(post), result.ctypes.data, None, None, 0, None,
                                            None, 0)
        if rc != 0 and (raise_on_chunk_failure or rc != -6):
            check(rc)
        return dict(rc=rc, label=label, log_post=post, result=result)

    def trace(self, chunk):
        """the reference's trace! rows of one chunk's clustering (TOTAL / CAND / PICK / DUMP / RANGE / LK / COUNTS;
        pseudo_mcmc.rs:122-127,236,250-262,467-472,539) after run(): a list of rows"""
        need = C.c_size_t(0)
        buf = C.create_string_buffer(1 << 16)
        rc = self._lib.jtk_lc_session_trace(self._h, int(chunk), buf, len(buf), C.byref(need))
        if rc != 0 and need.value > len(buf):
            buf = C.create_string_buffer(need.value)
            rc = self._lib.jtk_lc_session_trace(self._h, int(chunk), buf, len(buf), C.byref(need))
        check(rc)
        return buf.raw[:need.value].decode().splitlines()

    def chain_profile(self):
        """jtk_lc_debug_chain_profile (include/jtk_lc_debug.h): per chunk, the cycles of its chain and its events"""
        cyc = np.zeros(self.batch.n_chunks, dtype=np.uint64)
        ev = np.zeros(self.batch.n_chunks, dtype=np.uint32)
        f = self._lib.jtk_lc_debug_chain_profile
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
        check(f(self._h, u64p(cyc), u32p(ev)))
        return cyc, ev

    def lane(self):
        """jtk_lc_debug_session_lane (include/jtk_lc_debug.h): the index of the session's lane on its device"""
        lane = self._lib.jtk_lc_debug_session_lane(self._h)
        if lane < 0:
            check(lane)
        return lane

    def passes(self):
        """jtk_lc_debug_session_passes (include/jtk_lc_debug.h): how the session's last passes ended, oldest first, each
        dict(pass_, how ("word" / "event" / None), event_pending, members, still_waiting, round_stream, next_round_stream,
        stamp_left, stamp_returned, stamp_fetched, stamp_round0)"""
        rec = (ffi.PassRecord * ffi.DEBUG_PASS_RECORDS)()
        n = self._lib.jtk_lc_debug_session_passes(self._h, rec, ffi.DEBUG_PASS_RECORDS)
        if n < 0:
            check(n)
        how = {ffi.LEFT_BY_WORD: "word", ffi.LEFT_BY_EVENT: "event"}
        return [dict(pass_=int(r.pass_), how=how.get(int(r.how)), event_pending=bool(r.event_pending), members=int(r.members),
                     still_waiting=int(r.still_waiting), round_stream=int(r.round_stream),
                     next_round_stream=int(r.next_round_stream), stamp_left=int(r.stamp_left),
                     stamp_returned=int(r.stamp_returned), stamp_fetched=int(r.stamp_fetched), stamp_round0=int(r.stamp_round0))
                for r in rec[:n]]

    def close(self):
        if self._h:
            self._lib.jtk_lc_session_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def lane_hold(lane, hold, device=0):
    """jtk_lc_debug_lane_hold (include/jtk_lc_debug.h): hold (True) or release (False) the chain launches of a lane; a lane
    that does not exist and a release without a hold raise JtkError"""
    check(ffi.lib().jtk_lc_debug_lane_hold(int(device), int(lane), int(bool(hold))))


def lane_state(lane, device=0):
    """jtk_lc_debug_lane_state: dict(in_pass, holds, pending, launch_calls, records); records = the most recent launch calls,
    oldest first, each dict(members, segments=[class 0, class 1], chunks=[...], seg_chunks=[[per segment], [...]])"""
    st = ffi.LaneState()
    check(ffi.lib().jtk_lc_debug_lane_state(int(device), int(lane), C.byref(st)))
    records = []
    for r in st.records[:st.n_records]:
        seg = [int(r.segments[0]), int(r.segments[1])]
        records.append(dict(members=int(r.members), segments=seg, chunks=[int(r.chunks[0]), int(r.chunks[1])],
                            seg_chunks=[[int(r.seg_chunks[j][i]) for i in range(seg[j])] for j in range(2)]))
    return dict(in_pass=int(st.in_pass), holds=int(st.holds), pending=int(st.pending), launch_calls=int(st.launch_calls),
                records=records)


def round_hold(lane, hold, device=0):
    """jtk_lc_debug_round_hold (include/jtk_lc_debug.h): hold (True / 1) or release (False / 0) the round launches of a lane, or
    let the sessions parked now launch once under the hold ("step" / 2)"""
    code = 2 if hold == "step" else int(hold)
    check(ffi.lib().jtk_lc_debug_round_hold(int(device), int(lane), code))


def round_state(lane, device=0):
    """jtk_lc_debug_round_state: dict(in_rounds, holds, parked, launch_calls, records); records = the most recent round launches,
    oldest first, each dict(members, merged, round=[per member; None = the opening of a pass], chunks=[...], phmm_items=[...])"""
    st = ffi.RoundState()
    check(ffi.lib().jtk_lc_debug_round_state(int(device), int(lane), C.byref(st)))
    records = []
    for r in st.records[:st.n_records]:
        n = int(r.members)
        records.append(dict(members=n, merged=bool(r.merged),
                            round=[None if r.round[i] == ffi.DEBUG_ROUND_OPEN else int(r.round[i]) for i in range(n)],
                            chunks=[int(r.chunks[i]) for i in range(n)], phmm_items=[int(r.phmm_items[i]) for i in range(n)]))
    return dict(in_rounds=int(st.in_rounds), holds=int(st.holds), parked=int(st.parked), launch_calls=int(st.launch_calls),
                records=records)


def normalize_pileup(label, log_post, cluster_num):
    """normalize_local_clustering for one pile-up (normalize.rs:21-50), in place."""
    label = np.ascontiguousarray(label, dtype=np.uint32)
    log_post = np.ascontiguousarray(log_post, dtype=np.float64)
    check(ffi.lib().jtk_lc_normalize_pileup(len(label), int(cluster_num), u32p(label), f64p(log_post),
                                            log_post.shape[1]))
    return label, log_post


def record_rows(chunk_ids, n_reads, tmpl_len, read_bases_per_chunk, copy_num, result, cons_len, timing):
    """The reference's per-chunk `RECORD` lines (local_clustering/mod.rs:121: chunk id, elapsed ms, polish ms, consensus
    length, score, coverage).  The device runs the chunks of a call together, so a chunk's time is its SHARE of the call's
    kernel time per family: pair-HMM and polishing by band cells x passes, the chain by proposals x candidate k."""
    n = np.asarray(n_reads, dtype=np.float64)
    passes = np.minimum(result["polish_rounds"].astype(np.float64) + 1.0, 21.0)
    w_dp = passes * (n * np.asarray(tmpl_len, dtype=np.float64) + np.asarray(read_bases_per_chunk, dtype=np.float64))
    k_tried = np.maximum(1, np.minimum(np.asarray(copy_num, dtype=np.int64), 1 + 2 * result["n_variants"].astype(np.int64)) - 1)
    w_mc = n * k_tried * (result["n_variants"] > 0)
    km = timing["kernel_ms"]
    polish_ms = (km["phmm"] + km["polish"]) * w_dp / max(float(w_dp.sum()), 1.0)
    elapsed = polish_ms + km["filter"] / max(1, len(n)) + km["mcmc"] * w_mc / max(float(w_mc.sum()), 1.0)
    return ["RECORD\t%d\t%.3f\t%.3f\t%d\t%.3f\t%d" % (int(chunk_ids[c]), elapsed[c], polish_ms[c], int(cons_len[c]),
                                                      float(result["score"][c]), int(n[c])) for c in range(len(n))]
