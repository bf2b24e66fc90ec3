"""Small named problems for the purge entry points (tests/purge_reference.py; jtk_lc_node_errors, jtk_lc_error_quantile,
jtk_lc_estimate_error_rate, jtk_lc_purge_diverged): one for each place the code can go wrong.  CASES[name] = dict(ds=, and where
a case was built for it: node_status= {node index: status}, fit_status=, n_iter= (lo, hi), purge_status=, flags= {chunk id:
[flag per cluster]}, fallback= the fit's first read rate when the case fixes one).  QUANTILE[name] = (err_num, err_len).

A data set is laid out like a real one: every read has a raw sequence, its nodes sit in it at `position_from_start` (a negative
gap makes two nodes overlap), a reverse node holds the reverse complement of its stretch, so that the reads can be rebuilt and
recovered after a purge."""
import random

import purge_reference as R

COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}
M, X, I, D = 0, 1, 2, 3
WAVES_PER_PASS = 2048 * 4        # the column walk's grid: 2,048 workgroups of four waves, one node per wave and pass


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def revcomp(s):
    return "".join(COMPLEMENT[b] for b in reversed(s.upper()))


def other(rng, b):
    return rng.choice([x for x in "ACGT" if x != b.upper()])


def read_for(tmpl, ops, rng):
    """a node sequence on which `ops` show what they say: 0 copies the template base, 1 changes it, 2 inserts, 3 skips"""
    out, r = [], 0
    for op in ops:
        if op == M:
            out.append(tmpl[r])
        elif op == X:
            out.append(other(rng, tmpl[r]))
        elif op == I:
            out.append(rng.choice("ACGT"))
        if op != I:
            r += 1
    return "".join(out)


def cigar_of(ops):
    out = []
    for op in ops:
        k = "MMID"[op]
        if out and out[-1][0] == k:
            out[-1][1] += 1
        else:
            out.append([k, 1])
    return "".join("%d%s" % (n, k) for k, n in out)


def hard(k, c):
    p = [-10000.0] * k
    if k:
        p[c % k] = 0.0
    return p


def node(chunk, cluster, seq, ops, k=1, forward=True, post=None, raw_ops=False):
    n = dict(chunk=chunk, cluster=cluster, is_forward=forward, posterior=hard(k, cluster) if post is None else list(post), seq=seq)
    if raw_ops:
        n["ops"] = list(ops)
    else:
        n["cigar"] = cigar_of(ops)
    return n


def lay_out(rid, items, rng, lead=3, trail=2):
    """items = [(node, gap)]: the read's raw sequence around its nodes; gap < 0 lets a node start inside the one before it (its
    first bases then ARE that node's last bases, whatever the node was given)"""
    raw, nodes = rand_seq(rng, lead), []
    for n, gap in items:
        orig = n["seq"] if n["is_forward"] else revcomp(n["seq"])
        if nodes and gap < 0:
            pos = len(raw) + gap
            orig = raw[pos:] + orig[-gap:]
        else:
            raw += rand_seq(rng, max(gap, 0))
            pos = len(raw)
        raw = raw[:pos] + orig
        nodes.append(dict(n, seq=orig if n["is_forward"] else revcomp(orig), position_from_start=pos))
    return dict(id=rid, nodes=nodes, seq=raw + rand_seq(rng, trail))


def make(reads, chunks, rng, gaps=None):
    """reads = [[node, ...]], chunks = [(id, cluster_num, copy_num, seq)]; gaps = {(read, node index): gap}, default 2"""
    gaps = gaps or {}
    return dict(reads=[lay_out(10 + 3 * r, [(n, gaps.get((r, i), 2)) for i, n in enumerate(ns)], rng) for r, ns in enumerate(reads)],
                chunks=[dict(id=i, cluster_num=k, copy_num=cp, score=1.0, seq=s) for i, k, cp, s in chunks], coverage=10.0)


CASES = {}


# ---- the column walk: 64 ops per step

def _mixed_ops(rng, n):
    return [rng.choice((M, M, M, M, M, M, X, I, D)) for _ in range(n)]


def _columns():
    rng = random.Random(1)
    lists = [_mixed_ops(rng, n) for n in (1, 63, 64, 65, 127, 128, 129, 301)]
    lists.append([M] * 60 + [I] * 10 + [M] * 30)                 # an insertion run over a step's edge
    lists.append([M] * 60 + [D] * 10 + [M] * 30)                 # a deletion run over it
    lists.append([X if i in (0, 63, 64, 127) else M for i in range(200)])   # a mismatch in the first and the last lane
    lists.append([I] * 64 + [D] * 64 + [M])                      # a step that moves one position only
    chunks, nodes = [], []
    for i, ops in enumerate(lists):
        tmpl = rand_seq(rng, len([o for o in ops if o != I]) + 4)
        chunks.append((100 + i, 1, 1, tmpl))
        nodes.append(node(100 + i, 0, read_for(tmpl, ops, rng), ops))
    n_mixed = len(nodes)
    # lower case on either side; the op code does not decide between '|' and 'X', the bases do
    tmpl = rand_seq(rng, 90)
    ops = _mixed_ops(rng, 80)
    chunks.append((200, 1, 1, tmpl.lower()))
    nodes.append(node(200, 0, read_for(tmpl, ops, rng), ops))
    chunks.append((201, 1, 1, tmpl))
    nodes.append(node(201, 0, read_for(tmpl, ops, rng).lower(), ops))
    seq = read_for(tmpl, [M] * 70, rng)
    chunks.append((202, 1, 1, tmpl))
    nodes.append(node(202, 0, seq, [X] * 35 + [M] * 35, raw_ops=True))                  # says Mismatch, shows '|'
    nodes.append(node(202, 0, read_for(tmpl, [X] * 70, rng), [M] * 70, raw_ops=True))   # says Match, shows 'X'
    # a node that consumes less than its sequence, and less than the template
    nodes.append(node(202, 0, seq + "ACGTA", [M] * 64, raw_ops=True))
    return make([nodes[:5], nodes[5:n_mixed], nodes[n_mixed:]], chunks, rng)


CASES["columns"] = dict(ds=_columns(), fit_status=0)


def _columns_bad():
    rng = random.Random(2)
    tmpl = rand_seq(rng, 64)
    seq64 = tmpl                                                  # 64 bases, 64 template bases
    good = node(300, 0, seq64, [M] * 64, raw_ops=True)
    bad = [
        node(300, 0, seq64, [M] * 64 + [I], raw_ops=True),       # the read ends with the step: op 64 is one too many
        node(300, 0, seq64[:63], [M] * 64, raw_ops=True),        # ... and in the step's last lane
        node(300, 0, seq64, [M] * 64 + [D], raw_ops=True),       # the same for the template
        node(300, 0, seq64 + "A", [M] * 63 + [I, D, D], raw_ops=True),
        node(300, 0, seq64, [M] * 30 + [4] + [M] * 10, raw_ops=True),                     # no such op
        node(300, 0, seq64[:20], [M] * 10 + [4] + [M] * 30, raw_ops=True),                # no such op, in front of an overrun
        node(300, 0, seq64[:20], [M] * 25 + [7] + [M] * 10, raw_ops=True),                # an overrun in front of no such op
        node(300, 0, seq64, [], raw_ops=True),                    # no columns
        node(301, 0, seq64, [M] * 64, raw_ops=True),              # a chunk nobody knows
        node(300, 0, "", [D] * 64, raw_ops=True),                 # an empty sequence is fine while nothing reads it
    ]
    reads = [[good] + bad[:4], bad[4:7] + [good], bad[7:] + [good]]
    ds = make(reads, [(300, 1, 1, tmpl)], rng)
    status = {1: -5, 2: -5, 3: -5, 4: -5, 5: -1, 6: -1, 7: -5, 9: -6, 10: -6}
    return dict(ds=ds, node_status=status, fit_status=-1, purge_status=-6)


CASES["columns_bad"] = _columns_bad()


def _beyond_one_pass():
    """more nodes than the column walk has waves: 8,300 nodes of 3 to 9 columns in reads of five"""
    rng = random.Random(3)
    tmpls = {i: rand_seq(rng, 12) for i in range(400, 407)}
    nodes = []
    for i in range(WAVES_PER_PASS + 108):
        cid = 400 + i % 7
        ops = _mixed_ops(rng, 3 + i % 7)
        nodes.append(node(cid, 0, read_for(tmpls[cid], ops, rng), ops))
    return make([nodes[i:i + 5] for i in range(0, len(nodes), 5)], [(i, 1, 1, t) for i, t in tmpls.items()], rng)


CASES["beyond_one_pass"] = dict(ds=_beyond_one_pass(), fit_status=0)


# ---- the fit: nodes of L columns with k mismatches, rate k / L

def rated(chunk, cluster, tmpl, length, k, rng, n_clusters=2, forward=True, post=None):
    where = set((2 * j + 1) * length // (2 * k) for j in range(k)) if k else set()
    ops = [X if i in where else M for i in range(length)]
    seq = read_for(tmpl, ops, rng)
    return node(chunk, cluster, seq, [M] * length, k=n_clusters, forward=forward, post=post)


def fit_case(seed, spec, clusters, gaps=None, posts=None):
    """spec = [[(chunk, cluster, columns, mismatches[, is_forward]), ...] per read]; clusters = {chunk id: cluster_num} in chunks[] order"""
    rng = random.Random(seed)
    tmpls = {cid: rand_seq(rng, 320) for cid in clusters}
    posts = posts or {}
    reads = [[rated(c, cl, tmpls[c], n, k, rng, n_clusters=clusters[c], forward=not fwd or fwd[0], post=posts.get((r, i)))
              for i, (c, cl, n, k, *fwd) in enumerate(row)] for r, row in enumerate(spec)]
    return make(reads, [(cid, k, max(k, 1), tmpls[cid]) for cid, k in clusters.items()], rng, gaps=gaps)


# every rate equal: the first pass already meets the test
CASES["fit_one_pass"] = dict(ds=fit_case(4, [[(1, 0, 100, 5), (2, 1, 200, 10)], [(2, 0, 100, 5), (1, 1, 60, 3)]], {1: 2, 2: 2}),
                             fit_status=0, n_iter=(1, 1), flags={1: [0, 0], 2: [0, 0]})


def _diverged_cluster(n_reads=40):
    """chunk 2's cluster 1 is far off on every other read, every read has its own rate: the fit needs a good many passes"""
    spec = []
    for r in range(n_reads):
        base = 2 + r % 25
        spec.append([(1, r % 2, 200, base), (2, 1 if r % 2 == 0 else 0, 200, base + (40 if r % 2 == 0 else 0)), (3, 0, 200, base + r % 2)])
    return spec


CASES["fit_many_passes"] = dict(ds=fit_case(5, _diverged_cluster(), {1: 2, 2: 2, 3: 1}), fit_status=0, n_iter=(10, 200),
                                flags={1: [0, 0], 2: [0, 1], 3: [0]})

# a slot whose sum goes negative: chunk 5's nodes are clean, in reads whose other nodes are not (fallback 0.2): max(., 0) acts
CASES["fit_negative_slot"] = dict(ds=fit_case(6, [[(5, 0, 100, 0), (6, 0, 100, 20), (7, 0, 100, 20)] for _ in range(6)], {5: 1, 6: 1, 7: 1}),
                                  fit_status=0, negative_slot=5)

# a chunk with no cluster at all, a chunk and a cluster no node touches (divisor 0.1), a read without nodes; chunks[] not in id order
CASES["fit_empty_corners"] = dict(
    ds=fit_case(7, [[(12, 0, 100, 4), (9, 0, 150, 9)], [], [(9, 0, 120, 30), (12, 2, 90, 2)], []], {12: 3, 8: 0, 9: 1, 10: 2}),
    fit_status=0)

# a cluster index equal to cluster_num: the reference indexes past its table
CASES["fit_cluster_out_of_range"] = dict(ds=fit_case(8, [[(1, 0, 100, 5), (2, 2, 100, 5)]], {1: 2, 2: 2}), fit_status=-6, purge_status=-6)
CASES["no_nodes"] = dict(ds=fit_case(9, [[], []], {1: 2}), fit_status=-1, purge_status=-1)


def _real_valued():
    """about 40 reads over 6 chunks, lengths and counts that give rates with full mantissas"""
    rng = random.Random(10)
    spec = []
    for r in range(41):
        path = sorted(rng.sample(range(20, 26), 2 + r % 4))
        spec.append([(c, rng.randrange(2), rng.randrange(151, 300), rng.randrange(0, 40) + (45 if c == 22 and r % 4 == 0 else 0)) for c in path])
    for row in spec:            # the far-off nodes of chunk 22 are its cluster 1
        for i, (c, cl, n, k) in enumerate(row):
            if c == 22:
                row[i] = (c, 1 if k >= 45 else 0, n, k)
    return fit_case(10, spec, {c: 2 for c in (23, 20, 25, 21, 22, 24)})


CASES["fit_real_valued"] = dict(ds=_real_valued(), fit_status=0)


def order_shows(ds):
    """the fit with every slot's and every residual's terms added in reverse differs in at least one output bit"""
    num, length, _ = R.node_errors(ds)
    fallback = R.error_quantile(num, length, 0.5)
    a, b = R.estimate_error_rate(ds, num, length, fallback), R.estimate_error_rate(ds, num, length, fallback, reverse=True)
    return a["read_err"] != b["read_err"] or a["chunk_err"] != b["chunk_err"] or a["n_iter"] != b["n_iter"]


assert order_shows(CASES["fit_real_valued"]["ds"]), "fit_real_valued must tell summation orders apart"


# ---- the purge

CLEAN, FAR = 4, 64       # mismatches in 200 columns


def _purge_spec(n_reads, far_cluster, chunk=31, k=3):
    """reads over chunks 30, 31, 32; chunk 31 has k clusters, the nodes of `far_cluster` are far off"""
    spec = []
    for r in range(n_reads):
        cl = r % k
        spec.append([(30, r % 2, 200, CLEAN + r % 3), (chunk, cl, 200, FAR if cl in far_cluster else CLEAN), (32, 0, 200, CLEAN)])
    return spec


CASES["purge_no_flag"] = dict(ds=fit_case(11, _purge_spec(12, ()), {30: 2, 31: 3, 32: 1}), purge_status=0,
                              flags={30: [0, 0], 31: [0, 0, 0], 32: [0]})
# the middle cluster of three goes: cluster 2 becomes 1, the posteriors lose their middle entry
CASES["purge_middle_of_three"] = dict(ds=fit_case(12, _purge_spec(12, (1,)), {30: 2, 31: 3, 32: 1}), purge_status=0,
                                      flags={30: [0, 0], 31: [0, 1, 0], 32: [0]})
# every cluster of a chunk far off: "the fault of the consensus", nothing is flagged
CASES["purge_all_flagged"] = dict(ds=fit_case(13, _purge_spec(12, (0, 1, 2)), {30: 2, 31: 3, 32: 1}), purge_status=0, all_diverged=31,
                                  flags={30: [0, 0], 31: [0, 0, 0], 32: [0]})


def _loses_nodes():
    """read 0 is nothing but far-off nodes (it vanishes); read 1 loses its first, a middle and its last node; the lost middle one
    starts 30 bases inside the node before it and the node after it 10 bases inside that one too (an edge offset of -10 after the
    rebuild); chunk 33 is visited in reverse"""
    spec = _purge_spec(12, (1,))
    spec[0] = [(31, 1, 200, FAR), (31, 1, 180, FAR - 6)]
    spec[1] = [(31, 1, 200, FAR), (30, 0, 200, CLEAN), (33, 0, 150, CLEAN, False), (31, 1, 60, 20), (32, 0, 200, CLEAN), (30, 1, 200, CLEAN), (31, 1, 200, FAR)]
    gaps = {(1, 2): -7, (1, 3): -30, (1, 4): -40, (1, 5): 20, (1, 6): 0}
    return fit_case(14, spec, {30: 2, 31: 3, 32: 1, 33: 1}, gaps=gaps)


CASES["purge_loses_first_middle_last"] = dict(ds=_loses_nodes(), purge_status=0, flags={30: [0, 0], 31: [0, 1, 0], 32: [0], 33: [0]})
# a kept node of the flagged chunk with four posterior entries for three clusters: the reference indexes past cluster_info
CASES["purge_posterior_too_long"] = dict(ds=fit_case(15, _purge_spec(12, (1,)), {30: 2, 31: 3, 32: 1}, posts={(0, 1): [0.0, -1.0, -2.0, -3.0]}),
                                         purge_status=-6, fit_status=0)
# ... two entries are fine, and so are four on a node that goes, or on a chunk that loses nothing
CASES["purge_posterior_short"] = dict(
    ds=fit_case(16, _purge_spec(12, (1,)), {30: 2, 31: 3, 32: 1}, posts={(0, 1): [0.0, -1.0], (1, 1): [0.0, -1.0, -2.0, -3.0], (2, 0): [0.0] * 5}),
    purge_status=0, flags={30: [0, 0], 31: [0, 1, 0], 32: [0]})

NAMES = sorted(CASES)

QUANTILE = {
    "one_node": ([3], [7]),
    "odd": ([1, 9, 4, 0, 7], [10, 11, 13, 9, 300]),
    "even": ([5, 1, 9, 4, 0, 7], [17, 10, 11, 13, 9, 300]),
    "ties": ([2, 1, 4, 3, 1, 2, 0], [20, 10, 40, 30, 7, 14, 5]),
    "more_than_a_block": ([(i * 7919) % 251 for i in range(3000)], [251 + (i * 31) % 97 for i in range(3000)]),
}
