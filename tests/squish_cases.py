"""Small named problems for squish_erroneous_clusters (tests/squish_reference.py, jtk_lc_squish_clusters): one for each place
the code can go wrong.  CASES[name] = dict(ds=, cfg= overrides of the default configuration, status= expected status, and,
where a case was built for it, classes= {chunk id: expected class} / pairs= the expected surviving pairs / n_obs= {pair: count}).

Posteriors: `hard(k, c)` is -10000 everywhere but 0 at c (biased for every k), `flat(k)` is ln(1/k) everywhere (never biased
for k >= 2).  A chunk is (id, cluster_num, copy_num)."""
import math
import random

STIFF, ISOLATED, SUSPICIOUS = 0, 1, 2


def hard(k, c):
    p = [-10000.0] * k
    p[c % k] = 0.0
    return p


def flat(k):
    return [math.log(1.0 / k)] * k


def node(chunk, cluster, post=None, k=2):
    return dict(chunk=chunk, cluster=cluster, is_forward=True, posterior=hard(k, cluster) if post is None else list(post))


def make(reads, chunks):
    return dict(reads=[dict(id=i, nodes=list(nodes)) for i, nodes in enumerate(reads)],
                chunks=[dict(id=i, cluster_num=k, copy_num=cp, score=1.0) for i, k, cp in chunks], coverage=10.0)


def pair_reads(u, v, labels):
    """one read per (cu, cv) of `labels`, with one node of chunk u and one of chunk v"""
    return [[node(u, a), node(v, b)] for a, b in labels]


MATCH = [(i % 2, i % 2) for i in range(12)]                       # perfectly matching labels, 12 reads
ANTI = [(0, 0), (0, 1), (1, 0), (1, 1)] * 3                       # independent labels: ARI -0.1
CASES = {}

# ---- the strict count threshold: 10 shared reads die, 11 survive
CASES["count_threshold"] = dict(
    ds=make(pair_reads(1, 2, MATCH[:10]) + pair_reads(3, 4, MATCH[:11]), [(1, 2, 2), (2, 2, 2), (3, 2, 2), (4, 2, 2)]),
    pairs=[(3, 4)], n_obs={(3, 4): 11})

# ---- a chunk twice in a read: (5, 6) counts 2 per read, (5, 5) counts 1 per read; the minimum of the two nodes' clusters is the
# read's label (the first node says the opposite); four reads with a single node of 5 are observations of (5, 5) only
_twice = [[node(5, 1), node(6, i % 2), node(5, i % 2)] for i in range(11)] + [[node(5, i % 2)] for i in range(4)]
CASES["chunk_twice_in_read"] = dict(ds=make(_twice, [(5, 2, 2), (6, 2, 2)]), pairs=[(5, 5), (5, 6)], n_obs={(5, 5): 15, (5, 6): 11})

# ---- is_biased at its edges: k = 2 puts the threshold at 0.7; post_len 0 and 1 are biased
_above, _below = [math.log(0.7) + 1e-9, math.log(0.3)], [math.log(0.7) - 1e-9, math.log(0.3)]
_edges = pair_reads(7, 8, MATCH[:9])
_edges += [[node(7, 0, _above), node(8, 0)], [node(7, 1), node(8, 1, [])], [node(7, 0, [-5.0]), node(8, 0)]]
_edges += [[node(7, 1, _below), node(8, 0)], [node(7, 0), node(8, 1, _below)]]      # must not count: 12 observations, not 14
CASES["bias_threshold_edges"] = dict(ds=make(_edges, [(7, 2, 2), (8, 2, 2)]), pairs=[(7, 8)], n_obs={(7, 8): 12})

# ---- unbiased nodes vanish from the counts: 8 biased + 5 unbiased shared reads stay below the threshold
_unb = pair_reads(9, 10, MATCH[:8]) + [[node(9, i % 2, flat(2)), node(10, i % 2)] for i in range(5)]
CASES["unbiased_nodes_vanish"] = dict(ds=make(_unb, [(9, 2, 2), (10, 2, 2)]), pairs=[])

# ---- ... and from the tables: 11 biased reads match perfectly, 4 unbiased ones would spoil it
_unb2 = pair_reads(9, 10, MATCH[:11]) + [[node(9, 0, flat(2)), node(10, 1)] for _ in range(4)]
CASES["unbiased_nodes_not_in_table"] = dict(ds=make(_unb2, [(9, 2, 2), (10, 2, 2)]), pairs=[(9, 10)], n_obs={(9, 10): 11})

# ---- a chunk with one cluster drops out however many reads it shares
CASES["single_cluster_chunk"] = dict(ds=make(pair_reads(11, 12, [(0, i % 2) for i in range(15)]), [(11, 1, 2), (12, 2, 2)]), pairs=[])

# ---- both label vectors constant (cluster_num > 1): 1.0; one constant: 0; matching: 1; independent: negative, clamped
CASES["both_constant"] = dict(ds=make(pair_reads(13, 14, [(1, 0)] * 12), [(13, 2, 2), (14, 2, 2)]), pairs=[(13, 14)])
CASES["one_constant"] = dict(ds=make(pair_reads(15, 16, [(0, i % 2) for i in range(12)]), [(15, 2, 2), (16, 2, 2)]), pairs=[(15, 16)])
CASES["perfect_match"] = dict(ds=make(pair_reads(17, 18, MATCH), [(17, 2, 2), (18, 2, 2)]), pairs=[(17, 18)])
CASES["anti_correlated"] = dict(ds=make(pair_reads(19, 20, ANTI), [(19, 2, 2), (20, 2, 2)]), pairs=[(19, 20)])

# ---- an index of exactly ari_thr = 0.5: the table [[0, 0, 1], [1, 4, 0]] (6 reads, so count_thr 5); `<=` scores it as an error
_half = [(0, 2), (1, 0), (1, 1), (1, 1), (1, 1), (1, 1)]
CASES["ari_equals_threshold"] = dict(ds=make([[node(21, a, k=3), node(22, b, k=3)] for a, b in _half], [(21, 3, 2), (22, 3, 2)]),
                                     cfg=dict(count_thr=5), pairs=[(21, 22)], ari={(21, 22): 0.5})

# ---- the asymmetry of touch_chunks.  30-31-32 match each other (stiff).  29 contradicts 30 and is the SMALLER id of its pair:
# suspicious.  33 contradicts 32 and is the LARGER id: isolated.  28 contradicts 31 like 29 but has copy number 3: stiff.
_rel = pair_reads(30, 31, MATCH) + pair_reads(30, 32, MATCH) + pair_reads(31, 32, MATCH)
_rel += pair_reads(29, 30, ANTI) + pair_reads(32, 33, ANTI) + pair_reads(28, 31, ANTI)
CASES["suspicious_smaller_isolated_larger"] = dict(
    ds=make(_rel, [(28, 2, 3), (29, 2, 2), (30, 2, 2), (31, 2, 2), (32, 2, 2), (33, 2, 2)]),
    classes={28: STIFF, 29: SUSPICIOUS, 30: STIFF, 31: STIFF, 32: STIFF, 33: ISOLATED})

# ---- nothing survives; no read at all; no node at all
CASES["no_surviving_pair"] = dict(ds=make(pair_reads(34, 35, MATCH[:3]), [(34, 2, 2), (35, 2, 2)]), pairs=[])
CASES["no_reads"] = dict(ds=make([], [(34, 2, 2), (35, 2, 3)]), pairs=[], classes={34: ISOLATED, 35: STIFF})
CASES["empty_reads"] = dict(ds=make([[], [node(34, 0)], []], [(34, 2, 2)]), pairs=[])

# ---- a node on a chunk id outside chunks[]: harmless below the threshold, the reference's panic above it; not indexed at all
# when the other chunk already fails `1 < cluster_num` and comes first (:97 short-circuits)
CASES["stray_chunk_below_threshold"] = dict(ds=make(pair_reads(36, 99, MATCH[:10]) + pair_reads(36, 37, MATCH), [(36, 2, 2), (37, 2, 2)]),
                                            pairs=[(36, 37)])
CASES["stray_chunk_above_threshold"] = dict(ds=make(pair_reads(36, 99, MATCH[:11]) + pair_reads(36, 37, MATCH), [(36, 2, 2), (37, 2, 2)]),
                                            status=-6)
CASES["stray_chunk_smaller_id_above_threshold"] = dict(ds=make(pair_reads(2, 36, MATCH[:11]), [(36, 2, 2)]), status=-6)
CASES["stray_chunk_behind_single_cluster"] = dict(ds=make(pair_reads(36, 99, MATCH[:11]), [(36, 1, 2)]), pairs=[])

# ---- the table's limit: label 63 fits, label 64 does not
for _lab, _st in ((63, 0), (64, -3)):
    CASES["label_%d" % _lab] = dict(ds=make([[node(38, _lab if i % 2 else 0, k=70), node(39, i % 2)] for i in range(12)],
                                            [(38, 70, 2), (39, 2, 2)]), status=_st)
# a label of 64 hidden behind a smaller one in the same read still counts as unsupported
CASES["label_64_behind_minimum"] = dict(
    ds=make([[node(38, 0, k=70), node(39, i % 2), node(38, 64, k=70)] for i in range(12)], [(38, 70, 2), (39, 2, 2)]), status=-3)
# ... but not when the pair does not survive
CASES["label_64_below_threshold"] = dict(
    ds=make([[node(38, 64 if i % 2 else 0, k=70), node(39, i % 2)] for i in range(10)], [(38, 70, 2), (39, 2, 2)]), pairs=[])


# ---- a relationship graph with non-integer scores (summation order shows) on which the chain both rejects proposals
# (gen_bool draws) and meets diff >= 0 (p == 1: no draw): a ring of 9 matching chunks with chords of varying support, three
# contradicting hangers-on and a contradicting pair apart
def _graph_case():
    rng = random.Random(5)
    reads = []
    ring = list(range(40, 49))
    for i, u in enumerate(ring):
        for v in (ring[(i + 1) % 9], ring[(i + 3) % 9]):
            n = 11 + rng.randrange(9)
            reads += pair_reads(min(u, v), max(u, v), [(j % 2, j % 2) for j in range(n)])
    for u, v in ((49, 41), (39, 44), (50, 47), (51, 52)):
        reads += pair_reads(min(u, v), max(u, v), ANTI + ANTI[:rng.randrange(4)])
    rng.shuffle(reads)
    return make(reads, [(i, 2, 2) for i in range(39, 53)])


CASES["graph_fractional_scores"] = dict(ds=_graph_case(), cfg=dict(match_score=0.1, mismatch_score=-0.3, ari_thr=0.5))


# ---- one read of 300 nodes (more than a workgroup; 45,150 records from one read): count_thr 0 lets every pair of the 20
# two-cluster chunks survive with one observation each
def _long_read():
    order = list(range(100, 400))
    random.Random(7).shuffle(order)
    return make([[node(u, u % 2) for u in order]], [(u, 2 if u % 15 == 0 else 1, 2) for u in range(100, 400)])


CASES["one_read_of_300_nodes"] = dict(ds=_long_read(), cfg=dict(count_thr=0))


# ---- more reads than the per-read kernels have workgroups (1,024), more records than one launch has threads, more surviving
# pairs than the table kernel has workgroups (1,024): 4 reads over 300 chunks + 1,100 reads of two or three nodes; 50 chunks
# have two clusters -> 1,225 surviving pairs at count_thr 2
def _grid_case():
    rng = random.Random(11)
    two = [u for u in range(100, 400) if u % 6 == 0]
    reads = []
    for r in range(4):
        order = list(range(100, 400))
        rng.shuffle(order)
        reads.append([node(u, (u // 6 + r * (u % 4 == 0)) % 2) for u in order])
    for i in range(1100):
        us = rng.sample(two, 2 + i % 2)
        reads.append([node(u, rng.randrange(2)) for u in us])
    rng.shuffle(reads)
    return make(reads, [(u, 2 if u in two else 1, 2) for u in range(100, 400)])


CASES["beyond_every_grid"] = dict(ds=_grid_case(), cfg=dict(count_thr=2))

NAMES = sorted(CASES)
