"""Named cases of jtk_lc_fill_candidates, each the smallest that shows its point.  A case is dict(reads, target, why); a read
is a list of nodes (chunk, cluster, is_forward, query_len, position) as tests/fill_reference.py takes them.  The same cases
serve the CPU tests of the reference and the GPU tests of the device against it."""
import random

import numpy as np

A, B, C, D, E, P, Q, S, X, Y = 10, 11, 12, 13, 14, 20, 21, 22, 30, 31


def read(keys, qlen=100, gap=10, start=0, positions=None):
    """keys: chunk ids, or (chunk, cluster) or (chunk, cluster, is_forward); nodes of `qlen` bases `gap` apart from `start`."""
    nodes, pos = [], start
    for i, k in enumerate(keys):
        k = (k,) if isinstance(k, int) else tuple(k)
        chunk, cluster, fwd = k[0], (k[1] if len(k) > 1 else 0), (k[2] if len(k) > 2 else True)
        if positions is not None:
            pos = positions[i]
        nodes.append((chunk, cluster, bool(fwd), qlen, pos))
        pos += qlen + gap
    return nodes


def reverse(nodes, length=None):
    """the same read seen from the other strand: node order reversed, directions flipped, positions mirrored"""
    length = length if length is not None else max(p + q for (_, _, _, q, p) in nodes) + 7
    return [(c, k, not f, q, length - (p + q)) for (c, k, f, q, p) in reversed(nodes)]


def case(reads, why, target=None):
    return dict(reads=reads, target=target, why=why)


CASES = {}
CASES["identical"] = case([read([A, B, C]), read([A, B, C])], "two identical 3-node reads: coverage only")
for _l, _ins in ((1, [X]), (2, [X, Y]), (3, [X, Y, P])):
    CASES["middle_insertion_%d" % _l] = case([read([A, B]), read([A] + _ins + [B])],
                                             "Ins(%d) in the middle: first node to head, last to tail from length 2" % _l)
CASES["leading_insertion"] = case([read([A, B]), read([X, Y, A, B])], "Ins at position 0: only the last inserted node, to the tail list")
CASES["trailing_insertion"] = case([read([A, B]), read([A, B, X, Y])],
                                   "Ins at position == n: the wrapped arm; head entry at slot n, the tail entry there is never looked at")
CASES["half_arm_n3"] = case([read([A, B, C]), read([A, X, Y, B, C])], "2 * position + 1 == n: Ins(2) at slot 1 of n = 3 gives NO tail entry")
CASES["half_arm_n4"] = case([read([A, B, C, D]), read([A, X, Y, B, C, D])], "the same insertion in n = 4: head and tail")
CASES["reverse_query"] = case([read([A, B, C]), reverse(read([A, X, Y, B, C], gap=17))], "a query on the other strand, offsets swapped")
CASES["direction_tie"] = case([read([(A, 0, True), (A, 0, False)]), read([(A, 0, True), (A, 0, False)], gap=3)],
                              "forward and reverse counts tie: forward wins")
CASES["cluster_mismatch"] = case([read([A, B, C, D]), read([A, (B, 1), X, C, D])], "a -1 column inside a passing alignment")
CASES["reject_score"] = case([read([X, A, B]), read([Y, A, B])],
                             "pre-filter passes (2 keys) but no dovetail path reaches the matches: score 0 < 1")
CASES["reject_matched"] = case([read([A, B]), read([B, A])], "score 1 with one matched node < min(2, n, m)")
CASES["reject_ins_del"] = case([read([A, B, X, C, D]), read([A, B, Y, C, D])], "matched 2, score 1, but the end gaps put an Ins next to a Del")
CASES["one_node_target"] = case([read([A]), read([X, A, Y]), read([A, B])], "min_match = 1 for a 1-node target")
CASES["tandem_short"] = case([read([A, A, A]), read([A, A])], "A A A against A A: every tie-break decides")
CASES["tandem_mixed"] = case([read([A, A, A]), read([A, B, A]), read([A, A, B, A, A])], "A A A against A B A")
CASES["offset_truncates"] = case([read([A, B]), read([A, X, B], positions=[0, 97, 250]), read([A, X, B], positions=[0, 96, 250]),
                                  read([Y, A, B], positions=[0, 97, 300]), read([Y, A, B], positions=[0, 96, 300])],
                                 "head offsets -3, -4 and tail offsets -3, -4: the mean is -3 truncated, -4 floored")
CASES["negative_head"] = case([read([A, B], qlen=2), read([A, X, B], positions=[0, 90, 300])], "head position 2 - 10 = -8, written signed")
CASES["tail_clamped"] = case([read([A, B], start=5), read([X, A, B], positions=[0, 150, 300])], "tail position max(5 - 50, 0)")
for _mean, _total in ((4, 6), (5, 7), (9, 12), (10, 14)):    # mean_cov = 3 * total / 4: n = 3, every read covers three slots
    CASES["mean_cov_%d" % _mean] = case([read([A, B, C])] + [read([A, X, B, C])] * 2 + [read([A, Y, B, C])] + [read([A, B, C])] * (_total - 4),
                                        "mean_cov %d: key X is entered twice, key Y once, against ins_thr %d" % (_mean, min(_mean // 5, 2)),
                                        target=[1] + [0] * (_total - 1))
CASES["offsets_all_none"] = case([read([A, B]), read([A, B, X]), read([A, B, X, Y])],
                                 "the only entries without an offset: a query's last node, in the tail list of slot n (which is dropped)")
CASES["target_mask"] = case([read([A, B, C]), read([A, X, B, C]), read([A, B, Y, C]), read([B, C])], "only reads 1 and 3 get output",
                            target=[0, 1, 0, 1])
CASES["empty_query"] = case([read([A, B]), [], read([A, X, B]), []], "reads without nodes: no target, no query")


def _long(n, seed):
    """a read of n distinct chunks and a copy that lost and gained a few nodes"""
    rng = random.Random(seed)
    base = read(list(range(100, 100 + n)), gap=12)
    other, pos = [], 3
    for (c, k, f, q, _) in base:
        u = rng.random()
        if u < 0.08:
            continue
        if u > 0.94:
            other.append((1000 + c, 0, True, 80, pos))
            pos += 95
        other.append((c, 1 if u > 0.9 else 0, f, q, pos))
        pos += q + rng.randrange(5, 25)
    return base, other


for _n in (65, 130):
    _b, _o = _long(_n, 12)
    CASES["long_%d" % _n] = case([_b, _o, reverse(_o)], "%d nodes: more columns than lanes" % _n)
# the pair kernel keeps a pair in 8192 bytes of LDS: 24 (m + 1) + 4 (n + m + 2) + n ((m + 1) / 2) is 8150 at n = m = 99 and 8232 at 100
for _n in (99, 100):
    _b, _o = _long(_n, 12)
    CASES["lds_boundary_%d" % _n] = case([_b, _o], "n = m = %d: %s the LDS boundary" % (_n, "below" if _n == 99 else "above"))

RANDOM_SEED = 20240611


def random_family(seed=RANDOM_SEED, n_reads=200, n_chunks=40, dropout=0.15):
    """200 reads over 40 chunks of 1-3 clusters, both strands, nodes dropped at 15 % so that candidates exist"""
    rng = random.Random(seed)
    n_clusters = [rng.randrange(1, 4) for _ in range(n_chunks)]
    reads = []
    for _ in range(n_reads):
        first, length, hap = rng.randrange(0, n_chunks - 6), rng.randrange(6, 15), rng.randrange(0, 3)
        nodes, pos = [], rng.randrange(0, 50)
        for c in range(first, min(first + length, n_chunks)):
            q = 100 + rng.randrange(-6, 7)
            if rng.random() >= dropout:
                nodes.append((c, hap % n_clusters[c], True, q, pos))
            pos += q + rng.randrange(-8, 30)
        if not nodes:
            nodes.append((first, 0, True, 100, 0))
        reads.append(reverse(nodes, pos + 11) if rng.random() < 0.5 else nodes)
    return reads


CASES["random_family"] = case(random_family(), "seeded: 200 reads, 40 chunks, both strands, 15 % drop-outs")


def flatten(reads):
    """node_off (uint64) and a list of node tuples in the field order of jtk_fill_node_t"""
    node_off = np.zeros(len(reads) + 1, dtype=np.uint64)
    flat = []
    for r, nodes in enumerate(reads):
        flat += [(c, k, int(f), q, p) for (c, k, f, q, p) in nodes]
        node_off[r + 1] = len(flat)
    return node_off, flat
