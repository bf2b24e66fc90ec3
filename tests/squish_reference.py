"""An independent restatement of squish_erroneous_clusters, in plain Python (test infrastructure).

Written from the Rust alone -- haplotyper/src/squish_erroneous_clusters.rs, misc::adjusted_rand_index (misc.rs:22-46) and
Node::is_biased (definitions/src/lib.rs:703-709) -- and NOT from jtk_amd/csrc/squish.hip.  It works on the DataSet-like structure of
tests/correction_reference.py,

    ds = dict(reads=[dict(id=..., nodes=[dict(chunk=, cluster=, is_forward=, posterior=[...]), ...]), ...],
              chunks=[dict(id=, cluster_num=, copy_num=, score=), ...])

and follows the Rust's shape, not the library's: a dictionary of pair counts filled position pair by position pair, label lists
per pair, a contingency table sized by the largest label, Python integers masked to 64 bits where the Rust wraps.

`exp` is a parameter (tests/clustering_reference.py: LibmMath, or ProjectMath = include/jtk_math.h through the oracle's jo_exp).

Where the reference has no order.  Its pair list is what `par_iter` over a HashMap yields: the node numbering inside classify, the
sweep order of wipe_through, the proposal targets and the order of the float sums follow from it and differ from process to
process.  This file uses the order the library documents: pairs ascending by (u1, u2).  `classify` itself takes the list in the
order given.

Not in the reference tree, restated from the crates' published sources (parity with the crates themselves is unpinned):
  Xoshiro256PlusPlus  seed_from_u64 = four SplitMix64 outputs; next_u64 = rotl(s0 + s3, 23) + s0, then t = s1 << 17, s2 ^= s0,
                      s3 ^= s1, s1 ^= s2, s0 ^= s3, s2 ^= t, s3 = rotl(s3, 45)
  gen_range(0..n)     usize: zone = (n << lzcnt(n)) - 1; the first v with lo(v * n) <= zone gives hi(v * n) (64-bit draws)
  gen_bool(p)         p == 1 never draws; otherwise next_u64() < (p * 2^64) as u64

A reference panic (an index into `chunks` that is not there) raises ReferencePanic; `squish` reports it as status -6 with nothing
written.  The library's own limit (a label of 64 or more in a surviving pair's table) is status -3.
"""
M64 = (1 << 64) - 1
BIAS_THR = 0.2
STIFF, ISOLATED, SUSPICIOUS = 0, 1, 2
DEFAULT_CONFIG = dict(ari_thr=0.5, match_score=4.0, mismatch_score=-1.0, count_thr=10)   # :29-38
MAX_LABEL = 64


class ReferencePanic(Exception):
    pass


def _rotl(x, k):
    return ((x << k) | (x >> (64 - k))) & M64


class Xoshiro256PlusPlus:
    def __init__(self, s):
        self.s = list(s)

    @classmethod
    def seed_from_u64(cls, seed):
        out, x = [], seed & M64
        for _ in range(4):   # SplitMix64
            x = (x + 0x9E3779B97F4A7C15) & M64
            z = x
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
            out.append(z ^ (z >> 31))
        return cls(out)

    def next_u64(self):
        s = self.s
        r = (_rotl((s[0] + s[3]) & M64, 23) + s[0]) & M64
        t = (s[1] << 17) & M64
        s[2] ^= s[0]
        s[3] ^= s[1]
        s[1] ^= s[2]
        s[0] ^= s[3]
        s[2] ^= t
        s[3] = _rotl(s[3], 45)
        return r


class Rand085:
    """gen_range(0..n) on usize and gen_bool of rand 0.8.5; `draws` counts next_u64 calls, `no_draw` the p == 1 returns"""

    def __init__(self, core):
        self.core, self.draws, self.no_draw, self.rejected = core, 0, 0, 0

    def _next(self):
        self.draws += 1
        return self.core.next_u64()

    def gen_range(self, n):
        if n < 1:
            raise ReferencePanic("gen_range on an empty range")
        zone = ((n << (64 - n.bit_length())) - 1) & M64
        while True:
            m = self._next() * n
            if (m & M64) <= zone:
                return m >> 64

    def gen_bool(self, p):
        if p == 1.0:
            self.no_draw += 1
            return True
        if not 0.0 <= p < 1.0:
            raise ReferencePanic("gen_bool: p outside [0, 1]")
        hit = self._next() < int(p * 18446744073709551616.0)
        self.rejected += not hit
        return hit


def is_biased(node, exp, thr=BIAS_THR):
    """definitions/src/lib.rs:703-709"""
    post = node["posterior"]
    if len(post) <= 1:
        return True
    thr = 1.0 / float(len(post)) + thr
    return any(thr <= exp(x) for x in post)


def choose(x):
    return ((max(x, 1) - 1) * x & M64) // 2


def adjusted_rand_index(label, pred):
    """misc.rs:22-46 in wrapping u64 / i64 arithmetic"""
    assert len(label) == len(pred) and len(label) > 0
    cont = [[0] * (max(pred) + 1) for _ in range(max(label) + 1)]
    lab_sum, pred_sum = [0] * (max(label) + 1), [0] * (max(pred) + 1)
    for a, b in zip(label, pred):
        cont[a][b] += 1
        lab_sum[a] += 1
        pred_sum[b] += 1
    lab_match = sum(choose(x) for x in lab_sum) & M64
    pred_match = sum(choose(x) for x in pred_sum) & M64
    num_of_pairs = choose(len(label))
    both_match = sum(choose(x) for row in cont for x in row) & M64
    if not both_match <= ((lab_match + pred_match) & M64) // 2:
        raise ReferencePanic("adjusted_rand_index: assert both_match <= (lab_match + pred_match) / 2")

    def i64(x):
        x &= M64
        return x - (1 << 64) if x >> 63 else x
    match_prod = i64(lab_match * pred_match)
    denom = i64(i64(((num_of_pairs * ((lab_match + pred_match) & M64)) & M64) // 2) - match_prod)
    numer = i64(i64(num_of_pairs * both_match) - match_prod)
    if denom == 0:   # f64 division by zero
        return float("nan") if numer == 0 else (float("inf") if numer > 0 else float("-inf"))
    return float(numer) / float(denom)   # int -> float rounds to nearest even, like `as f64`


def biased_nodes(ds, exp):
    """per read, the (chunk, cluster) of its biased nodes in read order: what every loop of the Rust filters down to"""
    return [[(n["chunk"], n["cluster"]) for n in read["nodes"] if is_biased(n, exp)] for read in ds["reads"]]


def pair_counts(biased):
    """:80-90"""
    counts = {}
    for nodes in biased:
        for i, (ch1, _) in enumerate(nodes):
            for ch2, _ in nodes[i + 1:]:
                key = (min(ch1, ch2), max(ch1, ch2))
                counts[key] = counts.get(key, 0) + 1
    return counts


def check_correl(by_chunk, u1, cl1, u2, cl2):
    """:213-252 on by_chunk = per read {chunk: [clusters of its biased nodes]} -> (ari, observations)"""
    c1, c2 = [], []
    for seen in by_chunk:
        a, b = seen.get(u1), seen.get(u2)
        if a and b:
            c1.append(min(a))
            c2.append(min(b))
    if not c1:
        return 0.0, 0
    same = all(x == c1[0] for x in c1) and all(x == c2[0] for x in c2)
    if same:
        rel = 0.0 if (cl1 == 1 and cl2 == 1) else 1.0
    else:
        rel = adjusted_rand_index(c1, c2)
    if rel != rel:
        return 0.0, len(c1)
    return rel, len(c1)


def classify(pairs, cfg, exp, stats=None):
    """:254-365 on [(u1, u2, ari, count)] in the order given -> (ids in first-appearance order, their assignments)"""
    index = {}
    for u1, u2, _, _ in pairs:
        index.setdefault(u1, len(index))
        index.setdefault(u2, len(index))
    graph = [[] for _ in index]
    for u1, u2, ari, count in pairs:
        ari = min(max(ari, 0.0), 1.0)
        a, b = index[u1], index[u2]
        graph[a].append((b, ari, count))
        graph[b].append((a, ari, count))

    def score(ari, count):   # ClassifyParam::new(ari_thr, mismatch_score, match_score) :269, :299-304
        return cfg["mismatch_score"] * float(count) if ari <= cfg["ari_thr"] else cfg["match_score"] * float(count)

    asn = [True] * len(index)

    def diff_on_flip(t):
        total = 0.0
        for to, ari, count in graph[t]:
            if asn[to]:
                total = total + score(ari, count)
        return -total if asn[t] else total

    rng = Rand085(Xoshiro256PlusPlus.seed_from_u64(3093240))
    for _ in range(10):
        for i in range(len(asn)):        # wipe_through
            if 0.0 < diff_on_flip(i):
                asn[i] = not asn[i]
        for _ in range(1000):            # mcmc
            i = rng.gen_range(len(asn))
            diff = diff_on_flip(i)
            if rng.gen_bool(exp(min(diff, 0.0))):
                asn[i] = not asn[i]
    if stats is not None:
        stats.update(draws=rng.draws, no_draw=rng.no_draw, rejected=rng.rejected)
    return list(index), asn


def squish(ds, cfg=None, exp=None, stats=None):
    """squish_erroneous_clusters on `ds` (not modified) -> dict(status, pairs=[(u1, u2, ari, count)] ascending, counts,
    classes per chunk of ds["chunks"], cluster_num per chunk, cluster and touched per node in read order)"""
    import math
    cfg = dict(DEFAULT_CONFIG, **(cfg or {}))
    exp = exp or math.exp
    out = dict(status=0, pairs=[], classes=None, cluster_num=None, cluster=None, touched=None)
    biased = biased_nodes(ds, exp)
    counts = pair_counts(biased)
    by_chunk = []
    for nodes in biased:
        seen = {}
        for ch, cl in nodes:
            seen.setdefault(ch, []).append(cl)
        by_chunk.append(seen)
    chunks = {c["id"]: c["cluster_num"] for c in ds["chunks"]}
    kept = {k: v for k, v in counts.items() if cfg["count_thr"] < v}
    try:
        kept = {k: v for k, v in kept.items() if 1 < chunks[k[0]] and 1 < chunks[k[1]]}   # KeyError: the reference's panic
    except KeyError:
        out["status"] = -6
        return out
    pairs = []
    for u1, u2 in sorted(kept):          # the documented order
        rel, n = check_correl(by_chunk, u1, chunks[u1], u2, chunks[u2])
        for seen in by_chunk:            # the library's limit: a read that enters the table, every biased node of either chunk
            if u1 in seen and u2 in seen and max(seen[u1] + seen[u2]) >= MAX_LABEL:
                out["status"] = -3
                return out
        pairs.append((u1, u2, rel, n))
    out["pairs"], out["counts"] = pairs, kept
    touch = {}
    for u1, u2, _, _ in pairs:
        touch.setdefault(u1, []).append(u2)
    stiff = set()
    if pairs:
        ids, asn = classify(pairs, cfg, exp, stats)
        stiff = {u for u, a in zip(ids, asn) if a}
    classes = []
    for c in ds["chunks"]:
        if c["id"] in stiff or 2 < c["copy_num"]:
            classes.append(STIFF)
        elif c["id"] in touch and any(t in stiff for t in touch[c["id"]]):
            classes.append(SUSPICIOUS)
        else:
            classes.append(ISOLATED)
    class_of = {c["id"]: k for c, k in zip(ds["chunks"], classes)}   # (a HashMap: the last of equal ids wins)
    out["classes"] = classes
    out["cluster_num"] = [1 if class_of[c["id"]] == SUSPICIOUS else c["cluster_num"] for c in ds["chunks"]]
    out["cluster"], out["touched"] = [], []
    for read in ds["reads"]:
        for n in read["nodes"]:
            hit = class_of.get(n["chunk"]) == SUSPICIOUS
            out["cluster"].append(0 if hit else n["cluster"])
            out["touched"].append(1 if hit else 0)
    return out


def written_back(ds, res):
    """the DataSet after the step: :45-59 applied from a result of `squish` (or of the library, in the same shape)"""
    new = dict(ds, reads=[], chunks=[dict(c, cluster_num=int(k)) for c, k in zip(ds["chunks"], res["cluster_num"])])
    e = 0
    for read in ds["reads"]:
        nodes = []
        for n in read["nodes"]:
            nodes.append(dict(n, cluster=0, posterior=[0.0]) if res["touched"][e] else dict(n))
            e += 1
        new["reads"].append(dict(read, nodes=nodes))
    return new
