"""Seeding and chaining restated in plain Python from DESIGN.md section 4, "Seeding and chaining (own spec; stands in for
minimap2)": canonical k-mers with their strand bit, the invertible hash, the minimizers with every tie kept, the index with its
occurrence cut, the hits, the single-linkage clusters along the diagonal and the placement records, and map_trials, the host
arithmetic that turns a placement into a window of jtk_lc_encode_nodes.  No numpy, nothing of jtk_amd: this is what the device's
answers are compared with, record for record.  Written from the specification, not from map.hip.

A worked example, k = 3, w = 2, on `ACGGT`: codes A C G T = 0 1 2 3, the first base lowest.  `ACG`: forward 0 + 1*4 + 2*16 = 36;
its reverse complement is `CGT` = 1 + 2*4 + 3*16 = 57; canonical 36, strand 0.  `CGG`: forward 1 + 8 + 32 = 41, reverse `CCG` =
1 + 4 + 32 = 37; canonical 37, strand 1.  `GGT`: forward 2 + 8 + 48 = 58, reverse `ACC` = 0 + 4 + 16 = 20; canonical 20, strand 1.
n = 3 positions, the windows are {0, 1} and {1, 2}; a position is kept where its hash is the least of a window that holds it."""

CODE = [4] * 256
for _i, _b in enumerate("ACGT"):
    CODE[ord(_b)] = CODE[ord(_b.lower())] = _i

HASH_C0, HASH_C1, HASH_C2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB   # all odd
MAX_K, MAX_W = 31, 64
MAX_TARGET_LEN, MAX_QUERY_LEN, MAX_TARGETS = 65535, 4000000, 1 << 25
ALLOWED_END_GAP = 25      # encode/mod.rs:14
OFFSET_FACTOR = 0.1       # deletion_fill.rs:293
FIELDS = ("query", "target", "is_forward", "n_seeds", "qstart", "qend", "oq_start", "oq_end", "tstart", "tend", "diag_lo", "diag_hi")


def hash_kmer(x, k):
    """a bijection of [0, 4^k): xor with a constant, then twice (multiply by an odd constant mod 4^k, xor the upper half down)"""
    m = (1 << (2 * k)) - 1
    h = (x ^ HASH_C0) & m
    h = (h * HASH_C1) & m
    h ^= h >> k
    h = (h * HASH_C2) & m
    h ^= h >> k
    return h


def canonical(seq, p, k):
    """(canonical k-mer, strand) of seq[p:p+k], or None where it holds a byte that is no base or equals its reverse complement"""
    f = r = 0
    for i in range(k):
        c = CODE[seq[p + i]]
        if c > 3:
            return None
        f |= c << (2 * i)
        r |= (3 - c) << (2 * (k - 1 - i))
    if f == r:
        return None
    return (f, 0) if f < r else (r, 1)


def hashes(seq, k):
    """per k-mer position (hash, strand) or None"""
    out = []
    for p in range(len(seq) - k + 1):
        c = canonical(seq, p, k)
        out.append(None if c is None else (hash_kmer(c[0], k), c[1]))
    return out


def _sliding(values, width, pick):
    """pick (min or max) over values[j:j+width] for every j with j + width <= len(values), by a monotone deque"""
    from collections import deque
    out, dq = [], deque()
    worse = (lambda a, b: a >= b) if pick is min else (lambda a, b: a <= b)
    for i, v in enumerate(values):
        while dq and worse(values[dq[-1]], v):
            dq.pop()
        dq.append(i)
        if dq[0] <= i - width:
            dq.popleft()
        if i >= width - 1:
            out.append(values[dq[0]])
    return out


def sketch(seq, k, w):
    """the minimizers of seq (bytes) as (pos, hash, strand), ascending by pos.  A window's minimum is at most the hash of any
    position it holds, so a position attains the minimum of some window that holds it iff the LARGEST of those windows' minima
    equals its hash: a sliding minimum, then a sliding maximum over the minima."""
    assert 1 <= k <= MAX_K and 1 <= w
    hs = hashes(seq, k)
    n = len(hs)
    if n <= 0:
        return []
    inf = 1 << 64
    vals = [inf if h is None else h[0] for h in hs]
    width = min(w, n)
    minima = _sliding(vals, width, min)                   # window j is positions j .. j + width - 1
    lo = -1                                               # position p lies in the windows max(p - width + 1, 0) .. min(p, n - width)
    padded = [lo] * (width - 1) + minima + [lo] * (width - 1)
    largest = _sliding(padded, width, max)                # largest[p]: over the windows that hold p
    return [(p, hs[p][0], hs[p][1]) for p in range(n) if hs[p] is not None and largest[p] == hs[p][0]]


def check_limits(targets, queries, k, w):
    """None, or the reason the device refuses the call with JTK_ERR_UNSUPPORTED"""
    if k > MAX_K:
        return "k"
    if w > MAX_W:
        return "w"
    if len(targets) > MAX_TARGETS:
        return "targets"
    if any(len(t) > MAX_TARGET_LEN for t in targets):
        return "target length"
    if any(len(q) > MAX_QUERY_LEN for q in queries):
        return "query length"
    return None


def map_reads(targets, queries, k=15, w=10, max_occ=200, max_gap=100, min_seeds=4, skip_self=False):
    """the placement records (dicts of FIELDS) of every query (bytes) on every target (bytes), in the order (query, target, rev,
    diag_lo)"""
    index = {}
    for t, seq in enumerate(targets):
        for pos, h, strand in sketch(seq, k, w):
            index.setdefault(h, []).append((t, pos, strand))
    out = []
    for qi, seq in enumerate(queries):
        qlen = len(seq)
        hits = []
        for q, h, strand in sketch(seq, k, w):
            recs = index.get(h, ())
            if len(recs) > max_occ:
                continue
            for t, tpos, tstrand in recs:
                if skip_self and t == qi:
                    continue
                rev = strand ^ tstrand
                oq = qlen - (q + k) if rev else q
                hits.append((t, rev, oq - tpos, tpos, oq))
        hits.sort()
        cluster = []
        for i, hit in enumerate(hits):
            if cluster and (hit[0] != cluster[-1][0] or hit[1] != cluster[-1][1] or hit[2] - cluster[-1][2] > max_gap):
                _report(out, qi, qlen, cluster, k, min_seeds)
                cluster = []
            cluster.append(hit)
        if cluster:
            _report(out, qi, qlen, cluster, k, min_seeds)
    return out


def _report(out, qi, qlen, cluster, k, min_seeds):
    n_seeds = len({h[3] for h in cluster})
    if n_seeds < min_seeds:
        return
    t, rev = cluster[0][0], cluster[0][1]
    tmin, tmax = min(h[3] for h in cluster), max(h[3] for h in cluster) + k
    qmin, qmax = min(h[4] for h in cluster), max(h[4] for h in cluster) + k
    out.append(dict(query=qi, target=t, is_forward=0 if rev else 1, n_seeds=n_seeds, qstart=qlen - qmax if rev else qmin,
                    qend=qlen - qmin if rev else qmax, oq_start=qmin, oq_end=qmax, tstart=tmin, tend=tmax,
                    diag_lo=min(h[2] for h in cluster), diag_hi=max(h[2] for h in cluster)))


def map_trials(placements, query_lens, target_lens, sim_thr):
    """Per placement that passes the end-gap filter, (index of the placement, start, end, is_forward, sim_thr): the window
    [start, end) of the read, in forward coordinates, that encode_node is tried on.  The chunk's ends are projected along the
    placement (est_start, est_end on the oriented read); an estimate that leaves the read by more than ALLOWED_END_GAP bases at
    either end is dropped; the rest is widened by ceil(OFFSET_FACTOR * tlen) per side and clipped to the read."""
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
        if not int(p["is_forward"]):
            start, end = qlen - end, qlen - start
        out.append((i, start, end, int(p["is_forward"]), float(sim_thr)))
    return out
