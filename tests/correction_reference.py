"""An independent restatement of the cross-chunk correction, in plain Python (test infrastructure).

Written from the Rust alone -- haplotyper/src/phmm_likelihood_correction.rs:31-566, misc.rs (kmeans :229-341, logsumexp :84-92,
adjusted_rand_index :22-46) and Node::is_biased (definitions/src/lib.rs:703-709) -- and NOT from oracle/correction.c or
jtk_amd/csrc/correction.hip, which were written by one hand from one reading.  It works on a DataSet-like structure

    ds = dict(reads=[dict(id=..., nodes=[dict(chunk=, cluster=, is_forward=, posterior=[...]), ...]), ...],
              chunks=[dict(id=, cluster_num=, copy_num=, score=), ...],          # selected_chunks, in their order
              coverage=haploid coverage)

and is shaped differently from the C wherever the Rust allows: dictionaries and lists instead of flattened arrays, the whole
(len1+1) x (len2+1) x 3 table in align_swg instead of two rolling rows, a max-shifted sum instead of the streaming LogSumExp
recurrence in sim, f64::ln_1p as log1p (the C evaluates log(1 + x)), LAPACK instead of Jacobi.

What is NOT in the reference tree and therefore stays unpinned against the crates themselves:
  * nalgebra's symmetric_eigen: `eigen=` is a parameter.  numpy.linalg.eigh is the default and fully independent; the test
    modules can pass the oracle's Jacobi (jo_symmetric_eigen) instead, which gives the oracle's basis, so that everything
    downstream can be compared label for label (two haplotypes joined only by the 1e-16 links give two eigenvalues that are
    degenerate to working precision; the basis inside that eigenspace is arbitrary and normalize_columns is not
    rotation-invariant).
  * rand 0.8.5 / rand_xoshiro 0.6.0: restated below in Python integers from the crates' published sources.  The spec used:
      Xoroshiro128PlusPlus  seed_from_u64 = two SplitMix64 outputs; next_u64 = rotl(s0 + s1, 17) + s0, s1 ^= s0,
                            s0 = rotl(s0, 49) ^ s1 ^ (s1 << 21), s1 = rotl(s1, 28); next_u32 = the low half of next_u64
      gen_bool(p)           p == 1 never draws; otherwise next_u64() < (p * 2^64) as u64
      gen_range(0..n)       usize: zone = (n << lzcnt(n)) - 1; first v with lo(v * n) <= zone gives hi(v * n) (64-bit draws)
      SliceRandom::choose   gen_index(len): the same rejection in 32 bits on next_u32 when len <= u32::MAX
      choose_weighted       WeightedIndex<f64>::new: cumulative[i-1] = w[0] + ... + w[i-1] for i = 1..n-1 (the running total
                            BEFORE adding w[i]), total = the sum of all; a weight that is not >= 0, no item, or total == 0 is an
                            error (the caller unwraps: a panic).  UniformFloat::new(0, total): scale = total, lowered one ulp at
                            a time while scale * (1 - 2^-52) + 0 >= total.  One draw: value1_2 = the float with exponent 0 and
                            mantissa next_u64() >> 12, chosen = (value1_2 - 1) * scale + 0.  The index is the number of
                            cumulative weights that are <= chosen (partition point).
    tests/test_oracle_pinning.py states the same spec for gen_range / gen_index / gen_bool.  Parity with the crates themselves
    is unpinned (they are not on the build machine); `kmeans` and `Rand085` are importable on their own -- misc::kmeans is also
    the Metropolis chain's seeding (pseudo_mcmc.rs:657).
  * estimate_minimum_gain (kiley's simulator): the minimum gain is an input.

A reference panic (assert!, unwrap on None, index out of bounds, division by zero) raises ReferencePanic; `correct` reports it
as status -6 with nothing written, like the C entry points.

The reference's own error.  tests/test_correction_reference.py::test_reference_against_mpmath evaluates `sim` and `alignment`
in mpmath at 50 digits on the pairs of the test problems (saturated and single-cluster branches included):
    REF_VS_MPMATH = 1.5e-15 is the largest |float - mpmath| over the similarities (values in [0, 1], absolute);
    the largest over `sim` itself (values up to 80 in magnitude) is 7.2e-15.

Conditioning: for lnp within about 1e-9 of 0, short of the UPPER_THR saturation, lnp - ln_1p(-exp(lnp)) is ill-conditioned in
any double evaluation (lnp carries an absolute error of 1e-16); the figures above hold for posteriors <= -1e-6 or saturated.
"""
import math
import struct

import numpy as np

M64 = (1 << 64) - 1
NODE_DT = np.dtype([("chunk", "<u8"), ("cluster", "<u8"), ("is_forward", "<u4"), ("post_len", "<u4"), ("post_off", "<u8")])
CHUNK_DT = np.dtype([("id", "<u8"), ("cluster_num", "<u4"), ("copy_num", "<u4"), ("score", "<f8")])

REF_VS_MPMATH = 1.5e-15


class ReferencePanic(Exception):
    pass


def _require(cond, what):
    if not cond:
        raise ReferencePanic(what)


# ---------------------------------------------------------------------------------------------------------------------------
# rand_xoshiro 0.6.0 Xoroshiro128PlusPlus and the sampling layer of rand 0.8.5 (spec in the module docstring)
# ---------------------------------------------------------------------------------------------------------------------------
def _rotl(x, k):
    return ((x << k) | (x >> (64 - k))) & M64


class Xoroshiro128PlusPlus:
    def __init__(self, s0, s1):
        self.s0, self.s1 = s0, s1

    @classmethod
    def seed_from_u64(cls, seed):
        out = []
        x = seed & M64
        for _ in range(2):  # SplitMix64
            x = (x + 0x9E3779B97F4A7C15) & M64
            z = x
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
            out.append(z ^ (z >> 31))
        return cls(*out)

    def next_u64(self):
        s0, s1 = self.s0, self.s1
        r = (_rotl((s0 + s1) & M64, 17) + s0) & M64
        s1 ^= s0
        self.s0 = _rotl(s0, 49) ^ s1 ^ ((s1 << 21) & M64)
        self.s1 = _rotl(s1, 28)
        return r

    def next_u32(self):
        return self.next_u64() & 0xFFFFFFFF


class Rand085:
    """the calls misc::kmeans makes on `R: Rng`, over any generator with next_u64 / next_u32"""

    def __init__(self, core):
        self.core = core

    def gen_bool(self, p):
        if p == 1.0:
            return True
        _require(0.0 <= p < 1.0, "gen_bool: Bernoulli::new(p).unwrap() with p outside [0, 1]")  # a NaN included
        return self.core.next_u64() < int(p * 18446744073709551616.0)

    def choose_iter(self, items):
        """IteratorRandom::choose on an iterator whose size_hint is (0, Some(_)), such as a Filter: the reservoir path, one
        gen_index(consumed) per element, an element replacing the result when the index is 0.  None for no element."""
        result, consumed = None, 0
        for elem in items:
            consumed += 1
            if self.gen_index(consumed) == 0:
                result = elem
        return result

    def _range(self, n, bits, draw):
        zone = ((n << (bits - n.bit_length())) - 1) & ((1 << bits) - 1)
        while True:
            m = draw() * n
            if (m & ((1 << bits) - 1)) <= zone:
                return m >> bits

    def gen_range(self, n):  # gen_range(0..n) on usize
        _require(n >= 1, "gen_range on an empty range")
        return self._range(n, 64, self.core.next_u64)

    def gen_index(self, ubound):
        if ubound <= 0xFFFFFFFF:
            _require(ubound >= 1, "gen_range on an empty range")
            return self._range(ubound, 32, self.core.next_u32)
        return self.gen_range(ubound)

    def choose(self, n):  # SliceRandom::choose on a slice of length n: its index, None when empty
        return None if n == 0 else self.gen_index(n)

    def choose_weighted(self, weights):  # index, or None for a WeightedError
        if len(weights) == 0 or not weights[0] >= 0.0:
            return None
        cumulative, total = [], weights[0]
        for w in weights[1:]:
            if not w >= 0.0:
                return None
            cumulative.append(total)
            total += w
        if total == 0.0:
            return None
        scale, max_rand = total, 1.0 - 2.0 ** -52
        while scale * max_rand + 0.0 >= total:
            scale = struct.unpack("<d", struct.pack("<Q", struct.unpack("<Q", struct.pack("<d", scale))[0] - 1))[0]
        value1_2 = struct.unpack("<d", struct.pack("<Q", (self.core.next_u64() >> 12) | (1023 << 52)))[0]
        chosen = (value1_2 - 1.0) * scale + 0.0
        lo, hi = 0, len(cumulative)
        while lo < hi:  # partition point of `w <= chosen`
            mid = (lo + hi) // 2
            if cumulative[mid] <= chosen:
                lo = mid + 1
            else:
                hi = mid
        return lo


# ---------------------------------------------------------------------------------------------------------------------------
# misc.rs
# ---------------------------------------------------------------------------------------------------------------------------
def logsumexp(xs):
    """misc::logsumexp :84-92"""
    if len(xs) == 0:
        return 0.0
    m = max(xs)
    s = math.log(sum(math.exp(x - m) for x in xs))
    _require(s >= 0.0, "logsumexp: assert sum >= 0")
    return m + s


def adjusted_rand_index(label, pred):
    """misc::adjusted_rand_index :22-46 (usize / i64 arithmetic; 0 / 0 is NaN)"""
    _require(len(label) == len(pred), "ARI lengths")
    _require(len(label) > 0, "ARI of nothing: max().unwrap()")
    table = {}
    for a, b in zip(label, pred):
        table[(a, b)] = table.get((a, b), 0) + 1
    rows, cols = {}, {}
    for (a, b), c in table.items():
        rows[a] = rows.get(a, 0) + c
        cols[b] = cols.get(b, 0) + c
    pairs = lambda x: (max(x, 1) - 1) * x // 2
    lab_match, pred_match = sum(map(pairs, rows.values())), sum(map(pairs, cols.values()))
    both_match = sum(map(pairs, table.values()))
    _require(both_match <= (lab_match + pred_match) // 2, "ARI assert")
    prod = lab_match * pred_match
    denom = pairs(len(label)) * (lab_match + pred_match) // 2 - prod
    numer = pairs(len(label)) * both_match - prod
    if denom == 0:
        return float("nan") if numer == 0 else math.copysign(float("inf"), numer)
    return numer / denom


KMEANS_UPDATE_THR = 0.00000001


def kmeans(data, k, rng):
    """misc::kmeans :229-341 on an (n, dim) array and a Rand085; returns (residual, assignments)"""
    data = np.asarray(data, dtype=np.float64)
    _require(k >= 1, "kmeans: assert 1 <= k")
    n, dim = data.shape
    _require(dim > 0, "kmeans: assert 0 < dim")

    def nearest(centers):  # update_assignments: min_by is the first minimum, as is argmin
        d = ((data[:, None, :] - np.asarray(centers)[None, :, :]) ** 2).sum(axis=2)
        return d.argmin(axis=1)

    if rng.gen_bool(0.5):
        asn = np.array([rng.gen_range(k) for _ in range(n)], dtype=np.int64)
    else:  # suggest_first
        _require(k <= n, "suggest_first: assert k <= len")
        centers = [data[rng.choose(n)]]
        for _ in range(k - 1):
            dists = ((data[:, None, :] - np.asarray(centers)[None, :, :]) ** 2).sum(axis=2).min(axis=1)
            idx = rng.choose_weighted(dists.tolist())
            _require(idx is not None, "choose_weighted: WeightedError unwrapped")
            centers.append(data[idx])
        asn = nearest(centers)
    centers = np.zeros((k, dim))
    residual = lambda: float(((data - centers[asn]) ** 2).sum(axis=1).sum())
    dist = residual()
    while True:
        counts = np.bincount(asn, minlength=k)
        centers = np.zeros((k, dim))
        np.add.at(centers, asn, data)
        centers[counts > 0] /= counts[counts > 0, None]
        asn = nearest(centers)
        new_dist = residual()
        _require(new_dist < dist + KMEANS_UPDATE_THR, "kmeans: the residual grew")
        if dist - new_dist < KMEANS_UPDATE_THR:
            break
        dist = new_dist
    return dist, [int(a) for a in asn]


# ---------------------------------------------------------------------------------------------------------------------------
# arithmetic back ends: floats (the reference as the Rust runs it) and mpmath (the reference's own error)
# ---------------------------------------------------------------------------------------------------------------------------
class FloatMath:
    exp, log, log1p = staticmethod(math.exp), staticmethod(math.log), staticmethod(math.log1p)
    num = staticmethod(float)

    @staticmethod
    def safe_exp(x):
        try:
            return math.exp(x)
        except OverflowError:
            return float("inf")


class MpMath:
    def __init__(self, digits=50):
        import mpmath
        self.mp = mpmath
        mpmath.mp.dps = digits
        self.exp, self.log, self.log1p, self.num = mpmath.exp, mpmath.log, mpmath.log1p, mpmath.mpf
        self.safe_exp = mpmath.exp


MOCK_CP = 1.5
LOWER_CUT, UPPER_CUT, UPPER_THR = -80.0, 80.0, -1.8e-35
GAP_OPEN, GAP_EXTEND, MISM = -0.5, -100.0, -100.0


def _count(stats, key, by=1):
    if stats is not None:
        stats[key] = stats.get(key, 0) + by


def logit_from_lnp(lnp, B=FloatMath, stats=None):
    """:553-566"""
    _require(lnp <= 0, "logit_from_lnp: assert lnp <= 0")
    if lnp < LOWER_CUT:
        _count(stats, "lower_cut")
        return B.num(LOWER_CUT)
    if UPPER_THR < lnp:
        _count(stats, "upper_cut")
        return B.num(UPPER_CUT)
    _count(stats, "logit_interior")
    return lnp - B.log1p(-B.exp(lnp))


def sim(xs, ys, cps, B=FloatMath, stats=None):
    """:534-550; the log-sum-exp is a max-shifted sum, not the streaming recurrence"""
    _require(len(xs) == len(cps), "sim: posterior length differs from the copy-number vector's")
    _require(len(xs) == len(ys), "sim: posterior lengths differ")
    if len(cps) == 1:
        total = cps[0]
        _count(stats, ("single_cluster", float(total)))
        return -B.log(B.num(max(total, MOCK_CP)) - 1)
    terms = [B.num(x) + B.num(y) - B.log(B.num(cp)) for x, y, cp in zip(xs, ys, cps)]
    top = max(terms)
    lnp = top + B.log(sum(B.exp(t - top) for t in terms))
    if stats is not None and lnp == 0 and all(cp == 1.0 for cp in cps):
        _count(stats, "lnp_zero_with_cp_one")
    logit = logit_from_lnp(lnp, B, stats)
    _require(not (logit == float("inf") or logit == float("-inf")), "sim: infinite logit")
    return logit


def align_swg(arm1, arm2, copy_numbers, B=FloatMath, stats=None, memo=None, want_table=False):
    """:482-531 with the whole table.  arm = [(chunk id, posterior, key), ...]; `memo` caches sim by the two keys."""
    len1, len2 = len(arm1), len(arm2)
    lower = B.num((len1 + len2 + 2) * MISM)
    dp = [[[lower, lower, lower] for _ in range(len2 + 1)] for _ in range(len1 + 1)]  # match, del on arm2, del on arm1
    for i in range(1, len1 + 1):
        dp[i][0][2] = B.num(GAP_OPEN + (i - 1) * GAP_EXTEND)
    for j in range(1, len2 + 1):
        dp[0][j][1] = B.num(GAP_OPEN + (j - 1) * GAP_EXTEND)
    dp[0][0][0] = B.num(0.0)
    matches = 0
    for i in range(1, len1 + 1):
        u1, p1, k1 = arm1[i - 1]
        for j in range(1, len2 + 1):
            u2, p2, k2 = arm2[j - 1]
            if u1 == u2:
                matches += 1
                if memo is not None and (k1, k2) in memo:
                    score = memo[(k1, k2)]
                else:
                    _require(u1 < len(copy_numbers), "align_swg: copy_numbers[chunk] out of bounds")
                    score = sim(p1, p2, copy_numbers[u1], B, stats)
                    if memo is not None:
                        memo[(k1, k2)] = memo[(k2, k1)] = score
            else:
                score = B.num(MISM)
            mat = max(dp[i - 1][j - 1]) + score
            m, d2, d1 = dp[i][j - 1]
            del2 = max(m + GAP_OPEN, d2 + GAP_EXTEND, d1 + GAP_OPEN)
            m, d2, d1 = dp[i - 1][j]
            del1 = max(m + GAP_OPEN, d2 + GAP_OPEN, d1 + GAP_EXTEND)
            dp[i][j] = [mat, del2, del1]
    if stats is not None:
        if len1 == 0 or len2 == 0:
            _count(stats, "arm_pair_with_an_empty_arm")
            if len1 == 0 and len2 == 0:
                _count(stats, "arm_pair_both_empty")
        elif matches == 0:
            _count(stats, "arm_pair_without_common_chunk")
        stats["longest_arm1_vs_arm2"] = max(stats.get("longest_arm1_vs_arm2", (0, 0)), (len1 - len2, len1))
        stats["longest_arm2_vs_arm1"] = max(stats.get("longest_arm2_vs_arm1", (0, 0)), (len2 - len1, len2))
    best = max([max(c) for c in dp[len1]] + [max(row[len2]) for row in dp])
    return (best, dp) if want_table else best


def to_context(read, idx):
    """:243-261.  An arm entry is (chunk id, posterior, (read id, position)); returns (up, centre node, tail)."""
    center = read["nodes"][idx]
    ent = lambda q: (read["nodes"][q]["chunk"], read["nodes"][q]["posterior"], (read["id"], q))
    before = [ent(q) for q in range(idx - 1, -1, -1)]
    after = [ent(q) for q in range(idx + 1, len(read["nodes"]))]
    return (before, center, after) if center["is_forward"] else (after, center, before)


def alignment(ctx1, ctx2, copy_numbers, B=FloatMath, stats=None, memo=None):
    """:466-479"""
    up1, c1, down1 = ctx1
    up2, c2, down2 = ctx2
    _require(c1["chunk"] == c2["chunk"], "alignment: centres on different chunks")
    up = align_swg(up1, up2, copy_numbers, B, stats, memo)
    down = align_swg(down1, down2, copy_numbers, B, stats, memo)
    center = sim(c1["posterior"], c2["posterior"], copy_numbers[c1["chunk"]], B, stats)
    ratio = up + down + center
    return 1 / (1 + B.safe_exp(-ratio))


# ---------------------------------------------------------------------------------------------------------------------------
# phmm_likelihood_correction.rs, top down
# ---------------------------------------------------------------------------------------------------------------------------
def round_half_away(x):
    return math.copysign(math.floor(abs(x) + 0.5), x)


def estimate_copy_number_of_cluster(ds, decisions=None, stats=None, want_obs=False):
    """:131-181: vectors indexed by chunk id up to the largest id"""
    _require(len(ds["chunks"]) > 0, "no chunk: max().unwrap()")
    top = max(c["id"] for c in ds["chunks"])
    copy_num, cluster_num = [0] * (top + 1), [0] * (top + 1)
    for c in ds["chunks"]:
        copy_num[c["id"]], cluster_num[c["id"]] = c["copy_num"], c["cluster_num"]
    obs = [[0.0] * k for k in cluster_num]
    for read in ds["reads"]:
        for node in read["nodes"]:
            _require(node["chunk"] <= top, "obs_counts[chunk] out of bounds")
            total = logsumexp(node["posterior"])
            row = obs[node["chunk"]]
            for q in range(min(len(row), len(node["posterior"]))):  # zip truncates
                row[q] += math.exp(node["posterior"][q] - total)
    cov = ds["coverage"]
    out = []
    for cid, (row, total_cp) in enumerate(zip(obs, copy_num)):
        est = [max(round_half_away(o / cov), 1.0) for o in row]
        if decisions is not None:
            for o in row:
                decisions.append(("obs/cov vs .5", cid, abs(o / cov - (math.floor(o / cov) + 0.5))))
        rounded = int(round_half_away(sum(est)))
        if stats is not None and row and rounded > total_cp:
            _count(stats, "estimates_sum_above_copy_num")
        for _ in range(min(rounded, total_cp), total_cp):
            if not row:
                break
            gains = [(o - e * cov) ** 2 - (o - (e + 1.0) * cov) ** 2 for o, e in zip(row, est)]
            pick = max(range(len(gains)), key=lambda q: (gains[q], q))  # max_by: the last maximum
            if decisions is not None and len(gains) > 1:
                decisions.append(("now-next vs runner-up", cid, gains[pick] - max(g for q, g in enumerate(gains) if q != pick)))
            est[pick] += 1.0
            _count(stats, "increment_loop_iterations")
        out.append(est)
    return (out, obs) if want_obs else out


def filter_similarity(sims, pivot, decisions=None, cid=None):
    """:330-347 with select_nth :349-354"""
    SMALL, MIN_REQ = 0.0000000000000001, 0.51
    n = len(sims)
    keep = np.zeros((n, n), dtype=bool)
    for i in range(n):
        _require(pivot <= n, "select_nth: assert pivot <= len")
        _require(pivot < n, "select_nth: sims[pivot] out of bounds")
        threshold = max(float(np.sort(sims[i], kind="stable")[pivot]), MIN_REQ)
        hit = threshold <= sims[i]
        keep[i, hit] = True
        keep[hit, i] = True
        if decisions is not None:
            gap = np.abs(sims[i] - threshold)
            gap = gap[gap > 0.0]
            decisions.append(("similarity vs row threshold / 0.51", cid, float(gap.min()) if len(gap) else float("inf")))
    return np.where(keep, sims, SMALL)


def get_graph_laplacian(sims):
    """:385-402"""
    rowsum = sims.sum(axis=1)
    sq_inv = np.sqrt(1.0 / rowsum)
    lap = -sims * sq_inv[:, None] * sq_inv[None, :]
    np.fill_diagonal(lap, 1.0)
    return rowsum, lap


def eigh(a):
    return np.linalg.eigh(a)


EIGEN_THR = 0.2


def get_eigenvalues(lap, rowsum, eigen=eigh, decisions=None, cid=None):
    """:405-464: (features, pick_k, eigenvalues in the order used)"""
    _require(len(lap) > 0, "get_eigenvalues: no data")
    vals, vecs = eigen(lap)
    order = sorted(range(len(vals)), key=lambda q: abs(vals[q]))  # stable, by ABSOLUTE value
    lam = [float(vals[q]) for q in order]
    pick_k = 0
    while pick_k < len(lam) and lam[pick_k] < EIGEN_THR:  # take_while on the value itself
        pick_k += 1
    if decisions is not None:
        decisions.append(("eigenvalue vs 0.2", cid, min(abs(x - EIGEN_THR) for x in lam)))
        decisions.append(("spectral gap", cid, lam[pick_k] - lam[pick_k - 1] if 0 < pick_k < len(lam) else float("inf")))
    _require(pick_k > 0, "get_eigenvalues: pick_k == 0")
    feats = np.asarray(vecs)[:, order[:pick_k]] * np.sqrt(1.0 / rowsum)[:, None]
    return feats, pick_k, lam


def is_biased(node, thr):
    """Node::is_biased, definitions/src/lib.rs:703-709"""
    post = node["posterior"]
    if len(post) <= 1:
        return True
    return any(1.0 / len(post) + thr <= math.exp(x) for x in post)


def members_of(ds, chunk_id):
    """correct_chunk :191-199: every (read, position) on the chunk, stably sorted by the node's cluster"""
    mem = [(read, idx) for read in ds["reads"] for idx, node in enumerate(read["nodes"]) if node["chunk"] == chunk_id]
    mem.sort(key=lambda m: m[0]["nodes"][m[1]]["cluster"])
    return mem


def similarity_matrix(contexts, copy_numbers, stats=None, memo=None):
    n = len(contexts)
    sims = np.zeros((n, n))
    for i in range(n):
        for j in range(n):
            if i != j:
                sims[i, j] = alignment(contexts[i], contexts[j], copy_numbers, FloatMath, stats, memo)
    return sims


def correct_chunk(ds, chunk, copy_numbers, eigen=eigh, decisions=None, stats=None, memo=None):
    """correct_chunk :184-218 with clustering :263-328 and adj_rand_on_biased :220-240"""
    cid, k = chunk["id"], chunk["cluster_num"]
    mem = members_of(ds, cid)
    n = len(mem)
    if stats is not None:
        ids = [read["id"] for read, _ in mem]
        stats.setdefault("members_sharing_a_read", {})[cid] = n - len(set(ids))
        stats.setdefault("strands", {})[cid] = (sum(1 for r, i in mem if r["nodes"][i]["is_forward"]),
                                                 sum(1 for r, i in mem if not r["nodes"][i]["is_forward"]))
    contexts = [to_context(read, idx) for read, idx in mem]
    raw = similarity_matrix(contexts, copy_numbers, stats, memo)
    _require(chunk["copy_num"] != 0, "division by copy_num == 0")
    sims = filter_similarity(raw, n - n // chunk["copy_num"] // 4, decisions, cid)
    rowsum, lap = get_graph_laplacian(sims)
    feats, pick_k, lam = get_eigenvalues(lap, rowsum, eigen, decisions, cid)
    rows = []
    for f, (read, idx) in zip(feats, mem):  # append_posterior_probability :356-367
        post = read["nodes"][idx]["posterior"]
        total = logsumexp(post)
        rows.append(list(f) + [math.exp(x - total) for x in post])
    _require(all(len(r) == len(rows[0]) for r in rows), "feature rows of different length: kmeans' dist asserts")
    rows = np.array(rows)
    rows = rows / np.sqrt((rows * rows).sum(axis=0))[None, :]  # normalize_columns :369-381
    rng = Rand085(Xoroshiro128PlusPlus.seed_from_u64((cid * k) & M64))
    cluster_num = min(k, pick_k)
    runs = [kmeans(rows, cluster_num, rng) for _ in range(20)]
    best = min(range(20), key=lambda r: (runs[r][0], r))  # min_by: the first minimum
    asn = runs[best][1]
    if decisions is not None:
        others = [r[0] - runs[best][0] for r in runs if r[0] != runs[best][0]]
        decisions.append(("k-means residual: best vs next restart", cid, min(others) if others else float("inf")))
    _require(all(a <= cluster_num for a in asn), "assignment above cluster_num")
    prev = [read["nodes"][idx]["cluster"] for read, idx in mem]  # adj_rand_on_biased
    adjusted_rand_index(prev, asn)  # adj_raw: logged only, but it can panic
    biased = [(p, a) for (read, idx), p, a in zip(mem, prev, asn) if is_biased(read["nodes"][idx], 0.2)]
    _count(stats, "biased_members", len(biased))
    ari = adjusted_rand_index([b[0] for b in biased], [b[1] for b in biased])
    if math.isnan(ari):
        _count(stats, "ari_nan_on_biased")
        ari = 1.0
    return dict(id=cid, members=mem, asn=asn, k=cluster_num, pick_k=pick_k, ari=ari, raw_sims=raw, eigenvalues=lam, n=n)


ADJ_RAND_QUANTILE = 0.05


def supress_threshold(aris, stats=None):
    """:100-105"""
    ordered = sorted(aris)
    pick = math.ceil(len(ordered) * ADJ_RAND_QUANTILE)
    if stats is not None:
        stats["supress_pick"] = pick
    return ordered[pick] if pick < len(ordered) else 1.0


def protected_chunks(ds, min_gain, decisions=None):
    """get_protected_clusterings :108-129 with the minimum gain as an input"""
    coverage = {}
    for read in ds["reads"]:
        for node in read["nodes"]:
            coverage[node["chunk"]] = coverage.get(node["chunk"], 0) + 1
    out = set()
    for c in ds["chunks"]:
        if c["id"] not in coverage:
            continue
        k = float(c["cluster_num"])
        need = coverage[c["id"]] * ((k - 1.0) / k) * min_gain
        if decisions is not None and math.isfinite(need):
            decisions.append(("cov*frac*gain vs score", c["id"], abs(need - c["score"])))
        if need < c["score"]:
            out.add(c["id"])
    return out


def correct(ds, selection, min_gain, eigen=eigh):
    """AlignmentCorrection::correct_clustering_selected :31-97.  `ds` is not modified.  Returns a dict: status (0, or -6 with
    `panic` = the reason and nothing else changed), copy_numbers (by chunk id), per_chunk (id -> raw_sims, pick_k, k, ari,
    eigenvalues, n), cluster / touched / posterior per node in read order, cluster_num per chunk in `chunks` order, the
    decision log [(kind, chunk id, margin)] and the path counters."""
    decisions, stats, memo = [], {}, {}
    flat = [node for read in ds["reads"] for node in read["nodes"]]
    res = dict(status=0, panic=None, decisions=decisions, stats=stats, per_chunk={}, cluster=[n["cluster"] for n in flat],
               touched=[0] * len(flat), posterior=[list(n["posterior"]) for n in flat],
               cluster_num=[c["cluster_num"] for c in ds["chunks"]])
    selection = set(int(s) for s in selection)
    try:
        copy_numbers = estimate_copy_number_of_cluster(ds, decisions, stats)
        res["copy_numbers"] = copy_numbers
        done = [correct_chunk(ds, c, copy_numbers, eigen, decisions, stats, memo) for c in ds["chunks"]
                if 1 < c["cluster_num"] and c["id"] in selection]
        protected = protected_chunks(ds, min_gain, decisions)
        threshold = supress_threshold([d["ari"] for d in done], stats)
        res["supress_threshold"] = threshold
        new_k = {c["id"]: c["cluster_num"] for c in ds["chunks"]}
        copy_of = {c["id"]: c["copy_num"] for c in ds["chunks"]}
        on_read = {}
        for d in done:
            res["per_chunk"][d["id"]] = {q: d[q] for q in ("raw_sims", "pick_k", "k", "ari", "eigenvalues", "n")}
            decisions.append(("ARI vs suppression threshold", d["id"], abs(d["ari"] - threshold)))
            _require(d["k"] <= copy_of[d["id"]], "assert cluster_num <= copy_num")
            supress = d["k"] == 1 or d["ari"] < threshold
            if supress and d["id"] in protected:
                _count(stats, "protected")
                continue
            _count(stats, "supressed" if supress else "accepted")
            new_k[d["id"]] = 1 if supress else d["k"]
            for (read, idx), a in zip(d["members"], d["asn"]):
                on_read.setdefault(read["id"], []).append((idx, 0 if supress else a))
        # the write-back (:79-95) looks every read up BY ID, after every chunk's cluster_num is final
        out_post, out_cluster, out_touched = [], [], []
        for read in ds["reads"]:
            post = [list(n["posterior"]) for n in read["nodes"]]
            cl = [n["cluster"] for n in read["nodes"]]
            tc = [0] * len(cl)
            for idx, a in on_read.get(read["id"], []):
                cl[idx], tc[idx] = a, 1
                post[idx] = [-10000.0] * new_k[read["nodes"][idx]["chunk"]]
                _require(a < len(post[idx]), "posterior[asn] out of bounds")
                post[idx][a] = 0.0
            out_post += post
            out_cluster += cl
            out_touched += tc
        res.update(cluster=out_cluster, touched=out_touched, posterior=out_post,
                   cluster_num=[new_k[c["id"]] for c in ds["chunks"]])
    except ReferencePanic as exc:
        res.update(status=-6, panic=str(exc))
    except (ZeroDivisionError, FloatingPointError) as exc:
        res.update(status=-6, panic=repr(exc))
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# the DataSet-like structure <-> the flattened arrays of jtk_lc_correct_clustering / jo_correct_clustering
# ---------------------------------------------------------------------------------------------------------------------------
def flatten(ds):
    nodes, post, node_off = [], [], [0]
    for read in ds["reads"]:
        for n in read["nodes"]:
            nodes.append((n["chunk"], n["cluster"], 1 if n["is_forward"] else 0, len(n["posterior"]), len(post)))
            post.extend(n["posterior"])
        node_off.append(len(nodes))
    chunks = np.array([(c["id"], c["cluster_num"], c["copy_num"], c["score"]) for c in ds["chunks"]], dtype=CHUNK_DT)
    return dict(read_id=np.array([r["id"] for r in ds["reads"]], dtype=np.uint64), node_off=np.array(node_off, dtype=np.uint64),
                nodes=np.array(nodes, dtype=NODE_DT), posteriors=np.array(post + [0.0], dtype=np.float64)[:len(post)].copy(),
                chunks=chunks)


def unflatten(prob, coverage):
    post, off = prob["posteriors"], prob["node_off"]
    reads = []
    for r, rid in enumerate(prob["read_id"]):
        nodes = [dict(chunk=int(n["chunk"]), cluster=int(n["cluster"]), is_forward=bool(n["is_forward"]),
                      posterior=[float(x) for x in post[int(n["post_off"]):int(n["post_off"]) + int(n["post_len"])]])
                 for n in prob["nodes"][int(off[r]):int(off[r + 1])]]
        reads.append(dict(id=int(rid), nodes=nodes))
    chunks = [dict(id=int(c["id"]), cluster_num=int(c["cluster_num"]), copy_num=int(c["copy_num"]), score=float(c["score"]))
              for c in prob["chunks"]]
    return dict(reads=reads, chunks=chunks, coverage=float(coverage))


def written_back(ds, cluster, touched, cluster_num):
    """the DataSet after a call of the C entry points: their outputs (label and touched flag per node, cluster_num per chunk)
    applied as include/jtk_lc.h tells the caller to (:84-95)"""
    new_k = {c["id"]: int(k) for c, k in zip(ds["chunks"], cluster_num)}
    out = dict(reads=[], chunks=[dict(c, cluster_num=new_k[c["id"]]) for c in ds["chunks"]], coverage=ds["coverage"])
    e = 0
    for read in ds["reads"]:
        nodes = []
        for n in read["nodes"]:
            n = dict(n, posterior=list(n["posterior"]))
            if touched[e]:
                n["cluster"] = int(cluster[e])
                n["posterior"] = [-10000.0] * new_k[n["chunk"]]
                n["posterior"][n["cluster"]] = 0.0
            nodes.append(n)
            e += 1
        out["reads"].append(dict(id=read["id"], nodes=nodes))
    return out
