"""An independent restatement of the gains calibration, in plain Python (test infrastructure).

Written from haplotyper/src/likelihood_gains.rs alone (estimate_minimum_gain :6-39, estimate_gain :162-184, sample_triple and
gen_diff_haplotypes :213-251, gain_of :253-315) and, for the three calls into the un-vendored kiley crate, from the prose of this
project's own specification:

  generate_seq(rng, n)            n times BASES.choose(rng): one gen_index(4) per base
  Generate::gen(tmpl, rng)        start in Match at template position 0; draw the next state from the current state's transition
                                  row (choose_weighted over [-> Match, -> Ins, -> Del]); Match emits from mat_emit[x[i]] and advances,
                                  Ins emits from ins_emit[previous read base, 4 before the first], Del advances; stop at the
                                  template's end
  introduce_errors(s, rng, 0, 1, 0)   [Match x (len - 1), Del] under SliceRandom::shuffle (for i in (1..len).rev():
                                  swap(i, gen_index(i + 1))); the base where the Del lands is dropped
  likelihood_antidiagonal_bootstrap(tmpl, read, band)   align_reference.align, then phmm_reference.likelihood in that band

It shares no code with jtk_amd/csrc/gains.hip, oracle/likelihood_gains.c or oracle/phmm.c, none of which was followed while this
was written: the shuffle is a shuffle of a list, the reads of a simulation are drawn before anything is scored, the order statistics
are sorted(xs)[k].  The generator is clustering_reference.Xoshiro256StarStar under correction_reference.Rand085 (gen_index,
choose_weighted), both pinned by their own tests.  Parity with the real kiley stays unpinned.

Everything in between is returned, in the order the device batches it (one batch for estimate_gain: profile, simulation, then the
simulation's template with its 100 reads and its variant with the same 100 reads; for estimate_minimum_gain batches of
max(1, 50000 / seq_num) samples, each sample hap1 with its reads and hap2 with the same reads): see `batches_of`.

`margin`: every simulation records the smallest distance of any of its decisions from its threshold -- a null-count comparison
lk_base + min_gain < lk_diff, which difference is the median, which median is the final number, whether the floor decides -- next
to `scale`, the largest |log likelihood| it saw; bit-equal operands (the same read drawn twice gives the same difference twice;
null counts are integers) are exact ties that no rounding separates and are not counted.  `exact_margin` is the same over the
decisions whose OUTCOME a test compares exactly: the null-count comparisons and the floor.  (Which read supplies a median is not
one of them: an order statistic moves by no more than its inputs do, whichever element ends up in its place, and medians and
gains are compared within a bound.  Reads that agree around the variant and differ far from it give differences that agree to
1e-7 .. 1e-10 without being equal, so on templates of a dozen bases and more a median's nearest neighbour is often that close.)
"""
import hashlib

import numpy as np

import align_reference as A
import phmm_reference as R
from clustering_reference import Xoshiro256StarStar
from correction_reference import M64, Rand085, _require

SUBST, DEL, INS = 0, 1, 2                       # likelihood_gains.rs:194-199
SAMPLE_NUM, SEQ_NUM = 100, 50                   # gain_of :261-264
GAIN_POS, PROB_POS = SAMPLE_NUM // 10, SAMPLE_NUM * 2 // 3
MIN_REQ = 1.0                                   # estimate_minimum_gain :12
BASES = b"ACGT"
INF = float("inf")


def rng_of(seed):
    return Rand085(Xoshiro256StarStar.seed_from_u64(seed & M64))


def _arr(s):
    return np.frombuffer(bytes(s), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------------------
# the three kiley calls, from DESIGN section 4
# ---------------------------------------------------------------------------------------------------------------------------
def generate_seq(rng, n):
    return bytes(BASES[rng.choose(4)] for _ in range(n))


def gen_read(model, tmpl, rng):
    """Generate::gen of one strand's model (a phmm_reference.Model)"""
    rows, mat, ins = model.trans.tolist(), model.mat.tolist(), model.ins.tolist()
    x = R.codes(_arr(tmpl)).tolist()
    i, state, prev, out = 0, 0, 4, bytearray()
    while i < len(x):
        state = rng.choose_weighted(rows[state])
        _require(state is not None, "gen: a transition row without weight")
        if state == 2:
            i += 1
            continue
        b = rng.choose_weighted(mat[x[i]] if state == 0 else ins[prev])
        _require(b is not None, "gen: an emission row without weight")
        out.append(BASES[b])
        prev = b
        if state == 0:
            i += 1
    return bytes(out)


def introduce_one_deletion(seq, rng):
    ops = ["M"] * (len(seq) - 1) + ["D"]
    for i in range(len(ops) - 1, 0, -1):
        j = rng.gen_index(i + 1)
        ops[i], ops[j] = ops[j], ops[i]
    at = ops.index("D")
    return seq[:at] + seq[at + 1:]


class Scorer:
    """likelihood_antidiagonal_bootstrap under the model of a read's strand; a pure function of (strand, template, read), so equal
    arguments are scored once"""

    def __init__(self, forward, reverse, band):
        self.models, self.band, self.seen = (forward, reverse), band, {}

    def __call__(self, t, tmpl, read):
        """-> (ops, distance, log likelihood) of read number t of its simulation (even t: forward)"""
        key = (t % 2, tmpl, read)
        if key not in self.seen:
            x, y = _arr(tmpl), _arr(read)
            ops, dist = A.align(x, y)
            self.seen[key] = (ops.tobytes(), dist, R.likelihood(self.models[t % 2], x, y, ops, self.band))
        return self.seen[key]


# ---------------------------------------------------------------------------------------------------------------------------
# likelihood_gains.rs
# ---------------------------------------------------------------------------------------------------------------------------
def sample_triple(rng):
    homop = BASES[rng.choose(4)]
    right = BASES[rng.choose_weighted([1.0 if b != homop else 0.0 for b in BASES])]
    left = BASES[rng.choose_weighted([1.0 if b != homop and b != right else 0.0 for b in BASES])]
    return right, homop, left


def gen_diff_haplotypes(rng, length, diff_type):
    right, center, left = sample_triple(rng)
    center1 = [center] * length
    center2 = list(center1)
    if diff_type == SUBST:
        center2[0] = BASES[rng.choose_weighted([1.0 if b != center else 0.0 for b in BASES])]
    elif diff_type == DEL:
        del center2[0]
    else:
        diff = BASES[rng.choose_weighted([1.0 if b != center else 0.0 for b in BASES])]
        _require(1 <= len(center2), "Vec::insert(1, ..) past the end")
        center2.insert(1, diff)
    return bytes([right] + center1 + [left]), bytes([right] + center2 + [left])


def nth(xs, k):
    """select_nth_unstable_by(k).1: the k-th smallest"""
    return sorted(xs)[k]


def _gap(xs, k):
    """distance of the k-th smallest from its nearest neighbour in order that is not bit-equal to it"""
    s = sorted(xs)
    return min([abs(v - s[k]) for v in s if v != s[k]], default=INF)


def gain_decisions(diff_type, lk_base, lk_diff):
    """gain_of :275-306 on one simulation's 2 x (2 SEQ_NUM) likelihoods (reads 0 .. SEQ_NUM - 1 drawn from the variant, the rest
    from the template) -> (median, null count, margin)"""
    d = [lk_diff[t] - lk_base[t] for t in range(SEQ_NUM)]
    expected_gain = nth(d, SEQ_NUM // 2)
    min_gain = expected_gain / 10.0 if diff_type == SUBST else 0.0001
    null, exact = 0, INF
    for t in range(SEQ_NUM, 2 * SEQ_NUM):
        null += 1 if lk_base[t] + min_gain < lk_diff[t] else 0
        exact = min(exact, abs(lk_diff[t] - (lk_base[t] + min_gain)))
    return expected_gain, null, min(exact, _gap(d, SEQ_NUM // 2)), exact


def profile_of(medians, nulls):
    """gain_of :309-314 -> (gain, prob)"""
    return nth(medians, GAIN_POS), max(nth([c / SEQ_NUM for c in nulls], PROB_POS), 0.000000001)


def gain_simulation(forward, reverse, seed, seq_len, band, length, diff_type, i):
    """simulation i of gain_of: its sequences, every pair's ops, distance and likelihood, its median and null count"""
    rng = rng_of(i + seed)
    seg1 = generate_seq(rng, seq_len // 2)
    seg2 = generate_seq(rng, seq_len // 2)
    hap1, hap2 = gen_diff_haplotypes(rng, length, diff_type)
    template, diff = seg1 + hap1 + seg2, seg1 + hap2 + seg2
    models = (forward, reverse)
    reads = [gen_read(models[t % 2], diff, rng) for t in range(SEQ_NUM)]
    reads += [gen_read(models[t % 2], template, rng) for t in range(SEQ_NUM)]
    score = Scorer(forward, reverse, band)
    rows = [[score(t, tmpl, r) for t, r in enumerate(reads)] for tmpl in (template, diff)]
    lk = [[c[2] for c in row] for row in rows]
    median, null, margin, exact = gain_decisions(diff_type, lk[0], lk[1])
    return dict(tmpls=[template, diff], reads=reads, ops=[[c[0] for c in row] for row in rows],
                dist=[[c[1] for c in row] for row in rows], lk=lk, median=median, null=null, margin=margin, exact_margin=exact,
                scale=max(abs(v) for row in lk for v in row))


def profiles(homop_len):
    """estimate_gain :169-177: the (type, homopolymer length) profiles in the order they are computed"""
    return [(ty, length) for ty in (SUBST, DEL, INS) for length in range(1, homop_len + 1)]


def estimate_gain(forward, reverse, seed, seq_len, band, homop_len, sims=None):
    """-> dict(profiles = [(type, length)], sims = [profile][SAMPLE_NUM], gain, prob = [profile]); `sims` takes simulations
    computed elsewhere (tests/golden/make_gains_reference.py spreads them over processes)"""
    prof = profiles(homop_len)
    if sims is None:
        sims = [[gain_simulation(forward, reverse, seed, seq_len, band, length, ty, i) for i in range(SAMPLE_NUM)]
                for ty, length in prof]
    fin = [profile_of([s["median"] for s in ss], [s["null"] for s in ss]) for ss in sims]
    # which of the medians is the gain counts too (the null counts are integers: their ties are exact)
    margin = min(min([_gap([s["median"] for s in ss], GAIN_POS)] + [s["margin"] for s in ss]) for ss in sims)
    return dict(profiles=prof, sims=sims, gain=[g for g, _ in fin], prob=[p for _, p in fin], margin=margin,
                exact_margin=min(s["exact_margin"] for ss in sims for s in ss))


def minimum_gain_sample(forward, reverse, seed, seq_num, length, band, s):
    """sample s of estimate_minimum_gain :15-33"""
    rng = rng_of(seed + s)
    hap1 = generate_seq(rng, length)
    hap2 = introduce_one_deletion(hap1, rng)
    models = (forward, reverse)
    reads = [gen_read(models[t % 2], hap1, rng) for t in range(seq_num)]
    score = Scorer(forward, reverse, band)
    rows = [[score(t, tmpl, r) for t, r in enumerate(reads)] for tmpl in (hap1, hap2)]
    lk = [[c[2] for c in row] for row in rows]
    d = [lk[0][t] - lk[1][t] for t in range(seq_num)]
    return dict(tmpls=[hap1, hap2], reads=reads, ops=[[c[0] for c in row] for row in rows],
                dist=[[c[1] for c in row] for row in rows], lk=lk, median=nth(d, seq_num // 2), margin=_gap(d, seq_num // 2),
                exact_margin=INF,
                scale=max(abs(v) for row in lk for v in row))


def minimum_gain_of(medians):
    """:36-38 -> (the minimum gain, the distance of its two decisions from their thresholds, that of the floor alone)"""
    third = sorted(medians)[2]
    return max(third, MIN_REQ), min(_gap(medians, 2), abs(third - MIN_REQ)), abs(third - MIN_REQ)


def estimate_minimum_gain(forward, reverse, seed, sample_num, seq_num, length, band, sims=None):
    _require(sample_num >= 3 and seq_num >= 1 and length >= 1, "medians[2] / lks[SEQ_NUM / 2] / the shuffle out of bounds")
    if sims is None:
        sims = [minimum_gain_sample(forward, reverse, seed, seq_num, length, band, s) for s in range(sample_num)]
    value, margin, exact = minimum_gain_of([s["median"] for s in sims])
    return dict(sims=sims, min_gain=value, margin=min([margin] + [s["margin"] for s in sims]), exact_margin=exact)


# ---------------------------------------------------------------------------------------------------------------------------
# the order the device batches it, and what a fixture keeps of it
# ---------------------------------------------------------------------------------------------------------------------------
def batch_sizes(sample_num, seq_num):
    """estimate_minimum_gain's samples per likelihood batch (jtk_lc_estimate_minimum_gain keeps a batch near 100,000 pairs)"""
    per = max(1, 50000 // seq_num)
    return [min(per, sample_num - s0) for s0 in range(0, sample_num, per)]


def batches_of(sims, sizes=None):
    """simulations (a flat list, profiles one after the other) -> batches; a batch lists its templates, and per pair (template
    after template, each with all the reads of its simulation) the read, the strand flag (1 forward), ops, distance, likelihood"""
    out, at = [], 0
    for size in sizes or [len(sims)]:
        b = dict(tmpls=[], reads=[], strand=[], ops=[], dist=[], lk=[])
        for s in sims[at:at + size]:
            for k, tmpl in enumerate(s["tmpls"]):
                b["tmpls"].append(tmpl)
                b["reads"] += s["reads"]
                b["strand"] += [1 - t % 2 for t in range(len(s["reads"]))]
                b["ops"] += s["ops"][k]
                b["dist"] += s["dist"][k]
                b["lk"] += s["lk"][k]
        out.append(b)
        at += size
    return out


def digest(seqs):
    """of a list of byte strings, their lengths and then their bytes: the first 64 bits of the SHA-256"""
    h = hashlib.sha256(np.array([len(s) for s in seqs], dtype="<u8").tobytes())
    h.update(b"".join(bytes(s) for s in seqs))
    return h.hexdigest()[:16]


def distance_of(ops):
    return sum(1 for op in bytes(ops) if op != R.OP_MATCH)


def distinct_of(sim):
    """per pair of one simulation (template after template, each with all the reads): its index among the simulation's distinct
    (strand, template, read) by first appearance -- what a fixture stores one likelihood for -- and the number of them"""
    index, which = {}, []
    for tmpl in sim["tmpls"]:
        for t, read in enumerate(sim["reads"]):
            which.append(index.setdefault((t % 2, bytes(tmpl), bytes(read)), len(index)))
    return which, len(index)
