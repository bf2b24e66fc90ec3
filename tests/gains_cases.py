"""The cases on which the gains calibration is pinned to tests/gains_reference.py, and the fixture that carries the reference's
results to the tests (tests/golden/gains_reference/: <case>.json and the likelihoods in <case>.<k>.npy pieces;
tests/golden/make_gains_reference.py writes it).  tests/test_gains_reference.py (the oracle) and
tests/test_gpu_gains_reference.py (the device) share this file.  Each case is the smallest shape at which the named thing can go
wrong.

Models (forward and reverse differ in every one, so a strand mix-up shows):
  asym        test_phmm_reference.models()["asym"]: random rows, about 6 % Ins and 6 % Del out of Match
  deletions   the same emissions under transition rows that delete every second base: reads of 8- to 10-base templates come out
              with 0 and 1 bases
  noisy       a quarter of the steps an insertion and a quarter a deletion, from every state.  len12_band1 runs under it for the
              reference's sake: two reads that agree around the variant and differ some bases away score differences lk_diff -
              lk_base that differ only through the alignments that shift across the bases in between, a term of the order of (indel
              rate)^distance.  Under `asym` (6 %) that is 1e-7 .. 1e-10 at four to six bases, so that a median's nearest neighbour
              sat within 100 x the likelihood bound in 3 of 102 simulations looked at (smallest 2.6e-10 in the 600 of the case, 6.1e-8
              needed), and no seed passes 600 of them; at 25 % the term is 1e-3 .. 1e-4 and the smallest of 102 was 5.6e-5
  sparse      len = 200 with three bases in four deleted and near-uniform emissions: edit distances above 127
  insertions  four insertions per ten template bases, in runs: reads of a 200-base template pass 250 bases

estimate_gains (SAMPLE_NUM = 100 and SEQ_NUM = 50 are fixed: 20,000 pairs per profile):
  len6_asym        seq_len 6, homop_len 1, band 3: templates of 8 to 10 bases, every gen_diff_haplotypes branch at len = 1 (insert(1, ..)
                   appends)
  len6_deletions   the same shape under `deletions`: reads of length 0 and 1
  len12_band1      seq_len 12, homop_len 2, band 1, under `noisy`: the narrowest band, two homopolymer lengths, six profiles in one batch
estimate_minimum_gain (sample_num, seq_num, len, band):
  lower_bounds     (3, 1, 2, 1): medians[2] and lks[0] are the only choices
  second_stride    (3, 4, 66, 30): anti-diagonals of 65 and more cells (lane 0 of edit_ops_kernel takes a second cell), phmm_kernel's
                   widest band
  upper_bound      (3, 4, 200, 25): four strides per anti-diagonal, a W x W byte matrix above 48 KiB
  top_bit          (3, 4, 200, 25) under `sparse`: distances above 127 in edit_ops_kernel's bytes; the floor decides
  too_long         (3, 4, 200, 25) under `insertions`: the device answers JTK_ERR_UNSUPPORTED and leaves *out untouched (the reference
                   and the oracle have no such limit: the oracle is pinned on it like on the others)
  two_batches      (4, 12501, 2, 1): per = 50000 / 12501 = 3 samples per device batch, so batches of 3 and 1
"""
import json
import os

import numpy as np

import gains_reference as G
import phmm_reference as R
import test_phmm_reference as TP

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gains_reference")
SIM_KEYS = ("seqs", "ops", "dist", "distinct", "median", "null", "margin", "exact_margin", "scale")   # a case's "sims", by column
PIECE = 18000                   # doubles per <case>.<k>.npy: 144,128 bytes, below the largest file tests/golden held before
LK_RTOL = TP.LK_RTOL            # the bound test_phmm_reference.assert_table_matches applies to lk: |lk - ref| <= LK_RTOL |ref|
MARGIN_FACTOR = 100.0           # no decision of the reference within 100 x the bound of its threshold (gains_reference: `margin`)


def _with_rows(m, rows):
    return R.Model(rows, m.mat, m.ins)


def _flattened(m, diag):
    """emissions close to uniform: `diag` on the diagonal of mat_emit, the insertion rows pulled halfway to 1/4"""
    mat = np.where(np.eye(4) > 0, diag, (1.0 - diag) / 3.0)
    return R.Model(m.trans, mat, 0.5 * m.ins + 0.125)


def models():
    f, r = TP.models()["asym"]
    out = {"asym": (f, r)}
    out["deletions"] = (_with_rows(f, [[0.50, 0.05, 0.45], [0.55, 0.10, 0.35], [0.40, 0.05, 0.55]]),
                        _with_rows(r, [[0.46, 0.06, 0.48], [0.50, 0.12, 0.38], [0.42, 0.04, 0.54]]))
    out["noisy"] = (_with_rows(f, [[0.50, 0.25, 0.25], [0.55, 0.20, 0.25], [0.45, 0.25, 0.30]]),
                    _with_rows(r, [[0.52, 0.22, 0.26], [0.50, 0.24, 0.26], [0.48, 0.27, 0.25]]))
    out["sparse"] = (_with_rows(_flattened(f, 0.28), [[0.28, 0.02, 0.70], [0.30, 0.10, 0.60], [0.25, 0.02, 0.73]]),
                     _with_rows(_flattened(r, 0.31), [[0.26, 0.03, 0.71], [0.32, 0.08, 0.60], [0.24, 0.03, 0.73]]))
    out["insertions"] = (_with_rows(f, [[0.55, 0.40, 0.05], [0.45, 0.50, 0.05], [0.60, 0.35, 0.05]]),
                         _with_rows(r, [[0.57, 0.38, 0.05], [0.43, 0.52, 0.05], [0.58, 0.37, 0.05]]))
    return out


# name -> (model, seed, seq_len, band, homop_len)
GAINS_CASES = {
    "len6_asym": ("asym", 1201, 6, 3, 1),
    "len6_deletions": ("deletions", 77, 6, 3, 1),
    "len12_band1": ("noisy", 309423, 12, 1, 2),
}
# name -> (model, seed, sample_num, seq_num, len, band)
MIN_GAIN_CASES = {
    "lower_bounds": ("asym", 7, 3, 1, 2, 1),
    "second_stride": ("asym", 11, 3, 4, 66, 30),
    "upper_bound": ("asym", 23908, 3, 4, 200, 25),
    "top_bit": ("sparse", 5, 3, 4, 200, 25),
    "too_long": ("insertions", 3, 3, 4, 200, 25),
    "two_batches": ("asym", 41, 4, 12501, 2, 1),
}
MAX_DEVICE_LEN = 250            # jtk_lc_estimate_*'s limit on a simulated sequence (edit_ops_kernel keeps distances in a byte)
# what the CPU test recomputes of the cases too large to recompute whole: these simulations of every profile / these samples
RECOMPUTED_SIMS = (3, 98)
RECOMPUTED_SAMPLES = {"two_batches": (3,)}


def hmm_pair(name, Hmm):
    """the case's models as two jtk_hmm_t structures of the given binding (jtk_amd.ffi.Hmm or oracle_ffi.Hmm)"""
    f, r = models()[name]
    return f.fill(Hmm()), r.fill(Hmm())


# ---- one simulation <-> its fixture entry

def sim_entry(sim):
    """what the fixture keeps of a simulation, and its distinct likelihoods in order of first appearance"""
    which, n = G.distinct_of(sim)
    flat = [v for row in sim["lk"] for v in row]
    lk = [None] * n
    for w, v in zip(which, flat):
        if lk[w] is None:
            lk[w] = v
        assert lk[w] == v          # a pure function of (strand, template, read)
    e = dict(seqs=G.digest(sim["tmpls"] + sim["reads"]), ops=G.digest([o for row in sim["ops"] for o in row]),
             dist=G.digest([np.array([d for row in sim["dist"] for d in row], dtype="<u4").tobytes()]), distinct=n,
             median=sim["median"], margin=sim["margin"], exact_margin=sim["exact_margin"], scale=sim["scale"])
    if "null" in sim:
        e["null"] = sim["null"]
    return e, lk


def gains_sims(name, pick=None):
    """the simulations of a gains case as (profile index, i, simulation); `pick` limits i"""
    model, seed, seq_len, band, homop_len = GAINS_CASES[name]
    f, r = models()[model]
    for q, (ty, length) in enumerate(G.profiles(homop_len)):
        for i in (range(G.SAMPLE_NUM) if pick is None else pick):
            yield q, i, G.gain_simulation(f, r, seed, seq_len, band, length, ty, i)


def min_gain_sample(name, s):
    model, seed, sample_num, seq_num, length, band = MIN_GAIN_CASES[name]
    f, r = models()[model]
    return G.minimum_gain_sample(f, r, seed, seq_num, length, band, s)


# ---- the fixture

def case_path(name):
    return os.path.join(GOLDEN_DIR, name + ".json")


def dump_case(name, case):
    """a case's entry as <case>.json, its simulations' entries column by column"""
    case = dict(case)
    case["sims"] = {key: [e.get(key) for e in case["sims"]] for key in SIM_KEYS}
    with open(case_path(name), "w") as f:
        json.dump(case, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")


def load_index():
    """name -> the case's entry, "sims" a list of one dict per simulation in batch order"""
    out = {}
    for name in list(GAINS_CASES) + list(MIN_GAIN_CASES):
        case = json.load(open(case_path(name)))
        cols = case["sims"]
        case["sims"] = [{key: cols[key][k] for key in SIM_KEYS if cols[key][k] is not None} for k in range(len(cols["seqs"]))]
        out[name] = case
    return out


def load_lk(name, index=None):
    """the case's distinct likelihoods, simulation after simulation"""
    index = index or load_index()
    return np.concatenate([np.load(os.path.join(GOLDEN_DIR, "%s.%d.npy" % (name, k))) for k in range(index[name]["pieces"])])


def sim_slices(case):
    """[(entry, offset of its distinct likelihoods)] of a case's simulations in batch order"""
    out, at = [], 0
    for e in case["sims"]:
        out.append((e, at))
        at += e["distinct"]
    return out


def bound_of(scale):
    return LK_RTOL * scale
