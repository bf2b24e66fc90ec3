"""oracle/correction.c against tests/correction_reference.py, the independent Python restatement of
phmm_likelihood_correction.rs (CPU only).  The problems are tests/correction_cases.py; every case asserts, on the reference's own
counters, that it entered the path it is named for (`entered`, listed beside each case there).

By value: every corrected chunk's raw similarity matrix (the oracle returns the first corrected chunk's, and its copy numbers
come from all chunks whatever the selection, so one call per chunk with selection=[id] yields every matrix).  By outcome: the
adjusted Rand index of every chunk, labels, cluster_num, touched flags, the rewritten posteriors and the panic status.  The
oracle does not return its copy-number table, pick_k or k: the table is pinned through the similarities (every value contains
-ln cp of its chunk; test_copy_number_observations compares the observations it is rounded from, evaluated with the oracle's own
exp / log) and pick_k / k through cluster_num and the labels.

  * with the oracle's eigen-basis injected (jo_symmetric_eigen) labels are compared as arrays, on every case;
  * with numpy.linalg.eigh the adjusted Rand indices and cluster_num must be equal and labels are compared as partitions, on
    the cases whose decision log shows a spectral gap (EIGH_CASES: every eigenvalue the clustering uses is separated from the
    next one by more than 0.05; the cases left out have chunks with several near-zero eigenvalues, where LAPACK and Jacobi may
    return different bases of one eigenspace and normalize_columns is not rotation-invariant).

Measured numbers (this module prints them: pytest -s -k measured):
    REF_VS_MPMATH     1.5e-15   largest |reference - mpmath at 50 digits| over the similarities (test_reference_against_mpmath)
    ORACLE_VS_REF     1.5e-15   largest |oracle - reference| over all similarity values of all cases, 3.6e-15 over the
                                copy-number observations (sums of up to 100 probabilities)
    TOLERANCE         2.4e-14   8 * (REF_VS_MPMATH + ORACLE_VS_REF), absolute, on similarities
    TIE_MARGIN        3.6e-12   1e3 * the larger oracle-reference difference (the observations')
A case is valid only if no entry of the reference's decision log is within TIE_MARGIN of a tie (test_reference_is_tie_free; no
case is excluded).  Entries that are EXACTLY equal are not ties in this sense: two similarities that are equal to the last bit come
from equal operands or from the saturation of 1 / (1 + exp(-x)), which the 1-ulp difference between libm and the shared fdlibm
cannot separate; adjusted Rand indices are ratios of integers.

Conditioning near certainty.  For lnp within about 1e-9 of 0 (two nodes that agree with posteriors within 1e-9 of certainty, short
of the UPPER_THR saturation) lnp - ln_1p(-exp(lnp)) is ill-conditioned in ANY double evaluation, the Rust's included: lnp itself
carries an absolute error of 1e-16, i.e. 1e-7 relatively on 1 - p.  The oracle's and the kernel's log(1 + x) for ln_1p is within
that.  The cases keep every soft posterior <= -1e-6 (hard ones saturate), where the bounds above hold.

Seeded faults, one at a time in an uncommitted copy of oracle/correction.c; the tests of this module that then fail (sim =
test_similarities, basis = test_outcomes_with_the_oracles_basis, lapack = test_outcomes_with_lapack; case names shortened):
    arms not swapped for reverse nodes        30: sim on 15 cases (one_node_reads_mixed, sparse, tandem, unequal, hard, ...), basis on
                                              12, lapack on 2, test_two_passes.  Not one_node_reads_reverse: with EVERY member
                                              reverse the unswapped arms are swapped on both sides and up + down is unchanged.
    GAP_EXTEND charged on the first gap       29: sim on 16 cases, basis on 11, lapack on 2.  Not sim[arms_matching_after_gaps]:
                                              80 per hard node saturates 1 / (1 + exp(-x)) with either charge; the gaps of 2 and
                                              3 nodes are pinned by value on the reference only (test_gap_scores), the oracle's
                                              charge through the one-node gaps of the soft cases.
    sim with + ln cp                          34: sim on 15 cases, basis on 15, lapack on 3, test_two_passes
    UPPER_THR / LOWER_CUT exchanged           35: sim on 17 cases, basis on 15, lapack on 2, test_two_passes
    select_nth pivot off by one                6: basis[cluster_nums_14, min_gain_*, suppression, tandem, unequal]
    threshold < x for <=                      12: basis[gaps, hard, cluster_nums_9/14, min_gain_*, mixed, stray_alone, suppression,
                                              tandem, unequal], test_two_passes
    eigenvalues sorted by value, not |value|   0: not visible, see below
    min_by taking the last minimum            14: basis on 13 cases, test_two_passes
    ARI over all reads, not the biased ones   15: basis on 13 cases, lapack on 2
    floor for ceil in supress_threshold       10: basis on 10 cases
    write-back with the OLD cluster_num        -: cannot be seeded in the oracle, which returns labels and cluster_num and leaves
                                              the posteriors to the caller; R.written_back applies them with the NEW cluster_num
                                              and test_two_passes compares that with the reference's own write-back, node by node
  Not visible: "eigenvalues sorted by value".  The normalised Laplacian of a similarity graph has its eigenvalues in [0, 2]; a
  negative one is rounding noise of about 1e-16, whose absolute value sorts into the same near-zero group, so both orders pick
  the same eigenvectors, at most in another order, which permutes feature columns and changes no distance.

Run time: 12 s.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import correction_cases as K
import correction_reference as R
import oracle_ffi as O
from helpers import same_partition

REF_VS_MPMATH = R.REF_VS_MPMATH
ORACLE_VS_REF = 1.5e-15
ORACLE_VS_REF_OBS = 3.6e-15
TOLERANCE = 8 * (REF_VS_MPMATH + ORACLE_VS_REF)
TIE_MARGIN = 1e3 * max(ORACLE_VS_REF, ORACLE_VS_REF_OBS)

NAMES = list(K.CASES)
EIGH_GAP = 0.05


def jacobi(a):
    """the oracle's eigen-solver (include/jtk_eigen.h through jo_symmetric_eigen): eigenvalues in its own order, vectors"""
    n = len(a)
    work, v = np.array(a, dtype=np.float64, order="C"), np.zeros((n, n))
    f = O.lib().jo_symmetric_eigen
    f.argtypes, f.restype = [C.POINTER(C.c_double), C.c_size_t, C.POINTER(C.c_double)], None
    f(O.f64p(work), n, O.f64p(v))
    return np.diag(work).copy(), v


def oracle_run(ds, selection, min_gain, want_sims=0):
    prob = R.flatten(ds)
    chunks = prob["chunks"].copy()
    rc, cluster, touched, ari, sims = O.correct_clustering(prob["read_id"], prob["node_off"], prob["nodes"], prob["posteriors"], chunks,
                                                           np.asarray(selection, dtype=np.uint64), ds["coverage"], min_gain, want_sims)
    return dict(rc=rc, cluster=cluster, touched=touched, ari=ari, sims=sims, chunks=chunks)


def oracle_sims(ds, cid, n):
    """the oracle's raw similarity matrix of one chunk: it is the first (only) corrected chunk of a call with selection=[id]"""
    return oracle_run(ds, [cid], 1e9, want_sims=n)["sims"]


@functools.lru_cache(maxsize=None)
def made(name):
    return K.CASES[name]()


@functools.lru_cache(maxsize=None)
def reference(name, solver="jacobi"):
    m = made(name)
    return R.correct(m["ds"], m["selection"], m["min_gain"], eigen=jacobi if solver == "jacobi" else R.eigh)


@functools.lru_cache(maxsize=None)
def oracle(name):
    m = made(name)
    return oracle_run(m["ds"], m["selection"], m["min_gain"])


def compare_outcomes(ref, ora, ds, exact_labels):
    assert ora["rc"] == ref["status"]
    if ref["status"] != 0:
        assert not ora["touched"].any()
        return
    assert ora["chunks"]["cluster_num"].tolist() == ref["cluster_num"]
    assert ora["touched"].tolist() == ref["touched"]
    for i, c in enumerate(ds["chunks"]):
        if c["id"] in ref["per_chunk"]:
            assert ora["ari"][i] == ref["per_chunk"][c["id"]]["ari"], c["id"]
        else:
            assert math.isnan(ora["ari"][i])
    if exact_labels:
        assert ora["cluster"].tolist() == ref["cluster"]
    else:
        chunk_of = np.array([n["chunk"] for r in ds["reads"] for n in r["nodes"]])
        for cid in ref["per_chunk"]:
            m = chunk_of == cid
            assert same_partition(ora["cluster"][m], np.array(ref["cluster"])[m]), cid
    # the rewritten posteriors: the oracle's outputs applied as the header tells the caller to, against the reference's own write-back
    back = R.written_back(ds, ora["cluster"], ora["touched"], ora["chunks"]["cluster_num"])
    if exact_labels:
        assert [n["posterior"] for r in back["reads"] for n in r["nodes"]] == ref["posterior"]
    assert [len(n["posterior"]) for r in back["reads"] for n in r["nodes"]] == [len(p) for p in ref["posterior"]]


@pytest.mark.parametrize("name", NAMES)
def test_case_enters_its_path(name):
    made(name)["entered"](reference(name))
    assert reference(name)["status"] == made(name)["status"]


@pytest.mark.parametrize("name", NAMES)
def test_reference_is_tie_free(name):
    """no comparison that decides an outcome is within TIE_MARGIN of a tie, on the reference alone (no case is excluded)"""
    near = [d for d in reference(name)["decisions"] if d[0] != "spectral gap" and 0.0 < d[2] < TIE_MARGIN]
    assert not near, near[:5]


@pytest.mark.parametrize("name", NAMES)
def test_similarities(name):
    """every corrected chunk's raw similarity matrix, oracle against reference, within TOLERANCE (absolute)"""
    ref, ds = reference(name), made(name)["ds"]
    worst = 0.0
    for cid, pc in ref["per_chunk"].items():
        got = oracle_sims(ds, cid, pc["n"])
        worst = max(worst, float(np.abs(got - pc["raw_sims"]).max()))
    print("measured |oracle - reference| on similarities, %s: %.3g" % (name, worst))
    assert worst <= 1e-9, "a finding, not a tolerance"
    assert worst <= TOLERANCE


@pytest.mark.parametrize("name", NAMES)
def test_outcomes_with_the_oracles_basis(name):
    compare_outcomes(reference(name), oracle(name), made(name)["ds"], exact_labels=True)


def has_spectral_gap(ref):
    """every eigenvalue the clustering uses is more than EIGH_GAP away from the next one (the first unused one included)"""
    if ref["status"] != 0:
        return False
    for pc in ref["per_chunk"].values():
        lam = pc["eigenvalues"][:pc["pick_k"] + 1]
        if len(lam) > 1 and min(b - a for a, b in zip(lam, lam[1:])) <= EIGH_GAP:
            return False
    return True


EIGH_CASES = ["linked_haplotypes_a", "linked_haplotypes_b", "cluster_nums_coverage_6"]


@pytest.mark.parametrize("name", EIGH_CASES)
def test_outcomes_with_lapack(name):
    """the fully independent leg: numpy.linalg.eigh in the reference, on the cases with a spectral gap"""
    ref = reference(name, "eigh")
    assert has_spectral_gap(ref), [d for d in ref["decisions"] if d[0] == "spectral gap"]
    compare_outcomes(ref, oracle(name), made(name)["ds"], exact_labels=False)


def test_status_of_the_panic_cases():
    panics = [n for n in NAMES if made(n)["status"] == -6]
    assert len(panics) >= 5
    for n in panics:
        assert reference(n)["status"] == -6 and oracle(n)["rc"] == -6, n


def test_two_passes():
    """the correction fed its own output (JTK calls this stage repeatedly): the second pass runs on the -10000 / 0 posteriors and
    the NEW cluster_num of the first, through both saturations of logit_from_lnp"""
    m = made("hard_posteriors")
    first_ref, first_ora = reference("hard_posteriors"), oracle("hard_posteriors")
    compare_outcomes(first_ref, first_ora, m["ds"], exact_labels=True)
    ds2 = K.two_pass_input(first_ref, m)
    back = R.written_back(m["ds"], first_ora["cluster"], first_ora["touched"], first_ora["chunks"]["cluster_num"])
    assert back["reads"] == ds2["reads"] and back["chunks"] == ds2["chunks"]
    # the write-back used the NEW cluster_num: a suppressed chunk's nodes carry one posterior
    for c in ds2["chunks"]:
        for r in ds2["reads"]:
            for n in r["nodes"]:
                if n["chunk"] == c["id"]:
                    assert len(n["posterior"]) == c["cluster_num"]
    sel = [c["id"] for c in ds2["chunks"]]
    ref2 = R.correct(ds2, sel, 1e9, eigen=jacobi)
    assert ref2["status"] == 0 and ref2["stats"]["upper_cut"] > 0 and ref2["stats"]["lower_cut"] > 0
    assert not [d for d in ref2["decisions"] if d[0] != "spectral gap" and 0.0 < d[2] < TIE_MARGIN]
    for cid, pc in ref2["per_chunk"].items():
        assert np.abs(oracle_sims(ds2, cid, pc["n"]) - pc["raw_sims"]).max() <= TOLERANCE
    compare_outcomes(ref2, oracle_run(ds2, sel, 1e9), ds2, exact_labels=True)


def test_gap_scores():
    """GAP_OPEN once, then GAP_EXTEND: a read that lacks the g nodes next to chunk 50 against one that has them aligns as
    -0.5 - 100 (g - 1) + 80 per node behind the gap (hard posteriors of one haplotype: sim == UPPER_CUT), worked out by hand"""
    ds = made("arms_matching_after_gaps")["ds"]
    cn = R.estimate_copy_number_of_cluster(ds)
    full = next(r for r in ds["reads"] if len(r["nodes"]) == 9 and r["nodes"][0]["is_forward"])
    hap = full["nodes"][1]["cluster"]
    for g in (1, 2, 3):
        short = next(r for r in ds["reads"] if len(r["nodes"]) == 9 - g and r["nodes"][0]["is_forward"] and r["nodes"][1]["cluster"] == hap)
        a, b = R.to_context(full, 0)[2], R.to_context(short, 0)[2]
        assert len(a) == 8 and len(b) == 8 - g and a[g][0] == b[0][0]
        want = R.GAP_OPEN + (g - 1) * R.GAP_EXTEND + 80.0 * (8 - g)
        assert R.align_swg(a, b, cn) == want and R.align_swg(b, a, cn) == want, g
    # and the oracle agrees on the matrix these arms are in (test_similarities[arms_matching_after_gaps])


def test_copy_number_observations():
    """the observations the copy-number table is rounded from, summed with the ORACLE's exp / logsumexp in the same node order,
    against the reference's: their largest difference is the second input of TIE_MARGIN"""
    L = O.lib()
    worst = 0.0
    for name in NAMES:
        ds = made(name)["ds"]
        try:
            _, obs = R.estimate_copy_number_of_cluster(ds, want_obs=True)
        except R.ReferencePanic:
            continue
        mine = [[0.0] * len(row) for row in obs]
        for r in ds["reads"]:
            for n in r["nodes"]:
                p = np.array(n["posterior"])
                total = L.jo_logsumexp(O.f64p(p), len(p))
                for q in range(min(len(p), len(mine[n["chunk"]]))):
                    mine[n["chunk"]][q] += L.jo_exp(float(p[q]) - total)
        for a, b in zip(obs, mine):
            for x, y in zip(a, b):
                worst = max(worst, abs(x - y))
    print("measured |oracle - reference| on copy-number observations: %.3g" % worst)
    assert worst <= ORACLE_VS_REF_OBS


def test_reference_against_mpmath():
    """the reference's own error: sim and alignment in mpmath at 50 digits on pairs drawn from the test problems"""
    B = R.MpMath(50)
    rng = np.random.default_rng(5)
    worst_sim = worst_aln = 0.0
    pairs = 0
    for name in ("sparse_unordered_ids", "hard_posteriors", "single_cluster_neighbours", "cluster_nums_coverage_9", "arms_matching_after_gaps",
                 "unequal_and_disjoint_arms"):
        m = made(name)
        ds = m["ds"]
        cn = R.estimate_copy_number_of_cluster(ds)
        for cid in list(reference(name)["per_chunk"])[:3]:
            mem = R.members_of(ds, cid)
            ctx = [R.to_context(r, i) for r, i in mem]
            for _ in range(22):
                i, j = rng.choice(len(ctx), 2, replace=False)
                f = R.alignment(ctx[i], ctx[j], cn)
                g = R.alignment(ctx[i], ctx[j], cn, B)
                worst_aln = max(worst_aln, abs(float(B.num(f) - g)))
                x, y = ctx[i][1]["posterior"], ctx[j][1]["posterior"]
                worst_sim = max(worst_sim, abs(float(B.num(R.sim(x, y, cn[cid])) - R.sim(x, y, cn[cid], B))))
                pairs += 1
    print("measured |reference - mpmath|: similarities %.3g, sim %.3g, over %d pairs" % (worst_aln, worst_sim, pairs))
    assert pairs >= 300
    assert worst_aln <= REF_VS_MPMATH and worst_sim <= 7.2e-15


def test_sampling_layer_matches_the_oracles():
    """the Python rand layer against oracle/rng.c draw for draw (two restatements of one published spec; parity with the crate
    itself stays unpinned), and misc::kmeans against jo_kmeans on the same generator state"""
    L = O.lib()
    for seed in (0, 1, 12345, 2 ** 63 + 7):
        a, b = O.Rng(), R.Rand085(R.Xoroshiro128PlusPlus.seed_from_u64(seed))
        L.jo_rng128pp_seed_from_u64(C.byref(a), seed)
        rng = np.random.default_rng(seed % 1000)
        for it in range(300):
            kind = it % 4
            if kind == 0:
                assert bool(L.jo_gen_bool(C.byref(a), 0.5)) == b.gen_bool(0.5)
            elif kind == 1:
                n = int(rng.integers(1, 50))
                assert L.jo_gen_range_usize(C.byref(a), n) == b.gen_range(n)
            elif kind == 2:
                n = int(rng.integers(1, 400))
                assert L.jo_gen_index(C.byref(a), n) == b.choose(n)
            else:
                w = rng.uniform(0.0, 3.0, int(rng.integers(1, 40)))
                w[rng.random(len(w)) < 0.2] = 0.0
                got = L.jo_choose_weighted(C.byref(a), O.f64p(w), len(w))
                assert (None if got < 0 else got) == b.choose_weighted(w.tolist())
    rng = np.random.default_rng(9)
    for k, n, dim in ((2, 30, 4), (3, 50, 5), (4, 41, 7), (1, 10, 3)):
        data = rng.normal(size=(n, dim)) + 3.0 * rng.integers(0, k, n)[:, None]
        a, b = O.Rng(), R.Rand085(R.Xoroshiro128PlusPlus.seed_from_u64(77 * k))
        L.jo_rng128pp_seed_from_u64(C.byref(a), 77 * k)
        for _ in range(20):
            dist, asn = C.c_double(0.0), np.zeros(n, dtype=np.uintp)
            flat = np.ascontiguousarray(data)
            assert L.jo_kmeans(O.f64p(flat), n, dim, k, C.byref(a), C.byref(dist), O.szp(asn)) == 0
            d, s = R.kmeans(data, k, b)
            assert asn.tolist() == s and abs(d - dist.value) <= 1e-12 * max(1.0, d)
