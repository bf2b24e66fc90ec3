"""oracle/pseudo_mcmc.c, oracle/misc.c and oracle/local_clustering.c against tests/clustering_reference.py, the independent Python
restatement of the read clustering (CPU only).  The problems are tests/clustering_cases.py; test_cases_reach_their_branches asserts
on the reference's own log that every case entered the branch it is named for.

Function level (jo_kmeans, jo_mcmc_with_filter, jo_mcmc_clustering, jo_cluster_filtered_variants, jo_reassign_and_posterior): the
same generator state on both sides; the state and the draw count after the call are equal, results are compared as arrays and
floats by their bits.  Whole chunks (jo_cluster_features): labels, cluster_num, score and posterior rows.

Back ends.  With the project's exp / log (ProjectMath) everything is compared for equality, floats by their bits.  With libm the
labels and the cluster count must be equal and
    LIBM_TOLERANCE = 1024 ulp of the largest magnitude that enters the sums (the size table's largest entry, or the score).  A
                     size-table entry is max over c of x ln(c cov) - c cov - (ln 1 + .. + ln x): up to n + 1 <= 12 logarithms of
                     one ulp each, the first amplified by x <= 11, so at most 23 + 11 = 34 ulp of log error and 12 roundings of the
                     running sum: 46 ulp per entry.  A score is a chain's maximum, which holds k <= 4 entries (184 ulp) plus up to
                     k dim <= 18 exactly representable gains (18 roundings), minus the same k entries summed again (184 ulp and 4
                     roundings): 390 ulp.  A posterior is an exact gain minus logsumexp (k exps, one log, k + 1 roundings: 10 ulp).
                     390 rounded up to the next power of two is 512; one more factor of two because the ulp is taken at the
                     largest magnitude while libm and jtk_math.h may each be one ulp off (pinned to within one ulp of EACH OTHER
                     only for exp and log separately).  Absolute bound = 1024 * 2^-52 * max(|size table|, |score|, 1).
    DECISION_BOUND = 1e-10: a decision of the reference (log.margin) closer than this to its threshold may flip between the two
                     libraries: 390 ulp of a size table below 256 in magnitude (asserted per case) is 2.2e-11.  A libm case may
                     differ in labels only if its log shows such a decision, and at most one case in ten may (asserted; share
                     measured: 0 of 24).
Feature cases: none dropped for the reference's cost; read counts are 2 to 11 (clustering_cases.CASES) and 64 to 256
(LARGE_CASES: the smallest shape of every device path past 63 reads, each with a predicate on the reference's log,
test_large_cases_reach_their_branches).  The large cases run with the project's exp / log ONLY.  The libm comparison is not
extended to them: LIBM_TOLERANCE counts n + 1 <= 12 logarithms per size-table entry and DECISION_BOUND assumes a size table below
256 in magnitude, and neither holds at 256 reads (257 logarithms; 256 ln 256 alone is 1420).  Not covered at any size:
mcmc_kernel_huge's shapes (more than 1,023 reads: 41 M proposals per tried k) and the recursive split of copy numbers of 8 and
more; both stay pinned to the oracle by tests/test_gpu_parity.py and tests/test_gpu_shapes.py.  Pile-ups (clustering_cases.PILEUPS): ont_diploid
and hifi_diploid as synth makes them, ont_4copy reduced to 8 reads per haplotype on 200 bp (at 160 reads the Python chain took
386 s), and `planted`, 24 hand-made reads whose variants fail one filter each (clustering_cases.planted); the same run on the
device.  test_planted_columns_are_dropped_by_their_own_filter adds a profile matrix at the filter's interface for the columns no
read can carry (copy rows, the positions just inside the mask, an insertion next to its own base).  A fifth pile-up,
ont_diploid_80_reads (40 reads per haplotype on 200 bp, five candidate columns, three picked), is the only one above 63 reads.

The references are computed once per process, in a pool of up to 8 worker processes, and compared with
tests/golden/clustering_reference.json, the committed outputs the GPU module reads (tests/golden/make_clustering_reference.py
writes it).  Measured run time of this module, everything included: see RUN_TIME below; the slowest CPU module before it,
tests/test_trace_rows.py, takes about 100 s.

Seeded faults, one at a time in an uncommitted copy of the oracle, and the test of this module that then fails: see
SEEDED_FAULTS below.
"""
import ctypes as C
import functools
import json
import math
import os

import numpy as np
import pytest

import clustering_cases as K
import clustering_reference as R
import oracle_ffi as O
from filter_cases import planted_profiles
from helpers import bits, oracle_params
from jtk_amd import batch as jb, ffi

LIBM_TOLERANCE = 1024
RUN_TIME = ("about 320 to 390 s on 8 CPUs, 77 tests (two measured runs; the parent: about 180 s, 56 tests): 165 to 200 s for the feature references in the pool "
            "(both back ends for the small cases, the project's for the 16 large ones: 1,400 CPU-seconds; the longest single job is tab4_68_reads, three "
            "tried k, 161 s on its own, then tab2_256_reads, 109 s), 20 + 30 + 70 + 8 + 38 s of Python chain for the five pile-ups, 10 s for the three large "
            "single chains")
SEEDED_FAULTS = {   # one-line changes to an uncommitted copy of oracle/: the tests of this module that then fail
    "max_by keeps the first of the 20 restarts": "test_feature_chunk_against_the_reference[diploid_1_column, diploid_4_columns, "
                                                 "diploid_6_columns, diploid_nine_columns, three_copies, four_copies, one_column_four_copies, zero_rows]",
    "gen_bool(1.0) consumes a draw": "test_feature_chunk_against_the_reference[three_copies, four_copies, zero_rows], "
                                     "test_one_chain_against_the_oracle[zero_rows]",
    "<= for < in the stop rule": "test_feature_chunk_against_the_reference[stop_rule_exact_tie]",
    "no_new_variants dropped from expected_gains": "test_feature_chunk_against_the_reference[no_new_variants_decides]",
    "chi-square threshold on the wrong side": "test_planted_columns_are_dropped_by_their_own_filter, test_candidate_columns_against_the_oracle",
    # at 64 reads and more (the other large cases pass with either; so does every case of CASES and every small chain):
    "the size prior read at size - 1 for sizes of 64 and more": "test_feature_chunk_against_the_reference[light_127_reads_2_columns, "
                                                                "k2_127_reads_8_columns, k2_120_reads_70_and_50, tab2_128_reads_3_columns, tab2_255_reads, "
                                                                "tab2_256_reads], test_one_chain_against_the_oracle[k2_120_reads_70_and_50]",
    "an accepted move of a read of index 64 or more leaves the column counts as they were":
        "test_feature_chunk_against_the_reference[every large case but light_64_reads_1_column and k2_64_reads_3_columns, which have no such read], "
        "test_one_chain_against_the_oracle[k2_120_reads_70_and_50, light_81_reads_zero_rows, tab3_66_reads]",
    "POS_FRAC compared with <=": "none, and none can: num_pos / (num_pos + num_neg + 1e-7) equals the double 0.70 only if 0.7e-7 / "
                                 "(num_pos + num_neg) is below half an ulp of 0.7 (5.6e-17), i.e. beyond 1e9 reads in one cluster; at every "
                                 "reachable count `<` and `<=` agree (7 positives of 10 give 0.69999999, not informative either way)",
}
DECISION_BOUND = 1e-10
NAMES = list(K.CASES)
LARGE_NAMES = list(K.LARGE_CASES)   # 64 to 256 reads: the project's exp / log only
ALL_CASES = dict(K.CASES, **K.LARGE_CASES)
GOLDEN, PILEUPS, pileup = K.GOLDEN, K.PILEUPS, K.pileup


def params_of(case):
    return jb.default_params(case["coverage"])


def _reference(arg):
    name, backend = arg
    c = ALL_CASES[name]()
    gains = R.Gains.from_params(params_of(c))
    B = R.ProjectMath() if backend == "project" else R.LibmMath
    return R.cluster_features(c["x"].tolist(), c["vt"].tolist(), c["copy_num"], c["coverage"], c["local_coverage"], gains, c["chunk_id"], B)


@functools.lru_cache(maxsize=None)
def references():
    """{(case, back end): clustering_reference.cluster_features' result}, all at once in worker processes"""
    import multiprocessing as mp
    O.lib()
    jobs = [(n, b) for b in ("project", "libm") for n in NAMES] + [(n, "project") for n in LARGE_NAMES]
    shape = {n: (ALL_CASES[n]()["x"].shape, ALL_CASES[n]()["copy_num"]) for n in ALL_CASES}
    # proposals (2000 n per restart and tried k) times the work of one (the columns of k clusters, a fixed part): the longest first
    cost = {n: rows * sum(4 + k * dim for k in range(2, max(cp, 2) + 1)) for n, ((rows, dim), cp) in shape.items()}
    jobs.sort(key=lambda j: -cost[j[0]])
    with mp.get_context("fork").Pool(min(8, os.cpu_count() or 1)) as pool:
        return dict(zip(jobs, pool.map(_reference, jobs, chunksize=1)))


def oracle_features(case):
    x = case["x"]
    n, dim = x.shape
    cp = case["copy_num"]
    ch = np.zeros(1, dtype=ffi.FEATURE_CHUNK_DT)
    ch[0] = (case["chunk_id"], cp, n, dim, 0, 0, 0, 0, case["local_coverage"])
    lab, post, res = np.zeros(n, np.uint32), np.zeros((n, cp)), np.zeros(1, dtype=ffi.RESULT_DT)
    var = np.ascontiguousarray(x.ravel() if x.size else np.zeros(1))
    vts = np.ascontiguousarray(case["vt"].ravel().astype(np.uint32) if dim else np.zeros(2, np.uint32))
    rc = O.lib().jo_cluster_features(C.byref(oracle_params(params_of(case))), 1, ch.ctypes.data, O.f64p(var), O.u32p(vts), O.u32p(lab),
                                     O.f64p(post), cp, res.ctypes.data, 1)
    return rc, lab, post, res[0]


def as_fixture(out):
    """what the GPU module needs of a reference result, JSON-ready (floats as their bit patterns)"""
    if out["status"] != 0:
        return dict(status=out["status"])
    hexbits = lambda xs: ["%016x" % int(b) for b in bits(np.array(xs, dtype=np.float64).ravel())]
    return dict(status=0, label=out["label"], cluster_num=out["cluster_num"], score=hexbits([out["score"]])[0],
                post=[hexbits(row) for row in out["post"]], draws=out["log"].draws)


# ---------------------------------------------------------------------------------------------------------------------------
# generator and function level
# ---------------------------------------------------------------------------------------------------------------------------
def both_rngs(seed):
    mine = R.Rand085(R.Xoshiro256StarStar.seed_from_u64(seed))
    theirs = O.Rng()
    O.lib().jo_rng_seed_from_u64(C.byref(theirs), seed)
    return mine, theirs


def same_rng(mine, theirs):
    return list(theirs.s) == list(mine.core.state()) and int(theirs.draws) == mine.core.draws


def test_generator_known_answers(oracle):
    g = R.Xoshiro256StarStar([1, 2, 3, 4])   # the vector of the xoshiro256** reference implementation (rand_xoshiro's own test)
    assert [g.next_u64() for _ in range(4)] == [11520, 0, 1509978240, 1215971899390074240]
    for seed in (0, 1, 3490 * 1000, (1 << 64) - 1):
        mine, theirs = both_rngs(seed)
        assert same_rng(mine, theirs)
        for k in (2, 3, 4, 7):
            for old in range(k):   # (0..k).filter(|&c| c != old).choose(rng): value and draw count
                assert mine.choose_iter([c for c in range(k) if c != old]) == O.lib().jo_choose_other(C.byref(theirs), k, old)
                assert same_rng(mine, theirs)
        for p in (0.5, 1.0, 0.0, 1e-9, 1.0 - 2.0 ** -53):
            assert mine.gen_bool(p) == bool(O.lib().jo_gen_bool(C.byref(theirs), p)) and same_rng(mine, theirs)
        for n in (1, 2, 3, 10, 1 << 33):
            assert mine.gen_range(n) == O.lib().jo_gen_range_usize(C.byref(theirs), n) and same_rng(mine, theirs)
            assert mine.gen_index(n) == O.lib().jo_gen_index(C.byref(theirs), n) and same_rng(mine, theirs)
    assert R.chunk_rng(7).core.state() == R.Xoshiro256StarStar.seed_from_u64(7 * 3490).state()


def _flat(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64).ravel())


SMALL = ["diploid_2_columns", "three_copies", "duplicate_rows", "zero_rows", "noise_only", "one_column_four_copies"]


@pytest.mark.parametrize("name", SMALL)
def test_kmeans_against_the_oracle(oracle, name):
    c = K.CASES[name]()
    x = c["x"]
    n, dim = x.shape
    paths = set()
    for k in (1, 2, 3):
        for seed in range(12):
            mine, theirs = both_rngs(seed * 131 + k)
            asn = np.zeros(n, dtype=np.uintp)
            dist = C.c_double(0)
            rc = O.lib().jo_kmeans(O.f64p(_flat(x)), n, dim, k, C.byref(theirs), C.byref(dist), O.szp(asn))
            log = R.Log()
            try:
                d, a = R.kmeans(x.tolist(), k, mine, log)
            except R.ReferencePanic:
                assert rc == -1, (k, seed)
                paths.add("panic")
                continue
            assert rc == 0 and a == asn.tolist() and bits([d])[0] == bits([dist.value])[0], (k, seed)
            assert same_rng(mine, theirs), (k, seed)
            paths.add("random" if log.kmeans["random_start"] else "seeded")
    assert {"random", "seeded"} <= paths
    if name == "duplicate_rows":
        assert "panic" in paths   # two distinct rows, k = 3: every weight is zero


LARGE_CHAINS = ["k2_120_reads_70_and_50", "light_81_reads_zero_rows", "tab3_66_reads"]   # one start each per k: 3 to 5 s a chain


@pytest.mark.parametrize("name", SMALL + LARGE_CHAINS)
def test_one_chain_against_the_oracle(oracle, name):
    c = ALL_CASES[name]()
    x = c["x"]
    n, dim = x.shape
    B = R.ProjectMath()
    for k in range(2, min(c["copy_num"], 1 + 2 * dim) + 1):
        for seed in range(1 if name in LARGE_CHAINS else 3):
            mine, theirs = both_rngs(seed + 17 * k)
            start = [int(v) for v in np.random.default_rng(seed).integers(0, k, n)]
            asn = np.array(start, dtype=np.uintp)
            lk = O.lib().jo_mcmc_with_filter(O.f64p(_flat(x)), n, dim, O.szp(asn), k, c["coverage"], C.byref(theirs))
            got = list(start)
            want = R.mcmc_with_filter(x.tolist(), got, k, c["coverage"], mine, B)
            assert got == asn.tolist() and bits([want])[0] == bits([lk])[0], (k, seed)
            assert same_rng(mine, theirs), (k, seed)


@pytest.mark.parametrize("name", ["diploid_nine_columns", "one_column_four_copies"])
def test_restarts_and_cluster_count_against_the_oracle(oracle, name):
    """mcmc_clustering, cluster_filtered_variants and the tail, each through its own oracle entry"""
    c = K.CASES[name]()
    x = c["x"]
    n, dim = x.shape
    B = R.ProjectMath()
    gains = R.Gains.from_params(params_of(c))
    # mcmc_clustering
    mine, theirs = both_rngs(99)
    asn, score, lkg, used = np.zeros(n, dtype=np.uintp), C.c_double(0), np.zeros(n), np.zeros(dim, dtype=np.uint8)
    rc = O.lib().jo_mcmc_clustering(O.f64p(_flat(x)), n, dim, 2, c["coverage"], C.byref(theirs), O.szp(asn), C.byref(score), O.f64p(lkg),
                                    O.u8p(used))
    a, s, g, u = R.mcmc_clustering(x.tolist(), 2, c["coverage"], mine, B)
    assert rc == 0 and a == asn.tolist() and bits([s])[0] == bits([score.value])[0]
    assert np.array_equal(bits(g), bits(lkg)) and [bool(v) for v in used] == u and same_rng(mine, theirs)
    # cluster_filtered_variants
    mine, theirs = both_rngs(c["chunk_id"] * 3490)
    p = oracle_params(params_of(c))
    cfg = O.ClusterConfig(0, C.pointer(p.gains), c["coverage"], c["copy_num"], c["local_coverage"])
    homop = np.ascontiguousarray(c["vt"][:, 0], dtype=np.uintp)
    types = np.ascontiguousarray(c["vt"][:, 1], dtype=np.intc)
    asn, lkg, score, k_out = np.zeros(n, dtype=np.uintp), np.zeros(n * c["copy_num"]), C.c_double(0), C.c_size_t(0)
    rc = O.lib().jo_cluster_filtered_variants(O.f64p(_flat(x)), n, dim, O.szp(homop), types.ctypes.data_as(C.POINTER(C.c_int)), C.byref(cfg),
                                              C.byref(theirs), O.szp(asn), O.f64p(lkg), C.byref(score), C.byref(k_out))
    a, g, s, k = R.cluster_filtered_variants(x.tolist(), [tuple(v) for v in c["vt"].tolist()], c["copy_num"], c["coverage"],
                                             c["local_coverage"], gains, mine, B)
    assert rc == 0 and k == k_out.value and a == asn.tolist() and bits([s])[0] == bits([score.value])[0] and same_rng(mine, theirs)
    assert np.array_equal(bits(_flat(g)), bits(lkg[:n * k]))
    # the tail
    O.lib().jo_reassign_and_posterior(n, k, O.szp(asn), O.f64p(lkg))
    a2, post = R.reassign_and_posterior(a, g, B)
    assert a2 == asn.tolist() and np.array_equal(bits(_flat(post)), bits(lkg[:n * k]))


def test_the_tail_on_its_own(oracle):
    """:98-105: the last maximum, `lks[asn] + 0.001 < max` moving a label, and the margin keeping one"""
    B = R.ProjectMath()
    rows = [[1.0, 1.0005, 0.5], [1.0, 1.002, 1.002], [0.0, 0.0, 0.0], [-3.0, -1.0, -2.0], [2.0, 2.001, 2.0]]
    start = [0, 0, 1, 2, 0]
    log = R.Log()
    a, post = R.reassign_and_posterior(start, rows, B, log)
    assert a == [0, 2, 1, 1, 0] and log.tail == dict(changed=2, within_margin=2)
    asn, lkg = np.array(start, dtype=np.uintp), _flat(rows)
    O.lib().jo_reassign_and_posterior(5, 3, O.szp(asn), O.f64p(lkg))
    assert asn.tolist() == a and np.array_equal(bits(lkg), bits(_flat(post)))


# ---------------------------------------------------------------------------------------------------------------------------
# whole chunks
# ---------------------------------------------------------------------------------------------------------------------------
def test_cases_reach_their_branches():
    refs = references()
    for name in NAMES:
        out = refs[(name, "project")]
        assert (out["status"] != 0) == (name in K.PANICS), (name, out["panic"])
        if name in K.REACHES:
            assert out["status"] == 0 and K.REACHES[name](out["log"]), name
    assert set(K.REACHES) | set(K.PANICS) == set(NAMES)
    logs = [out["log"] for (name, b), out in refs.items() if b == "project" and out["status"] == 0]
    for what, reached in K.REACHED_SOMEWHERE.items():
        assert any(reached(g) for g in logs), what
    tried = {t["k"] for g in logs for t in g.tried}
    assert tried == {2, 3, 4}
    assert {len(K.CASES[n]()["vt"]) for n in NAMES if K.CASES[n]()["copy_num"] == 2} >= {1, 2, 3, 4, 6, 9}
    panics = {refs[(n, "project")]["panic"].split(":")[0] for n in K.PANICS}
    assert panics == {"choose_weighted(..).unwrap()", "LKCount", "gen_bool"}   # (a NaN value reaches the weights first)


def test_large_cases_reach_their_branches():
    """every case of 64 reads and more: the predicate it is listed with holds on the reference's own log, and between them the
    cases run every (kernel, chain) of the dispatch they were drawn for, as clustering_cases.device_path restates it"""
    refs = references()
    assert set(K.LARGE_REACHES) == set(LARGE_NAMES)
    for name in LARGE_NAMES:
        out = refs[(name, "project")]
        assert out["status"] == 0, (name, out["panic"])
        print(name, K.device_path(K.LARGE_CASES[name]()), out["log"].chain, [(t["k"], t["accepted"], t["sizes"]) for t in out["log"].tried])
        assert K.LARGE_REACHES[name](out["log"]), name
    logs = [refs[(name, "project")]["log"] for name in LARGE_NAMES]
    for what, reached in K.LARGE_REACHED_SOMEWHERE.items():
        assert any(reached(g) for g in logs), what
    assert {K.device_path(K.LARGE_CASES[n]()) for n in LARGE_NAMES} == K.LARGE_PATHS
    assert {K.device_path(K.CASES[n]())[1] for n in NAMES if K.CASES[n]()["x"].size and K.CASES[n]()["copy_num"] >= 2} == {
        "mcmc_chain_k2<1, 1>", "mcmc_chain_k2<2, 1>", "mcmc_chain_k2<3, 1>", "mcmc_chain_k2<4, 1>", "mcmc_chain_k2<8, 1>",
        "mcmc_chain_tab<2> SMALL", "mcmc_chain_tab<3> SMALL", "mcmc_chain_tab<4> SMALL"}
    shapes = {(c["copy_num"], c["x"].shape[0], c["x"].shape[1]) for c in (K.LARGE_CASES[n]() for n in LARGE_NAMES)}
    assert {(n, d) for cp, n, d in shapes if cp == 2} >= {(64, 1), (65, 2), (127, 2), (64, 3), (127, 8), (120, 3), (128, 3), (70, 9),
                                                          (255, 1), (256, 1)}
    assert {d for cp, n, d in shapes if cp == 2 and 64 <= n <= 127} >= {1, 2, 3, 4, 6, 8}
    assert {(cp, n) for cp, n, d in shapes if cp > 2} == {(3, 66), (4, 68)}
    for name in LARGE_NAMES:   # the haploid coverage is that of a pile-up of this many reads: within a fifth of n / copy_num
        c = K.LARGE_CASES[name]()
        assert abs(c["coverage"] * c["copy_num"] / len(c["x"]) - 1.0) <= 0.2, name


@pytest.mark.parametrize("name", NAMES + LARGE_NAMES)
def test_feature_chunk_against_the_reference(oracle, name):
    ref = references()[(name, "project")]
    c = ALL_CASES[name]()
    rc, lab, post, res = oracle_features(c)
    if ref["status"] != 0:
        assert rc != 0 and res["status"] == -6, ref["panic"]
        return
    assert rc == 0 and res["status"] == 0
    k = ref["cluster_num"]
    assert int(res["cluster_num"]) == k and lab.tolist() == ref["label"]
    assert bits([res["score"]])[0] == bits([ref["score"]])[0], (float(res["score"]), ref["score"])
    assert np.array_equal(bits(post[:, :k]), bits(np.array(ref["post"]).reshape(len(lab), k)))


def test_feature_chunks_with_libm(oracle):
    """the reference as a Rust build evaluates it (libm) against the oracle (jtk_math.h): bounds in the module docstring"""
    refs = references()
    left_out, compared, worst = [], 0, 0.0
    for name in NAMES:
        ref = refs[(name, "libm")]
        c = K.CASES[name]()
        rc, lab, post, res = oracle_features(c)
        if ref["status"] != 0:
            assert rc != 0 and res["status"] == -6
            continue
        compared += 1
        k = ref["cluster_num"]
        if int(res["cluster_num"]) != k or lab.tolist() != ref["label"]:
            assert ref["log"].margin < DECISION_BOUND, (name, ref["log"].margin)
            left_out.append(name)
            continue
        n = len(lab)
        table = max([1.0, abs(ref["score"])] + [abs(x * math.log(max(c["coverage"], 1e-300) * q) - c["coverage"] * q) + math.lgamma(x + 1)
                                                for x in range(n + 1) for q in range(1, c["copy_num"] + 1)])
        assert table < 256.0, name   # what DECISION_BOUND assumes
        tol = LIBM_TOLERANCE * 2.0 ** -52 * table
        err = max([abs(float(res["score"]) - ref["score"])] + [float(np.abs(post[:, :k] - np.array(ref["post"]).reshape(n, k)).max())])
        print("%-28s |oracle - libm reference| %.3g (bound %.3g), smallest decision margin %.3g" % (name, err, tol, ref["log"].margin))
        worst = max(worst, err / tol)
        assert err <= tol, name
    print("left out: %d of %d %s; largest error / bound %.3g" % (len(left_out), compared, left_out, worst))
    assert 10 * len(left_out) <= compared


def as_pileup_fixture(ref):
    return dict(as_fixture(ref), cands=cand_rows(ref))


def test_inlined_chain_is_the_plain_one(oracle):
    """mcmc_with_filter writes the generator, the flip and get_lk out in its loop; mcmc_with_filter_plain goes through the
    helpers.  Same labels, maximum, generator state and draw count, for k = 2 and k = 3."""
    B = R.ProjectMath()
    for name, k in (("zero_rows", 2), ("one_column_four_copies", 3), ("weak_columns", 2)):
        c = K.CASES[name]()
        x = c["x"].tolist()
        a, b = both_rngs(5)[0], both_rngs(5)[0]
        start = [int(v) for v in np.random.default_rng(1).integers(0, k, len(x))]
        one, two = list(start), list(start)
        got = R.mcmc_with_filter(x, one, k, c["coverage"], a, B)
        want = R.mcmc_with_filter_plain(x, two, k, c["coverage"], b, B)
        assert one == two and bits([got])[0] == bits([want])[0], name
        assert a.core.state() == b.core.state() and a.core.draws == b.core.draws, name


def test_committed_reference_outputs_are_the_live_ones():
    """tests/golden/clustering_reference.json (read by tests/test_gpu_clustering_reference.py) against the reference run here"""
    gold = json.load(open(GOLDEN))
    refs = references()
    assert sorted(gold["cases"]) == sorted(NAMES) and sorted(gold["large_cases"]) == sorted(LARGE_NAMES)
    for name in NAMES:
        assert gold["cases"][name] == as_fixture(refs[(name, "project")]), name
    for name in LARGE_NAMES:
        assert gold["large_cases"][name] == as_fixture(refs[(name, "project")]), name
    assert sorted(gold["pileups"]) == sorted(PILEUPS)
    for config in PILEUPS:
        assert gold["pileups"][config] == as_pileup_fixture(pileup_reference(config)), config


# ---------------------------------------------------------------------------------------------------------------------------
# which columns become candidates
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", list(PILEUPS))
def test_candidate_columns_against_the_oracle(oracle, config):
    """filter_profiles' selection (:426-466) restated in numpy from the oracle's per-read tables: the TOTAL count and the CAND
    set (column, row, lk, count) are the oracle's rows, and filter + pick + clustering together give the oracle's labels
    (skip_polish: the template the tables are taken on is the one given).  ont_4copy is reduced to 32 reads on 200 bp for the
    reference's cost."""
    from jtk_amd import synth
    b, p = pileup(config)
    po = oracle_params(p)
    out, rows = O.trace_chunk(po, b, 0, skip_polish=True)
    ref = pileup_reference(config)
    copy_num, n = int(b.chunks["copy_num"][0]), int(b.chunks["n_reads"][0])
    local = n / copy_num if copy_num <= 2 else max(n / copy_num, float(p.haploid_coverage))
    assert int(rows[0].split("\t")[1]) == len(ref["cands"]) > 0
    want = [r.split("\t")[1:] for r in rows if r.startswith("CAND\t")]
    assert want == cand_rows(ref)
    if config == "planted":   # every planted column dropped by the filter it was planted for, the one left a candidate
        col = K.planted()[2]
        for name, _, why in K.PLANTED:
            assert ref["dropped"].get(col[name]) == why and (col[name] in [c[0] for c in ref["cands"]]) == (why is None), name
        assert {"edge", "row", "homopolymer", "strand", "gain_per_count"} <= set(ref["dropped"].values())
    else:
        assert {"row", "homopolymer", "pvalue"} <= set(ref["dropped"].values())   # (a HiFi pile-up has no gain near its ends)
    assert ref["status"] == 0 and ref["label"] == out["label"].tolist() and ref["cluster_num"] == int(out["result"]["cluster_num"][0])
    assert bits([ref["score"]])[0] == bits(out["result"]["score"])[0]
    k = ref["cluster_num"]
    assert np.array_equal(bits(out["log_post"][:, :k]), bits(np.array(ref["post"]).reshape(n, k)))
    if config == "ont_4copy":   # copy_num > 2: the Poisson term over k = 1 .. 4, local_coverage = max(n / copy_num, coverage), k = 2 .. 4
        assert copy_num == 4 and local == float(p.haploid_coverage) > n / copy_num and ref["log"].range == (2, 4)


def cand_rows(ref):
    return [[str(pos // 14), str(pos % 14), "%.1f" % lk, str(count)] for pos, lk, count in ref["cands"]]


@functools.lru_cache(maxsize=None)
def pileup_reference(config):
    """clustering_reference.cluster_profiles on the oracle's per-read tables of the pile-up (table - lk, as the numpy test of
    tests/test_trace_rows.py takes them)"""
    b, p = pileup(config)
    po = oracle_params(p)
    tmpl = b.template(0)
    radius = int(math.ceil(len(tmpl) * p.band_frac)) // 2
    tabs = []
    for r in b.chunk_reads(0):
        tab, lk = O.modification_table(po.forward if b.strand[r] else po.reverse, tmpl, b.read(r), b.read_ops(r), radius)
        tabs.append(tab - lk)
    strands = [bool(b.strand[r]) for r in b.chunk_reads(0)]
    copy_num, n = int(b.chunks["copy_num"][0]), len(tabs)
    local = n / copy_num if copy_num <= 2 else max(n / copy_num, float(p.haploid_coverage))   # mod.rs:108-111
    return R.cluster_profiles(np.array(tabs), tmpl, strands, R.Gains.from_params(p), copy_num, float(p.haploid_coverage), local,
                              int(b.chunks["chunk_id"][0]), R.ProjectMath())


def test_planted_columns_are_dropped_by_their_own_filter(oracle):
    """the oracle's filter_profiles (TOTAL / CAND rows and the picked columns) against the restatement on planted_profiles(), and
    from the restatement's own record: every planted column was dropped by the filter it was planted for, the others kept"""
    tmpl, prof, strands, where, why = planted_profiles()
    p = jb.default_params(5.0)
    gains = R.Gains.from_params(p)
    cands, dropped = R.filter_candidates(prof, tmpl, strands, gains, 2, 5.0, R.ProjectMath())
    kept = {pos for pos, _, _ in cands}
    for name, (bp, row) in where.items():
        pos = bp * 14 + row
        if why[name] is None:
            assert pos in kept and pos not in dropped, name
        else:
            assert dropped.get(pos) == why[name] and pos not in kept, (name, dropped.get(pos))
    assert len(kept) == sum(w is None for w in why.values())
    # the boundaries: chi-square of the strand-biased column is 12 (perfect association of 12 reads), of the others 0; the small
    # gain is 18 against 6 * 0.8 * 4.556 = 21.9 while its count's p-value passes; bp 7 and 54 = temp_len - 7 are inside the mask
    picks = R.pick_filtered_profiles(cands, prof, 2)
    po = oracle_params(p)
    cfg = O.ClusterConfig(0, C.pointer(po.gains), 5.0, 2, 6.0)
    L = O.lib()
    buf = C.create_string_buffer(1 << 16)
    t = O.Trace(C.cast(buf, C.c_void_p), len(buf), 0)
    pos_out, score_out = np.zeros(6, dtype=np.uintp), np.zeros(6)
    st = np.array(strands, dtype=np.uint8)
    flat = np.ascontiguousarray(prof.ravel())
    L.jo_trace_set(C.byref(t))
    try:
        d = L.jo_filter_profiles(O.u8p(tmpl), len(tmpl), O.f64p(flat), len(prof), O.u8p(st), C.byref(cfg), O.szp(pos_out), O.f64p(score_out))
    finally:
        L.jo_trace_set(None)
    rows = buf.raw[:t.len].decode().splitlines()
    assert rows[0] == "TOTAL\t%d" % len(cands)
    assert [r.split("\t")[1:] for r in rows if r.startswith("CAND\t")] == [[str(pos // 14), str(pos % 14), "%.1f" % lk, str(c)]
                                                                          for pos, lk, c in cands]
    assert pos_out[:d].tolist() == [pos for pos, _ in picks] and np.array_equal(bits(score_out[:d]), bits([lk for _, lk in picks]))
