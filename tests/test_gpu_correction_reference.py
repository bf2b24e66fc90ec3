"""jtk_lc_correct_clustering (correction.hip) against tests/correction_reference.py, the independent Python restatement of
phmm_likelihood_correction.rs, and against oracle/correction.c, on the problems of tests/correction_cases.py with the every-job
hook of include/jtk_lc_debug.h on.

  * EVERY corrected chunk's raw similarity matrix is within TOLERANCE of the reference (the bound of
    tests/test_correction_reference.py: 8 x (reference-vs-mpmath + oracle-vs-reference, both measured on the CPU), never measured
    against the kernel) and bit-equal to the oracle's (one oracle call per chunk with selection=[id]);
  * outcomes (status, labels, cluster_num, touched flags, the rewritten posteriors) as in the CPU module, the reference running on
    the oracle's eigen-basis;
  * several jobs of different member count and longest arm in ONE call, at the default budget and with JTK_CC_SIMS_BUDGET small
    enough for one job per batch (the scratch rows are sized by the longest arm of the batch): identical matrices;
  * one call with more ordered pairs than the kernel's 262,144 threads (the grid-stride loop and its job look-up take a second
    trip): whole matrices against the oracle, a fixed-seed sample of 2,400 pairs against the reference, with pair indices on both
    sides of 262,144 and the first and last pair of every job;
  * the two-pass case of hard posteriors, and the stray-chunk cases by status.
"""
import numpy as np
import pytest

import correction_cases as K
import correction_reference as R
import test_correction_reference as T
from helpers import bits
from jtk_amd import api, ffi

pytestmark = pytest.mark.gpu


def device_run(ds, selection, min_gain):
    prob = R.flatten(ds)
    chunks = prob["chunks"].copy()
    try:
        cluster, touched, sims = api.correct_clustering_with_sims(prob["read_id"], prob["node_off"], prob["nodes"], prob["posteriors"], chunks,
                                                                  np.asarray(selection, dtype=np.uint64), ds["coverage"], min_gain)
        rc = 0
    except ffi.JtkError as e:
        rc, sims = e.status, []
        cluster, touched = np.zeros(len(prob["nodes"]), np.uint64), np.zeros(len(prob["nodes"]), np.uint8)
    return dict(rc=rc, cluster=cluster, touched=touched, chunks=chunks, sims=sims, ari=None)


def compare(ref, ds, selection, min_gain):
    dev = device_run(ds, selection, min_gain)
    ora = T.oracle_run(ds, selection, min_gain)
    assert dev["rc"] == ref["status"] == ora["rc"]
    if ref["status"] != 0:
        return dev
    assert len(dev["sims"]) == len(ref["per_chunk"])
    for got, (cid, pc) in zip(dev["sims"], ref["per_chunk"].items()):
        assert got.shape == pc["raw_sims"].shape, cid
        worst = float(np.abs(got - pc["raw_sims"]).max())
        print("|device - reference| on chunk %d: %.3g" % (cid, worst))
        assert worst <= T.TOLERANCE, cid
        assert np.array_equal(bits(got), bits(T.oracle_sims(ds, cid, pc["n"]))), cid
    assert np.array_equal(dev["cluster"], ora["cluster"]) and np.array_equal(dev["touched"], ora["touched"])
    assert np.array_equal(dev["chunks"], ora["chunks"])
    dev["ari"] = ora["ari"]  # the device entry point does not return it; everything else below is the device's
    T.compare_outcomes(ref, dev, ds, exact_labels=True)
    return dev


@pytest.mark.parametrize("name", T.NAMES)
def test_every_job_against_reference_and_oracle(name):
    m = T.made(name)
    compare(T.reference(name), m["ds"], m["selection"], m["min_gain"])


def test_stray_chunk_statuses():
    for name, want in (("stray_chunk_alone", 0), ("stray_chunk_meets_itself", -6), ("stray_chunk_above_largest_id", -6)):
        m = T.made(name)
        assert device_run(m["ds"], m["selection"], m["min_gain"])["rc"] == want == T.reference(name)["status"], name


def test_two_passes():
    m = T.made("hard_posteriors")
    first = compare(T.reference("hard_posteriors"), m["ds"], m["selection"], m["min_gain"])
    ds2 = R.written_back(m["ds"], first["cluster"], first["touched"], first["chunks"]["cluster_num"])
    assert ds2["reads"] == K.two_pass_input(T.reference("hard_posteriors"), m)["reads"]
    sel = [c["id"] for c in ds2["chunks"]]
    ref2 = R.correct(ds2, sel, 1e9, eigen=T.jacobi)
    assert ref2["status"] == 0 and ref2["stats"]["upper_cut"] > 0 and ref2["stats"]["lower_cut"] > 0
    compare(ref2, ds2, sel, 1e9)


@pytest.mark.changes_env
def test_jobs_of_different_shape_in_one_call_and_one_per_batch(monkeypatch):
    m = K.several_jobs_of_different_shape()
    ref = R.correct(m["ds"], m["selection"], m["min_gain"], eigen=T.jacobi)
    shapes = {(pc["n"]) for pc in ref["per_chunk"].values()}
    assert ref["status"] == 0 and len(shapes) >= 3
    longest = []
    for cid in ref["per_chunk"]:
        longest.append(max(max(len(c[0]), len(c[2])) for c in (R.to_context(r, i) for r, i in R.members_of(m["ds"], cid))))
    assert len(set(longest)) >= 2 and max(longest) == 19   # the rows are sized by one job's arm, the others are shorter
    assert not [d for d in ref["decisions"] if d[0] != "spectral gap" and 0.0 < d[2] < T.TIE_MARGIN]
    one_call = compare(ref, m["ds"], m["selection"], m["min_gain"])
    monkeypatch.setenv("JTK_CC_SIMS_BUDGET", "10")   # fewer doubles than any matrix: every job is its own batch
    batched = compare(ref, m["ds"], m["selection"], m["min_gain"])
    assert len(one_call["sims"]) == len(batched["sims"]) == 4
    for a, b in zip(one_call["sims"], batched["sims"]):
        assert np.array_equal(bits(a), bits(b))


def test_more_pairs_than_threads():
    m = K.more_pairs_than_threads()
    ds, sel = m["ds"], m["selection"]
    dev = device_run(ds, sel, 1e9)
    assert dev["rc"] == 0 and len(dev["sims"]) == len(sel)
    sizes = [s.shape[0] for s in dev["sims"]]
    first_pair = np.concatenate([[0], np.cumsum([n * n for n in sizes])])
    assert first_pair[-1] > 262144 and sum(1 for f in first_pair[:-1] if f < 262144) >= 2 and first_pair[-2] >= 262144
    for cid, got in zip(sel, dev["sims"]):   # whole matrices against the oracle
        assert np.array_equal(bits(got), bits(T.oracle_sims(ds, cid, got.shape[0]))), cid
    ora = T.oracle_run(ds, sel, 1e9)
    assert ora["rc"] == 0 and np.array_equal(dev["cluster"], ora["cluster"]) and np.array_equal(dev["chunks"], ora["chunks"])
    # the reference on a sample of pair indices: both sides of 262,144, the first and last pair of every job
    rng = np.random.default_rng(17)
    total = int(first_pair[-1])
    picks = set(rng.integers(0, 262144, 1200).tolist()) | set(rng.integers(262144, total, 1200).tolist())
    picks |= {262143, 262144, 262145} | {int(f) + 1 for f in first_pair[:-1]} | {int(f) - 2 for f in first_pair[1:]}
    assert len(picks) >= 2000
    cn = R.estimate_copy_number_of_cluster(ds)
    ctx = {cid: [R.to_context(r, i) for r, i in R.members_of(ds, cid)] for cid in sel}
    memo, worst = {}, 0.0
    for p in sorted(picks):
        job = int(np.searchsorted(first_pair, p, side="right")) - 1
        i, j = divmod(p - int(first_pair[job]), sizes[job])
        want = 0.0 if i == j else R.alignment(ctx[sel[job]][i], ctx[sel[job]][j], cn, memo=memo)
        worst = max(worst, abs(want - dev["sims"][job][i, j]))
    print("|device - reference| over %d sampled pairs: %.3g" % (len(picks), worst))
    assert worst <= T.TOLERANCE
