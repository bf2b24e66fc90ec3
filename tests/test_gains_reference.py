"""The oracle's gains calibration (oracle/likelihood_gains.c with the sampler and the bootstrap likelihood of oracle/phmm.c) against
tests/gains_reference.py, the independent Python restatement, on the cases of tests/gains_cases.py; and the fixture
tests/golden/gains_reference/ against a recomputation.  The device is pinned to the same reference, read by read, in
tests/test_gpu_gains_reference.py; until these two files the gains calibration was compared with nothing but the oracle, which
restates likelihood_gains.rs by the same hand as jtk_amd/csrc/gains.hip does.

  fixture     the minimum-gain cases of a few pairs are recomputed whole and compared with the fixture entry by entry; of the gains
              cases (20,000 pairs per profile) simulations 3 and 98 of every profile, and of two_batches sample 3 (the one in the
              second device batch), chosen here and not by the fixture.  Digests, null counts and numbers of distinct pairs are
              equal; likelihoods and medians agree to 1e-13 relative (numpy's logaddexp on another libm).
  margins     no decision of the reference (a null-count comparison, which difference is the median, which median is the final
              number, whether the floor decides) sits within 100 x the likelihood bound of its threshold.  Stored per case by the
              generator, asserted here, case by case, and once more for the part of it on which the exact comparisons of both test
              files rest, the null-count comparisons and the floor.  Seeds, and for len12_band1 the model, were chosen for it on the
              reference alone (tests/gains_cases.py says why that case needs a noisy model).
  oracle      jo_estimate_gain: gain within twice the bound, prob equal; jo_estimate_minimum_gain within twice the bound (too_long
              included: the oracle has no 250-base limit); jo_generate_seq and jo_phmm_gen byte for byte and state for state from
              equal generator states, under all ten models of the cases; jo_phmm_likelihood_bootstrap within the bound, a read of
              length 0 included.
  arguments   both device entry points refuse sample_num < 3, len 1 and 201, band 0 and 31, homop_len 0 and 9, seq_len 1, seq_num 0
              and null pointers with JTK_ERR_INVALID_ARG before they look for a device, and leave *out alone.

The bound: test_phmm_reference.LK_RTOL |lk|, the one assert_table_matches applies to a likelihood.  A median is an order statistic
of differences of two likelihoods, each within the bound, so it moves by at most twice the bound at the largest |lk| of its
simulation (`scale`); the final numbers are order statistics of medians.

Findings: none.  The oracle and the reference agree on every case; so does the device (tests/test_gpu_gains_reference.py).

Run time: 25 s for this file on one CPU (15 s of it the 24 recomputed simulations of the gains cases, 10 s of those len12_band1's).
"""
import ctypes as C

import numpy as np
import pytest

import gains_cases as K
import gains_reference as G
import oracle_ffi as O
from jtk_amd import ffi
from test_clustering_reference import same_rng

INDEX = K.load_index()
RECOMPUTE_RTOL = 1e-13


def _same_entry(entry, lk_fix, sim, where):
    e, lk = K.sim_entry(sim)
    for key in ("seqs", "ops", "dist", "distinct", "null"):
        assert e.get(key) == entry.get(key), (where, key)
    assert np.allclose(lk, lk_fix, rtol=RECOMPUTE_RTOL, atol=0), where
    assert abs(e["median"] - entry["median"]) <= RECOMPUTE_RTOL * entry["scale"], where
    assert abs(e["scale"] - entry["scale"]) <= RECOMPUTE_RTOL * entry["scale"], where
    for got, want in ((e["margin"], entry["margin"]), (e["exact_margin"], entry["exact_margin"])):
        assert got == want or abs(got - want) <= 2 * RECOMPUTE_RTOL * entry["scale"], (where, got, want)


@pytest.mark.parametrize("name", [n for n in K.MIN_GAIN_CASES if n not in K.RECOMPUTED_SAMPLES])
def test_small_cases_recomputed(name):
    case, lk = INDEX[name], K.load_lk(name)
    assert case["args"] == list(K.MIN_GAIN_CASES[name]) and len(case["sims"]) == case["args"][2]
    medians = []
    for s, (entry, at) in enumerate(K.sim_slices(case)):
        sim = K.min_gain_sample(name, s)
        _same_entry(entry, lk[at:at + entry["distinct"]], sim, (name, s))
        medians.append(sim["median"])
    value = G.minimum_gain_of(medians)[0]
    assert abs(value - case["min_gain"]) <= RECOMPUTE_RTOL * case["scale"]
    assert case["batches"] == G.batch_sizes(case["args"][2], case["args"][3]) == [case["args"][2]]


@pytest.mark.parametrize("name", list(K.GAINS_CASES))
def test_gains_simulations_recomputed(name):
    case, lk = INDEX[name], K.load_lk(name)
    slices = K.sim_slices(case)
    assert case["args"] == list(K.GAINS_CASES[name]) and len(slices) == G.SAMPLE_NUM * len(G.profiles(case["args"][4]))
    assert case["profiles"] == [list(p) for p in G.profiles(case["args"][4])]
    for q, i, sim in K.gains_sims(name, pick=K.RECOMPUTED_SIMS):
        entry, at = slices[q * G.SAMPLE_NUM + i]
        _same_entry(entry, lk[at:at + entry["distinct"]], sim, (name, q, i))
    # the final numbers follow from the stored medians and counts
    for q in range(len(case["profiles"])):
        ss = case["sims"][q * G.SAMPLE_NUM:(q + 1) * G.SAMPLE_NUM]
        assert G.profile_of([e["median"] for e in ss], [e["null"] for e in ss]) == (case["gain"][q], case["prob"][q])


def test_second_batch_sample_recomputed():
    name = "two_batches"
    case, lk = INDEX[name], K.load_lk(name)
    slices = K.sim_slices(case)
    assert case["batches"] == [3, 1] and len(slices) == 4
    for s in K.RECOMPUTED_SAMPLES[name]:
        entry, at = slices[s]
        _same_entry(entry, lk[at:at + entry["distinct"]], K.min_gain_sample(name, s), (name, s))
    assert G.minimum_gain_of([e["median"] for e in case["sims"]])[0] == case["min_gain"]


@pytest.mark.parametrize("name", list(K.GAINS_CASES) + list(K.MIN_GAIN_CASES))
def test_no_decision_of_the_reference_is_close_to_its_threshold(name):
    """no null-count comparison, choice of a median or choice of the final order statistic of the reference within 100 x the bound of
    its threshold.  (Why len12_band1 runs under the `noisy` model: tests/gains_cases.py.)"""
    case = INDEX[name]
    print(name, "margin", case["margin"], "exact_margin", case["exact_margin"], "needed", K.MARGIN_FACTOR * K.bound_of(case["scale"]))
    assert case["margin"] >= K.MARGIN_FACTOR * K.bound_of(case["scale"]), (name, case["margin"], case["scale"])


def test_no_exactly_compared_decision_is_close_to_its_threshold():
    assert set(INDEX) == set(K.GAINS_CASES) | set(K.MIN_GAIN_CASES)
    for name, case in INDEX.items():
        assert case["exact_margin"] >= K.MARGIN_FACTOR * K.bound_of(case["scale"]), (name, case["exact_margin"], case["scale"])
        assert case["margin"] <= min(e["margin"] for e in case["sims"]) and case["scale"] == max(e["scale"] for e in case["sims"])
        assert case["margin"] <= case["exact_margin"] <= min(e["exact_margin"] for e in case["sims"])


def test_cases_reach_what_they_are_for():
    """from the reference's own sequences (the generator asserts the same before it writes)"""
    assert INDEX["len6_deletions"]["len0"] > 0 and INDEX["len6_deletions"]["len1"] > 0
    assert INDEX["second_stride"]["max_diagonal"] >= 65 and INDEX["upper_bound"]["max_diagonal"] > 192
    assert INDEX["top_bit"]["max_dist"] > 127 and INDEX["top_bit"]["longest"] <= K.MAX_DEVICE_LEN
    assert INDEX["too_long"]["longest"] > K.MAX_DEVICE_LEN and INDEX["too_long"]["status"] == "unsupported"
    assert [n for n, c in INDEX.items() if c["status"] != "ok"] == ["too_long"]
    assert INDEX["top_bit"]["floor_decides"] and INDEX["top_bit"]["min_gain"] == G.MIN_REQ
    assert not INDEX["second_stride"]["floor_decides"] and INDEX["second_stride"]["min_gain"] > G.MIN_REQ
    assert INDEX["two_batches"]["batches"] == [3, 1]
    for name in INDEX:
        f, r = K.models()[INDEX[name]["args"][0]]
        assert not np.allclose(f.flat(), r.flat(), rtol=1e-3), name


# ---- the oracle

@pytest.mark.parametrize("name", list(K.GAINS_CASES))
def test_oracle_estimate_gain(oracle, name):
    case = INDEX[name]
    model, seed, seq_len, band, homop_len = K.GAINS_CASES[name]
    hf, hr = K.hmm_pair(model, O.Hmm)
    out = O.Gains()
    O.lib().jo_estimate_gain(C.byref(hf), C.byref(hr), seed, seq_len, band, homop_len, C.byref(out))
    assert out.max_homopolymer_len == homop_len
    for q, (ty, length) in enumerate(case["profiles"]):
        got = (out.subst, out.deletions, out.insertions)[ty][length - 1]
        assert abs(got.gain - case["gain"][q]) <= 2 * K.bound_of(case["scale"]), (name, ty, length, got.gain, case["gain"][q])
        assert got.prob == case["prob"][q], (name, ty, length, got.prob, case["prob"][q])


@pytest.mark.parametrize("name", list(K.MIN_GAIN_CASES))
def test_oracle_estimate_minimum_gain(oracle, name):
    case = INDEX[name]
    model, seed, sample_num, seq_num, length, band = K.MIN_GAIN_CASES[name]
    hf, hr = K.hmm_pair(model, O.Hmm)
    got = O.lib().jo_estimate_minimum_gain(C.byref(hf), C.byref(hr), seed, sample_num, seq_num, length, band, 4)
    assert abs(got - case["min_gain"]) <= 2 * K.bound_of(case["scale"]), (name, got, case["min_gain"])
    if case["floor_decides"]:
        assert got == G.MIN_REQ


def _rng_pair(seed):
    theirs = O.Rng()
    O.lib().jo_rng_seed_from_u64(C.byref(theirs), seed)
    return G.rng_of(seed), theirs


def test_oracle_generate_seq_and_gen(oracle):
    """from equal generator states: the same bytes and the same state afterwards, so a different number or order of draws shows
    even where the bytes agree"""
    L = O.lib()
    for name, (f, r) in K.models().items():
        for k, m in enumerate((f, r)):
            mine, theirs = _rng_pair(1000 * k + len(name))
            h = m.fill(O.Hmm())
            for n in (1, 2, 9, 66, 200):
                buf = np.zeros(n, dtype=np.uint8)
                L.jo_generate_seq(C.byref(theirs), n, O.u8p(buf))
                tmpl = G.generate_seq(mine, n)
                assert bytes(buf) == tmpl and same_rng(mine, theirs), (name, k, n)
                for _ in range(6):
                    cap = 3 * n + 1024            # (the oracle writes into a buffer; no read of these models comes near it)
                    out = np.zeros(cap, dtype=np.uint8)
                    w = L.jo_phmm_gen(C.byref(h), O.u8p(buf), n, C.byref(theirs), O.u8p(out), cap)
                    assert bytes(out[:w]) == G.gen_read(m, tmpl, mine) and same_rng(mine, theirs), (name, k, n)


def test_oracle_bootstrap_likelihood(oracle):
    L = O.lib()
    seen0 = 0
    for name, band, n in (("asym", 1, 12), ("asym", 30, 66), ("deletions", 3, 9), ("sparse", 25, 120), ("insertions", 25, 80)):
        f, r = K.models()[name]
        rng = G.rng_of(len(name) + n)
        for k in range(12):
            tmpl = G.generate_seq(rng, n - k % 2)
            read = b"" if (name == "deletions" and k == 0) else G.gen_read((f, r)[k % 2], tmpl, rng)
            seen0 += len(read) == 0
            h = (f, r)[k % 2].fill(O.Hmm())
            x, y = O.seq(tmpl), np.frombuffer(read, dtype=np.uint8).copy() if read else np.zeros(1, np.uint8)
            got = L.jo_phmm_likelihood_bootstrap(C.byref(h), O.u8p(x), len(tmpl), O.u8p(y), len(read), band)
            ops, dist, want = G.Scorer(f, r, band)(k, tmpl, read)
            assert np.isfinite(want) and abs(got - want) <= K.bound_of(abs(want)), (name, k, got, want)
            assert bytes(O.edit_ops(x, y[:len(read)])) == ops and G.distance_of(ops) == dist
    assert seen0 >= 1


# ---- argument checks of the device entry points: refused before a device is looked for

def test_entry_points_refuse_bad_arguments(jtk_lib):
    hf, hr = K.hmm_pair("asym", ffi.Hmm)
    f, r = C.byref(hf), C.byref(hr)
    out = C.c_double(-7.5)
    bad = [(f, r, 1, 2, 4, 10, 3, C.byref(out)), (f, r, 1, 3, 0, 10, 3, C.byref(out)), (f, r, 1, 3, 4, 1, 3, C.byref(out)),
           (f, r, 1, 3, 4, 201, 25, C.byref(out)), (f, r, 1, 3, 4, 10, 0, C.byref(out)), (f, r, 1, 3, 4, 10, 31, C.byref(out)),
           (None, r, 1, 3, 4, 10, 3, C.byref(out)), (f, None, 1, 3, 4, 10, 3, C.byref(out)), (f, r, 1, 3, 4, 10, 3, None)]
    for args in bad:
        assert jtk_lib.jtk_lc_estimate_minimum_gain(*args, 0) == -1, args[2:7]
        assert out.value == -7.5 and b"jtk_lc_estimate_minimum_gain" in jtk_lib.jtk_lc_last_error()
    g = ffi.Gains()
    g.max_homopolymer_len = 77
    bad = [(f, r, 1, 6, 3, 0, C.byref(g)), (f, r, 1, 6, 3, 9, C.byref(g)), (f, r, 1, 1, 3, 1, C.byref(g)), (f, r, 1, 6, 0, 1, C.byref(g)),
           (f, r, 1, 6, 31, 1, C.byref(g)), (None, r, 1, 6, 3, 1, C.byref(g)), (f, None, 1, 6, 3, 1, C.byref(g)), (f, r, 1, 6, 3, 1, None)]
    for args in bad:
        assert jtk_lib.jtk_lc_estimate_gains(*args, 0) == -1, args[2:6]
        assert g.max_homopolymer_len == 77 and b"jtk_lc_estimate_gains" in jtk_lib.jtk_lc_last_error()
    # the diagnostic accessors report nothing: no call has kept anything
    assert jtk_lib.jtk_lc_debug_gains_batches() == 0
    assert jtk_lib.jtk_lc_debug_gains_batch_sizes(0, ffi.u64p(np.zeros(4, np.uint64))) == -1
    assert jtk_lib.jtk_lc_debug_gains_batch(0, None, None, None, None, None, None, None) == -1
