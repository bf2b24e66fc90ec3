"""jtk_lc_estimate_gains and jtk_lc_estimate_minimum_gain (jtk_amd/csrc/gains.hip) against tests/gains_reference.py, the independent
Python restatement of the gains calibration, read by read, on the cases of tests/gains_cases.py.  The reference's results come from
tests/golden/gains_reference/ (tests/golden/make_gains_reference.py writes it in minutes; tests/test_gains_reference.py recomputes
part of it on the CPU and pins the oracle to it).  Nothing here reads the reference checkout.

Until this file the two entry points were compared with the oracle alone (tests/test_gpu_parity.py), which restates
likelihood_gains.rs a second time by the same hand, and only in their final numbers: the 10th smallest of 100 medians of 50
differences and the 66th of 100 counts, which a few per cent of wrong alignments or likelihoods do not move.  edit_ops_kernel was
not looked at by any test.  Here the diagnostic switch of include/jtk_lc_debug.h (api.with_gains_batches) returns what the device
batches held, and every case compares
  templates and reads   byte for byte with the reference's, simulation by simulation in batch order: gains.hip's copy of the
                        generator and of the sampler, draw for draw;
  ops and their lengths as edit_ops_kernel wrote them, op for op with align_reference.align's; the distance recomputed from the
                        device's ops with the reference's;
  every likelihood      with phmm_reference.likelihood under that read's strand model, within the bound that
                        test_phmm_reference.assert_table_matches applies to lk (LK_RTOL |lk|);
  each median           within twice that bound at the simulation's largest |lk|; each null count exactly;
  the final numbers     gain and minimum gain within twice the bound, prob exactly; and bit for bit what the Python order statistics
                        of the reference give when fed the device's own likelihoods (nth, SEQ_NUM / 2, SAMPLE_NUM / 10,
                        SAMPLE_NUM * 2 / 3, expected_gain / 10 for substitutions only, the 1e-9 floor, max(., 1.0), the offset of
                        a second batch into the seeds and the medians) with no tolerance at all.
The exact comparisons rest on the reference's own margins (tests/test_gains_reference.py asserts them).  With the switch off the
accessors report nothing.

A read of length 0 (len6_deletions holds them, next to reads of length 1): edit_ops_kernel fills no cell and walks tl x Del;
band_prep_kernel finds no diagonal whose whole band lies inside the matrix, so phmm_kernel takes its generic steps throughout, where
the only active column is j = 0; every buffer that is sized by a read's length carries one byte or word to spare.  Read before the
first run, and the oracle run on the case on the CPU; the device agrees with the reference on every such pair.

Findings: none.  gains.hip agrees with the reference on every case.

Duration of `pytest tests -m gpu` on one MI355X: GPU_SUITE_SECONDS below.  The tests of this module take TEST_SECONDS each.

Seeded faults, each in an uncommitted copy of gains.hip built with build.build_experiment and run once: KERNEL_SEEDED_FAULTS below.
"""
import numpy as np
import pytest

import gains_cases as K
import gains_reference as G
from helpers import bits
from jtk_amd import api, ffi

pytestmark = pytest.mark.gpu
# `parent`: no full run of the parent commit was made with this change (there was machine time for one full run); the last figure
# on record for the suite is tests/test_gpu_clustering_reference.py's, two changes earlier
GPU_SUITE_SECONDS = dict(parent=None, this=(888.3, "347 passed, 1 skipped"))
TEST_SECONDS = {   # (call time of each test in the run of this module on its own; the other six take 0.01 to 0.02 s)
    "test_estimate_gains_against_the_reference[len6_asym]": 0.38, "test_estimate_gains_against_the_reference[len6_deletions]": 0.12,
    "test_estimate_gains_against_the_reference[len12_band1]": 0.21,
    "test_estimate_minimum_gain_against_the_reference[two_batches]": 0.11,   # 100,004 pairs: seq_num was not shrunk
}
# Each library was also given to the four gains tests of tests/test_gpu_parity.py (test_estimate_gains_matches_oracle,
# test_estimate_minimum_gain_matches_oracle, two cases each) in the same run.
KERNEL_SEEDED_FAULTS = {
    "(a) edit_ops_kernel's traceback writes Ins where it steps up a row and Del where it steps back a column (the moves unchanged)":
        "every test of this module that gets a result fails (the 3 of test_estimate_gains_against_the_reference, the 5 of "
        "test_estimate_minimum_gain_against_the_reference, test_nothing_is_kept_while_the_switch_is_off): the ops no longer consume the "
        "template and the read, band_prep_kernel says so and the call returns JTK_ERR_OPS_MISMATCH; only "
        "test_a_read_beyond_250_bases_is_refused passes (refused before any kernel).  The four tests of test_gpu_parity.py fail with "
        "the same status: a fault this loud was never in doubt",
    "(b) edit_ops_kernel drops the mismatch cost in the cells of a lane's second and later strides (i >= lo + 64)":
        "test_estimate_minimum_gain_against_the_reference[upper_bound] fails, at the ops of its first simulation; the 9 other tests "
        "of this module pass, second_stride among them (its anti-diagonals reach 66 cells, but the cells past the 64th lie in the "
        "matrix's corners, where no optimal path of reads that resemble their template goes: it takes len >= 130 for a second stride "
        "to cross the main diagonal).  All four tests of test_gpu_parity.py PASS on this library, at 100-base templates included: "
        "before this module nothing in the suite saw it",
}

INDEX = K.load_index()


def _split(data, off):
    data, off = bytes(data), [int(v) for v in off]
    return [data[a:b] for a, b in zip(off[:-1], off[1:])]


def _check_batches(name, batches, sizes, reads_per_sim):
    """every simulation of the case against its fixture entry; -> per simulation the device's likelihoods [2][reads]"""
    case, ref_lk = INDEX[name], K.load_lk(name)
    slices = K.sim_slices(case)
    assert [len(b["tmpl_off"]) - 1 for b in batches] == [2 * n for n in sizes], name
    out, s = [], 0
    for b, n_sims in zip(batches, sizes):
        pairs = 2 * n_sims * reads_per_sim
        assert len(b["lk"]) == len(b["ops_len"]) == len(b["read_off"]) - 1 == pairs, name
        assert int(b["tmpl_off"][0]) == 0 and int(b["read_off"][0]) == 0
        tmpls, reads = _split(b["tmpl"], b["tmpl_off"]), _split(b["reads"], b["read_off"])
        assert int(b["ops_len"].max()) <= ffi.DEBUG_GAINS_OPS_STRIDE
        ops = [row[:n].tobytes() for row, n in zip(b["ops"], b["ops_len"].tolist())]
        for k in range(n_sims):
            entry, at = slices[s]
            where = (name, "simulation", s)
            p0 = 2 * k * reads_per_sim
            sim = dict(tmpls=tmpls[2 * k:2 * k + 2], reads=reads[p0:p0 + reads_per_sim])
            # the same reads again under the second template
            assert reads[p0 + reads_per_sim:p0 + 2 * reads_per_sim] == sim["reads"], where
            assert G.digest(sim["tmpls"] + sim["reads"]) == entry["seqs"], where
            mine = ops[p0:p0 + 2 * reads_per_sim]
            assert G.digest(mine) == entry["ops"], where
            dist = np.array([G.distance_of(o) for o in mine], dtype="<u4")
            assert G.digest([dist.tobytes()]) == entry["dist"], where
            which, n_distinct = G.distinct_of(sim)
            assert n_distinct == entry["distinct"], where
            want = ref_lk[at:at + n_distinct][np.array(which)]
            got = b["lk"][p0:p0 + 2 * reads_per_sim]
            err = np.abs(got - want) - K.LK_RTOL * np.abs(want)
            assert np.all(np.isfinite(got)) and err.max() <= 0.0, where + (int(err.argmax()), got[err.argmax()], want[err.argmax()])
            out.append([got[:reads_per_sim].tolist(), got[reads_per_sim:].tolist()])
            s += 1
    assert s == len(slices), name
    return out


@pytest.mark.parametrize("name", list(K.GAINS_CASES))
def test_estimate_gains_against_the_reference(jtk_lib, name):
    case = INDEX[name]
    model, seed, seq_len, band, homop_len = K.GAINS_CASES[name]
    hf, hr = K.hmm_pair(model, ffi.Hmm)
    res, batches = api.with_gains_batches(api.estimate_gains, hf, hr, seed, seq_len, band, homop_len)
    assert jtk_lib.jtk_lc_debug_gains_batches() == 0          # nothing stays once the switch is off
    assert isinstance(res, ffi.Gains) and res.max_homopolymer_len == homop_len and len(batches) == 1
    profiles = G.profiles(homop_len)
    lks = _check_batches(name, batches, [G.SAMPLE_NUM * len(profiles)], 2 * G.SEQ_NUM)
    for q, (ty, length) in enumerate(profiles):
        medians, nulls = [], []
        for i in range(G.SAMPLE_NUM):
            entry = case["sims"][q * G.SAMPLE_NUM + i]
            base, dif = lks[q * G.SAMPLE_NUM + i]
            median, null = G.gain_decisions(ty, base, dif)[:2]
            assert abs(median - entry["median"]) <= 2 * K.bound_of(entry["scale"]), (name, q, i, median, entry["median"])
            assert null == entry["null"], (name, q, i)
            medians.append(median)
            nulls.append(null)
        got = (res.subst, res.deletions, res.insertions)[ty][length - 1]
        gain, prob = G.profile_of(medians, nulls)
        assert bits([got.gain, got.prob]).tolist() == bits([gain, prob]).tolist(), (name, ty, length, got.gain, gain, got.prob, prob)
        assert abs(got.gain - case["gain"][q]) <= 2 * K.bound_of(case["scale"]), (name, ty, length, got.gain, case["gain"][q])
        assert got.prob == case["prob"][q], (name, ty, length)
    if name == "len6_deletions":
        lens = np.diff(batches[0]["read_off"].astype(np.int64))
        assert (lens == 0).sum() == 2 * case["len0"] > 0 and (lens == 1).sum() == 2 * case["len1"] > 0


@pytest.mark.parametrize("name", [n for n, c in INDEX.items() if c["kind"] == "min_gain" and c["status"] == "ok"])
def test_estimate_minimum_gain_against_the_reference(jtk_lib, name):
    case = INDEX[name]
    model, seed, sample_num, seq_num, length, band = K.MIN_GAIN_CASES[name]
    hf, hr = K.hmm_pair(model, ffi.Hmm)
    res, batches = api.with_gains_batches(api.estimate_minimum_gain, hf, hr, seed, sample_num, seq_num, length, band)
    assert isinstance(res, float) and len(batches) == len(case["batches"])
    lks = _check_batches(name, batches, case["batches"], seq_num)
    medians = []
    for s, (base, dif) in enumerate(lks):          # (here `base` is hap1, and the difference is base - dif)
        medians.append(G.nth([base[t] - dif[t] for t in range(seq_num)], seq_num // 2))
        assert abs(medians[-1] - case["sims"][s]["median"]) <= 2 * K.bound_of(case["sims"][s]["scale"]), (name, s)
    assert bits([res]).tolist() == bits([G.minimum_gain_of(medians)[0]]).tolist(), (name, res, medians)
    assert abs(res - case["min_gain"]) <= 2 * K.bound_of(case["scale"]), (name, res, case["min_gain"])
    assert (res == G.MIN_REQ) == case["floor_decides"]
    if name == "top_bit":
        worst = max(G.distance_of(row[:n].tobytes()) for b in batches for row, n in zip(b["ops"], b["ops_len"].tolist()))
        assert worst == case["max_dist"] > 127


def test_a_read_beyond_250_bases_is_refused(jtk_lib):
    import ctypes as C
    case = INDEX["too_long"]
    model, seed, sample_num, seq_num, length, band = K.MIN_GAIN_CASES["too_long"]
    assert case["status"] == "unsupported" and case["longest"] > K.MAX_DEVICE_LEN
    hf, hr = K.hmm_pair(model, ffi.Hmm)
    res, batches = api.with_gains_batches(api.estimate_minimum_gain, hf, hr, seed, sample_num, seq_num, length, band)
    assert isinstance(res, ffi.JtkError) and res.status == -3 and "250" in str(res) and batches == []
    out = C.c_double(-7.5)
    assert jtk_lib.jtk_lc_estimate_minimum_gain(C.byref(hf), C.byref(hr), seed, sample_num, seq_num, length, band, C.byref(out), 0) == -3
    assert out.value == -7.5


def test_nothing_is_kept_while_the_switch_is_off(jtk_lib):
    model, seed, sample_num, seq_num, length, band = K.MIN_GAIN_CASES["lower_bounds"]
    hf, hr = K.hmm_pair(model, ffi.Hmm)
    res, batches = api.with_gains_batches(api.estimate_minimum_gain, hf, hr, seed, sample_num, seq_num, length, band)
    assert len(batches) == 1
    again = api.estimate_minimum_gain(hf, hr, seed, sample_num, seq_num, length, band)
    assert again == res and api.gains_batches() == [] and jtk_lib.jtk_lc_debug_gains_batches() == 0
    assert jtk_lib.jtk_lc_debug_gains_batch_sizes(0, ffi.u64p(np.zeros(4, np.uint64))) == -1
    # a call with the switch on replaces what the call before it kept
    jtk_lib.jtk_lc_debug_gains_keep(1)
    try:
        api.estimate_minimum_gain(hf, hr, seed, sample_num, seq_num, length, band)
        api.estimate_minimum_gain(hf, hr, seed + 1, sample_num, seq_num, length, band)
        assert jtk_lib.jtk_lc_debug_gains_batches() == 1
    finally:
        jtk_lib.jtk_lc_debug_gains_keep(0)
    assert jtk_lib.jtk_lc_debug_gains_batches() == 0
