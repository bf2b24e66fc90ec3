"""Merged chain launches whose segments DIFFER, on gathers that are certain (jtk_amd/csrc/session_lanes.h, launch_lane_chains,
launch_mcmc_merged; mcmc_kernel, mcmc_kernel_light and chain_split_kernel take a by-value table of up to 8 segments, one per
session of the lane, and a workgroup finds its own by a scan over the segments' first workgroups).

tests/test_gpu_lanes.py releases its sessions from a barrier: whether two of them ever share a launch is a race, and its sessions
are nearly the same segment.  Here the lane is HELD through the diagnostic entry points of include/jtk_lc_debug.h
(api.lane_hold / api.lane_state): with JTK_LC_LANES=1 every session shares lane 0, the test holds it, starts one thread per
session in a stated order -- the next only once the lane's pending count has grown, so the arrival order and with it the segment
order is the test's choice -- waits until all pend, releases, and then reads from the lane's ledger exactly which launches were
made: the member count of every call and, per chain class, the segments and the chunks of each segment.  No test passes on
outputs alone.  DEADLINE_MULTIPLE says how long a gather may take before the test gives up (a safety cap, no performance claim);
the hold is released in a `finally`, and a thread that failed before it arrived fails the test.

Cases (each the smallest shape at which the named thing can go wrong):
 (a) the five pile-ups of clustering_cases.PILEUPS as five sessions of ONE launch, each with its own batch and params and
     run(skip_polish=True), against tests/golden/clustering_reference.json (labels and cluster count as arrays, score and posterior
     rows by their bits: the assertions of test_pileup_against_the_reference).  The segments differ in haploid coverage and band
     fraction (params), post_stride (2 against 4), lds_n (80 against 24), lds_d, lds_k, and in the chain they run (light kernel,
     mcmc_chain_k2<4, 2> above 63 reads, mcmc_chain_tab<3> / <4>).  Two arrival orders: the 80-read session first and last; in both
     segment 0 has a posterior stride of 2.  The `alone` fixture asserts that pile-ups take other answers under another session's
     coverage -- that of segment 0, which is what a wrong params pointer would give them (POWER_OF_PARAMS) -- checked on the
     device alone: the Python reference needs the device's feature matrix first.
 (b) both chain classes in one gather: X = the batch of test_heterogeneous_batch_keeps_class_0_below_80_kib (a 420-read diploid
     pile-up evicted to class 1 by a shallow 7-copy one), Y = two diploid chunks (class 0 only).  Class 0 has 2 segments, class 1
     has 1, whose index in order (Y, X) is not its member's.  X_VARIANT says which X is committed and what it measured.
 (c) a middle segment with nothing to run (both chunks without a variant column: order_count == 0 in both kernels), and a
     middle session whose chunks fail before the chain (a band radius above 255): its status and return code stay, its mates'
     outputs equal theirs alone.
 (d) nine single-chunk sessions: one call of 8 and one of 1.  (Seventeen are covered on the CPU: tests/test_session_lanes.py.)
 (e) regrouping between passes: (A, B, C) gathered, then B alone and (C, A) gathered; pass 2 equals pass 1.
 (f) lane-mates that do not gather: while two sessions pend, a polish_chunks call on the same lane returns.  The split branch:
     see SPLIT_NOTE -- the parent pass of a split IS a member of the gather (S8, the small diploid pile-up declared copy number
     8), its sub-sessions are not (SR, a 48-read split with sub-problems, held a second time after the gathered launch).
 (g) case (a) once more with JTK_LC_SIDE_STREAM=0.
mcmc_kernel_huge beside a gather is not here: its launch is not merged, and its cheapest pile-up is 1,024 reads (tens of millions
of proposals in one workgroup); it stays with tests/test_gpu_shapes.py.

Durations and seeded faults: GPU_SUITE_SECONDS, TEST_SECONDS and LANE_SEEDED_FAULTS below.
"""
import json
import os
import threading
import time

import numpy as np
import pytest

import helpers
from clustering_cases import GOLDEN, PILEUPS, pileup
from jtk_amd import api, batch as jb, ffi, synth
from test_gpu_lanes import assert_same, diploid, no_variant, snapshot

pytestmark = [pytest.mark.gpu, pytest.mark.changes_env]

# A gather may take DEADLINE_MULTIPLE times the slowest session's measured single pass, plus DEADLINE_SECONDS, before the test
# gives up: sessions of one lane share a stream, so n of them need about n passes, and n <= 9 here.
DEADLINE_MULTIPLE = 20
DEADLINE_SECONDS = 5.0

# `pytest tests -m gpu` on one MI355X.  `this` is the one full run made with this module in place, when it had 12 of its 13
# tests (test_the_sub_sessions_of_a_split_launch_alone came after it: the module alone went from 18.1 s to 25.7 s); `parent` is
# derived, this less the module's 18.0 s in that run (no other GPU test was touched).
GPU_SUITE_SECONDS = dict(parent=(909.8, "derived: this less this module's 18.0 s"), this=(927.8, "525 passed, 1 skipped"),
                         this_with_the_13th_test=(935.4, "derived: this plus 7.6 s"))
# seconds per test, from one run of the module alone (25.7 s); the `alone` fixture (every session alone twice, and the power
# check of case (a): 39 short sessions, X twice at 3.1 s a pass, SR twice at 2.6 s) is the first test's setup
TEST_SECONDS = {
    "setup of the first test (the `alone` fixture)": 15.13,
    "test_both_chain_classes_in_one_gather[Y_first]": 3.12, "test_both_chain_classes_in_one_gather[X_first]": 3.12,
    "test_the_sub_sessions_of_a_split_launch_alone": 2.52,
    "test_five_reference_pileups_without_the_side_stream": 0.29, "test_five_reference_pileups_in_one_launch[80_reads_last]": 0.26,
    "test_five_reference_pileups_in_one_launch[80_reads_first]": 0.24, "test_regrouping_between_passes": 0.18,
    "test_nine_held_sessions_make_a_launch_of_eight_and_one_of_one": 0.11,
    "test_a_polish_call_on_the_lane_does_not_wait_for_the_hold": 0.07, "test_the_parent_pass_of_a_split_gathers": 0.07,
    "test_a_middle_segment_with_nothing_to_run[trivial_chunks]": 0.07, "test_a_middle_segment_with_nothing_to_run[failed_chunks]": 0.07,
    "test_hold_and_state_refuse_what_does_not_exist": 0.00,
}
# X as committed is the batch of test_heterogeneous_batch_keeps_class_0_below_80_kib unchanged (6 reads per copy in the 7-copy
# pile-up): one pass alone measured 3.06 s, under the five seconds above which the 7-read variant was to replace it (that
# variant measured 3.10 s: the 420-read diploid chain is the cost, not the 7-copy pile-up).
X_VARIANT = "full (42 reads in the 7-copy pile-up), 3.06 s a pass alone"
# The issue expected a session with a split chunk to pass by a held lane.  It does not, and should not: the PARENT pass of a split
# (the 4-way clustering of the whole pile-up) is an ordinary member of its lane's gather -- run_batch enters the gather unless the
# session is polish-only or resumes RNG streams -- so under a hold it pends like any other (test_the_parent_pass_of_a_split_gathers:
# the ledger shows it as the middle segment of three).  What launches alone are the SUB-sessions.  The small diploid pile-up
# declared copy_num = 8 (S8) has none (its 4-way clustering finds one cluster), and the smallest entry of
# helpers.RECURSIVE_SPLIT_CASES measured 12.9 s a pass alone, over the five seconds allowed, so it is not used; SR (48 reads,
# 2.6 s, six clusters, three sub-session launches) is this module's own.  test_the_sub_sessions_of_a_split_launch_alone holds
# the lane a second time as soon as the gathered launch is in the ledger: were a sub-session to enter the gather it would pend
# under that hold until the deadline.  (Should the sub-sessions ever reach their chain point before the second hold is taken the
# test still passes; it cannot fail without a fault.)
SPLIT_NOTE = "the parent pass of a split gathers; its sub-sessions do not"
# Case (a) against a wrong params pointer, measured alone on the device (each pile-up under each of the five coverages): under
# 30 (ont_diploid's, segment 0 of the order that ends with the 80-read session) hifi_diploid and ont_diploid_80_reads change
# their score bits; under 10 planted and ont_diploid_80_reads do, under 12 hifi_diploid does; under 40 (the 80-read
# session's own, segment 0 of the order that begins with it) and under 20 nothing changes, so only the 80_reads_last order has
# this power.  The fixture asserts it for that order.
POWER_OF_PARAMS = {30.0: ("hifi_diploid", "ont_diploid_80_reads"), 10.0: ("planted", "ont_diploid_80_reads"), 12.0: ("hifi_diploid",),
                   20.0: (), 40.0: ()}
# Seeded faults, one at a time in an uncommitted copy of the sources, one run of this module and one of tests/test_gpu_lanes.py per
# fault.  All four stay inside valid memory; none shrinks the LDS of a launch, drops a layout clamp or indexes past an allocation.
LANE_SEEDED_FAULTS = {
    "mcmc_segment_body hands mcmc_body the params of segment 0 (t.seg[0].params)":
        "this module: test_five_reference_pileups_in_one_launch[80_reads_last] (hifi_diploid's score is one ulp off the reference's) "
        "and test_the_sub_sessions_of_a_split_launch_alone (SR's labels under D1's coverage) fail, the 11 others pass; "
        "tests/test_gpu_lanes.py: all 4 pass (its sessions share one params' values)",
    "the wg0 scan of mcmc_segment_body with > for >= (the first workgroup of every later segment runs nothing)":
        "this module: the 12 tests that gather fail on labels or result records, test_hold_and_state_refuse_what_does_not_exist "
        "passes; tests/test_gpu_lanes.py: all 4 failed in this run (its sessions happened to meet; nothing makes them)",
    "launch_lane_chains fills segment i, the member's index, of a zeroed table instead of segment n_seg":
        "this module: test_both_chain_classes_in_one_gather[Y_first] fails on the ledger (class 1: chunks [3, 0] for [3, 1], the "
        "launch was given an empty segment 0), the 12 others pass; tests/test_gpu_lanes.py: all 4 pass (one chain class only)",
    "mcmc_segment_body hands mcmc_body the post_stride of segment 0":
        "this module, without test_both_chain_classes_in_one_gather[X_first] (with X's stride of 7 in segment 0 the fault would write "
        "past Y's posteriors): test_five_reference_pileups_in_one_launch[80_reads_last] and "
        "test_five_reference_pileups_without_the_side_stream (ont_4copy's posterior rows), "
        "test_both_chain_classes_in_one_gather[Y_first], test_the_parent_pass_of_a_split_gathers and "
        "test_the_sub_sessions_of_a_split_launch_alone fail, 7 pass -- among them, not explained, "
        "test_five_reference_pileups_in_one_launch[80_reads_first], the first test after the fixture; tests/test_gpu_lanes.py: not "
        "run (its session of stride 3 may arrive first, and the fault would then write past the others' posteriors)",
}

ORDER_80_FIRST = ("ont_diploid_80_reads", "ont_diploid", "hifi_diploid", "ont_4copy", "planted")
ORDER_80_LAST = ("ont_diploid", "hifi_diploid", "ont_4copy", "planted", "ont_diploid_80_reads")


@pytest.fixture(scope="module")
def lib(jtk_lib):
    assert jtk_lib.jtk_lc_device_ok(0) == 1, "needs a gfx950 device"
    return jtk_lib


def heterogeneous():
    """session X: the batch and params of tests/test_gpu_shapes.py::test_heterogeneous_batch_keeps_class_0_below_80_kib"""
    cfg_deep = dict(synth.CONFIGS["ont_diploid"], tmpl_len=240, reads_per_hap=210)
    cfg_wide = dict(synth.CONFIGS["ont_4copy"], tmpl_len=240, reads_per_hap=6, n_haps=7, copy_num=7, divergence=2.5e-2)
    b = jb.pack([synth.make_pileup(7100, cfg_deep, min_variants=1), synth.make_pileup(7200, cfg_wide, min_variants=2)])
    return b, jb.default_params(haploid_coverage=30.0, band_frac=cfg_deep["band_frac"])


def band_too_wide():
    """two diploid chunks of 300 bp under a band fraction of 1.8: radius ceil(540) / 2 = 270 > 255 (JTK_WIDE_MAX_RADIUS), as in
    test_band_wider_than_the_fallback_kernel_is_reported: both chunks fail before the chain"""
    b, _, p = helpers.small_batch(n_chunks=2, tmpl_len=300, reads_per_hap=3, first=770)
    p.band_frac = 1.8
    return b, p


def declared_eight_copies():
    """the batch of test_gpu_parity.py::test_edge_cases: three small diploid pile-ups declared copy number 1, 6 (trivial) and 8
    (the split branch, which finds one cluster and returns it)"""
    b, _, _ = helpers.small_batch(n_chunks=3, tmpl_len=300, reads_per_hap=3)
    b.chunks["copy_num"][0], b.chunks["copy_num"][1], b.chunks["copy_num"][2] = 1, 6, 8
    return b, jb.default_params(haploid_coverage=5.0)


def small_split():
    """one pile-up of 8 haplotypes x 6 reads on 300 bp, copy number 8: clustering_recursive's split branch with sub-problems
    (the 4-way clustering finds more than one cluster), the shape of helpers.RECURSIVE_SPLIT_CASES cut down to one small chunk"""
    b, _, p = helpers.small_batch(config="ont_4copy", n_chunks=1, tmpl_len=300, reads_per_hap=6, first=780, n_haps=8, copy_num=8,
                                  divergence=4e-2, min_variants=3)
    return b, p


PARAMS = jb.default_params(haploid_coverage=8.0, band_frac=synth.CONFIGS["ont_diploid"]["band_frac"])


def inputs():
    """name -> (batch, params, skip_polish) of every session the tests use"""
    x = {name: pileup(name) + (True,) for name in PILEUPS}
    x["X"] = heterogeneous() + (False,)
    # (diploid pile-ups of 300 bp that keep a variant column under PARAMS: the `alone` fixture asserts it)
    x["Y"] = (jb.pack([diploid(722, 9), diploid(725, 10)]), PARAMS, False)
    x["D1"] = (jb.pack([diploid(728, 11)]), PARAMS, False)
    x["D2"] = (jb.pack([diploid(731, 12), diploid(732, 10)]), PARAMS, False)
    x["D3"] = (jb.pack([diploid(733, 8), diploid(735, 11), diploid(736, 9)]), PARAMS, False)
    x["T"] = (jb.pack([no_variant(760), no_variant(761)]), PARAMS, False)
    x["F"] = band_too_wide() + (False,)
    x["S8"] = declared_eight_copies() + (False,)
    x["SR"] = small_split() + (False,)
    for i, (chunk_id, rph) in enumerate(((739, 10), (740, 8), (742, 11), (743, 9), (744, 7), (745, 12), (746, 10), (747, 8), (748, 6))):
        x["one%d" % i] = (jb.pack([diploid(chunk_id, rph)]), PARAMS, False)
    return x


def one_pass(session, skip_polish):
    session.run(skip_polish=skip_polish)
    out = session.fetch(raise_on_chunk_failure=False)
    return snapshot(out), out["rc"]


def differs(a, b):
    return not (np.array_equal(a["label"], b["label"]) and a["result"]["cluster_num"].tolist() == b["result"]["cluster_num"].tolist()
                and np.array_equal(helpers.bits(a["result"]["score"]), helpers.bits(b["result"]["score"])))


@pytest.fixture(scope="module")
def alone(lib):
    """every session of this module run alone, JTK_LC_LANES unset, once (two passes where a test runs two): name -> dict(out, rc,
    seconds, lds).  Also the power of case (a): every pile-up once more under another pile-up's haploid coverage."""
    assert "JTK_LC_LANES" not in os.environ and "JTK_LC_SIDE_STREAM" not in os.environ
    x, ref = inputs(), {}
    for name, (b, p, skip) in x.items():
        with api.Session(p, b) as s:
            t0 = time.perf_counter()
            out, rc = one_pass(s, skip)
            seconds = time.perf_counter() - t0
            lds, launches = api.last_timing()["chain_lds_bytes"], api.last_timing()["kernel_launches"]["mcmc"]
            again, rc2 = one_pass(s, skip)
        assert_same(again, out, (name, "second pass alone"))
        assert rc2 == rc
        ref[name] = dict(out=out, rc=rc, seconds=seconds, lds=lds, launches=launches)
        print("ALONE %-22s %6.3f s  chunks %d  rc %d  lds %s  chain launches %d  k %s" % (name, seconds, b.n_chunks, rc, lds, launches,
                                                                                        out["result"]["cluster_num"].tolist()))
    # the power of case (a) against a wrong params pointer: under the haploid coverage of its order's FIRST session (what a
    # kernel that took every segment's params from segment 0 would use) at least one later session answers otherwise
    power = {}
    for order in (ORDER_80_FIRST, ORDER_80_LAST):
        coverage = x[order[0]][1].haploid_coverage
        changed = []
        for name in order[1:]:
            b, p, skip = x[name]
            q = ffi.Params.from_buffer_copy(bytes(p))
            q.haploid_coverage = coverage
            with api.Session(q, b) as s:
                out, _ = one_pass(s, skip)
            if differs(out, ref[name]["out"]):
                changed.append(name)
        print("POWER under the coverage %.1f of %s: %s differ" % (coverage, order[0], changed))
        power[order] = changed
    # (no pile-up answers otherwise under the 80-read session's coverage of 40: only the order that ends with it has this power)
    assert power[ORDER_80_LAST], "no session changes label, cluster count or score bits under segment 0's coverage"
    # what the cases rest on
    assert ref["X"]["lds"][0] < ref["X"]["lds"][1] and ref["X"]["lds"][0] > 0, ref["X"]["lds"]   # one chunk in each class
    assert ref["Y"]["lds"][1] == 0
    t = ref["T"]["out"]["result"]
    assert (t["n_variants"] == 0).all() and (t["cluster_num"] == 1).all() and (t["status"] == 0).all()
    # the split of SR really has sub-problems: more chain launches than the parent's one, more than one cluster
    assert ref["SR"]["launches"] > 1 and int(ref["SR"]["out"]["result"]["cluster_num"][0]) > 1, (ref["SR"]["launches"], ref["SR"]["out"]["result"])
    assert ref["S8"]["launches"] == 1
    assert ref["F"]["rc"] == -6 and (ref["F"]["out"]["result"]["status"] == -3).all()
    for name in ("Y", "D1", "D2", "D3") + tuple("one%d" % i for i in range(9)):
        r = ref[name]["out"]["result"]
        assert (r["n_variants"] > 0).all() and (r["status"] == 0).all(), name
    ref["_power"] = power
    return x, ref


class Gate:
    """lane 0 of device 0 with JTK_LC_LANES=1: sessions made here share it"""

    def __init__(self, x, ref, names):
        self.names = list(names)
        self.sessions = [api.Session(x[n][1], x[n][0]) for n in self.names]
        self.skip = [x[n][2] for n in self.names]
        lanes = {s.lane() for s in self.sessions}
        assert lanes == {0}, ("the sessions must share one lane", lanes)
        self.deadline = DEADLINE_MULTIPLE * max(ref[n]["seconds"] for n in ref if not n.startswith("_")) + DEADLINE_SECONDS
        self.outs = [None] * len(self.names)
        self.rcs = [None] * len(self.names)
        self.errors = []

    def close(self):
        for s in self.sessions:
            s.close()

    def _work(self, i):
        try:
            self.outs[i], self.rcs[i] = one_pass(self.sessions[i], self.skip[i])
        except BaseException as e:  # noqa: BLE001 -- handed to the main thread
            self.errors.append((self.names[i], e))

    def _wait(self, what, done, thread=None):
        until = time.monotonic() + self.deadline
        while not done():
            assert not self.errors, self.errors
            assert thread is None or thread.is_alive() or done(), (what, "the thread ended before it arrived")
            assert time.monotonic() < until, (what, "not within %.1f s" % self.deadline, api.lane_state(0))
            time.sleep(0.0005)

    def gather(self, order, while_held=None, after_release=None):
        """one pass of the sessions `order` (indices), arriving in that order under a hold; returns the ledger's records of the
        launches the release made.  while_held(gate): called with all of them pending; after_release(gate, state before the
        hold, threads): called right after the release."""
        before = api.lane_state(0)
        assert (before["in_pass"], before["pending"], before["holds"]) == (0, 0, 0), before
        threads = []
        api.lane_hold(0, True)
        held = True
        try:
            for k, i in enumerate(order):
                t = threading.Thread(target=self._work, args=(i,))
                threads.append(t)
                t.start()
                self._wait((self.names[i], "arrival %d" % k), lambda: api.lane_state(0)["pending"] == k + 1, t)
            st = api.lane_state(0)
            assert st["pending"] == len(order) and st["in_pass"] == 0 and st["holds"] == 1, st
            assert st["launch_calls"] == before["launch_calls"], "a launch was made under the hold"
            if while_held:
                while_held(self)
            api.lane_hold(0, False)
            held = False
            if after_release:
                after_release(self, before, threads)
        finally:
            if held:
                api.lane_hold(0, False)
            for t in threads:
                t.join(self.deadline)
        assert not self.errors, self.errors
        assert not any(t.is_alive() for t in threads), "a session did not return after the release"
        return self.since(before)

    def since(self, before):
        after = api.lane_state(0)
        assert (after["in_pass"], after["pending"], after["holds"]) == (0, 0, 0), after
        made = after["launch_calls"] - before["launch_calls"]
        assert 0 <= made <= len(after["records"])
        return after["records"][len(after["records"]) - made:]


def record(seg_chunks_0, seg_chunks_1=(), members=None):
    """the ledger's record of one call: per class the chunks of each segment"""
    s0, s1 = list(seg_chunks_0), list(seg_chunks_1)
    return dict(members=max(len(s0), len(s1)) if members is None else members, segments=[len(s0), len(s1)],
                chunks=[sum(s0), sum(s1)], seg_chunks=[s0, s1])


@pytest.fixture
def one_lane(lib, alone, monkeypatch):
    monkeypatch.setenv("JTK_LC_LANES", "1")
    return alone


def against_the_reference(name, b, out):
    ref = json.load(open(GOLDEN))["pileups"][name]
    n, k = int(b.chunks["n_reads"][0]), ref["cluster_num"]
    assert ref["status"] == 0 and int(out["result"]["status"][0]) == 0 and int(out["result"]["cluster_num"][0]) == k, name
    assert out["label"].tolist() == ref["label"], name
    assert "%016x" % int(helpers.bits(out["result"]["score"])[0]) == ref["score"], name
    assert [["%016x" % int(v) for v in helpers.bits(row[:k])] for row in out["log_post"][:n]] == ref["post"], name


def five_pileups(x, ref, order):
    g = Gate(x, ref, order)
    try:
        made = g.gather(range(5))
    finally:
        g.close()
    assert made == [record([1] * 5)], made          # ONE launch of five segments of one chunk each, class 0
    strides = [x[n][0].post_stride for n in order]
    assert strides[0] == 2 and sorted(set(strides)) == [2, 4]
    for name, out, rc in zip(order, g.outs, g.rcs):
        assert rc == 0
        against_the_reference(name, x[name][0], out)
        assert_same(out, ref[name]["out"], (name, "gathered against alone"))


@pytest.mark.parametrize("order", [ORDER_80_FIRST, ORDER_80_LAST], ids=["80_reads_first", "80_reads_last"])
def test_five_reference_pileups_in_one_launch(one_lane, order):
    """(a)"""
    x, ref = one_lane
    for name in PILEUPS:   # alone, a session's pass gives the reference's answer too (what the gathered run is compared with)
        against_the_reference(name, x[name][0], ref[name]["out"])
    five_pileups(x, ref, order)


def test_five_reference_pileups_without_the_side_stream(one_lane, monkeypatch):
    """(g)"""
    x, ref = one_lane
    monkeypatch.setenv("JTK_LC_SIDE_STREAM", "0")
    five_pileups(x, ref, ORDER_80_FIRST)


@pytest.mark.parametrize("order", [("Y", "X"), ("X", "Y")], ids=["Y_first", "X_first"])
def test_both_chain_classes_in_one_gather(one_lane, order):
    """(b)"""
    x, ref = one_lane
    g = Gate(x, ref, order)
    try:
        made = g.gather(range(2))
    finally:
        g.close()
    chunks0 = [2, 1] if order[0] == "Y" else [1, 2]
    assert made == [record(chunks0, [1])], made      # class 0: both members; class 1: X alone, segment 0 whichever member X is
    for name, out, rc in zip(order, g.outs, g.rcs):
        assert rc == 0
        assert_same(out, ref[name]["out"], (name, order))


@pytest.mark.parametrize("middle", ["T", "F"], ids=["trivial_chunks", "failed_chunks"])
def test_a_middle_segment_with_nothing_to_run(one_lane, middle):
    """(c)"""
    x, ref = one_lane
    order = ("D1", middle, "D2")
    g = Gate(x, ref, order)
    try:
        made = g.gather(range(3))
    finally:
        g.close()
    assert made == [record([1, 2, 2])], made
    for name, out, rc in zip(order, g.outs, g.rcs):
        assert rc == ref[name]["rc"] == (-6 if name == "F" else 0), name
        assert_same(out, ref[name]["out"], (name, order))


def test_nine_held_sessions_make_a_launch_of_eight_and_one_of_one(one_lane):
    """(d)"""
    x, ref = one_lane
    order = ["one%d" % i for i in (3, 0, 8, 5, 1, 7, 2, 6, 4)]
    g = Gate(x, ref, order)
    try:
        made = g.gather(range(9))
    finally:
        g.close()
    assert made == [record([1] * 8), record([1])], made
    for name, out, rc in zip(order, g.outs, g.rcs):
        assert rc == 0
        assert_same(out, ref[name]["out"], name)


def test_regrouping_between_passes(one_lane):
    """(e): A, B, C have 1, 2 and 3 chunks, so the ledger shows who was where"""
    x, ref = one_lane
    order = ("D1", "Y", "D3")
    g = Gate(x, ref, order)
    try:
        made = g.gather([0, 1, 2])
        first = list(g.outs)
        assert made == [record([1, 2, 3])], made
        before = api.lane_state(0)
        g._work(1)                                   # B alone, no hold
        assert not g.errors, g.errors
        assert g.since(before) == [record([2])]
        second_b = g.outs[1]
        made = g.gather([2, 0])                      # C, then A
        assert made == [record([3, 1])], made
    finally:
        g.close()
    for i, name in enumerate(order):
        assert_same(first[i], ref[name]["out"], (name, "pass 1"))
        assert_same(second_b if i == 1 else g.outs[i], first[i], (name, "pass 2 against pass 1"))


def test_a_polish_call_on_the_lane_does_not_wait_for_the_hold(one_lane):
    """(f), first arrangement: polish_chunks is polish-only and enters no gather"""
    x, ref = one_lane
    b, p, _ = x["Y"]
    want = api.polish_chunks(p, b)
    got = {}

    def polish(gate):
        t = threading.Thread(target=lambda: got.update(out=api.polish_chunks(p, b)))
        t.start()
        t.join(gate.deadline)
        st = api.lane_state(0)
        assert not t.is_alive() and "out" in got, "the polish call waited for the hold"
        assert st["pending"] == 2 and st["holds"] == 1, st          # it returned while both sessions still pend

    g = Gate(x, ref, ("D1", "D2"))
    try:
        made = g.gather(range(2), while_held=polish)
    finally:
        g.close()
    assert made == [record([1, 2])], made
    for k in ("cons_off", "ops_out_off", "result"):
        assert got["out"][k].tobytes() == want[k].tobytes(), k
    n, m = int(want["cons_off"][-1]), int(want["ops_out_off"][-1])
    assert np.array_equal(got["out"]["cons"][:n], want["cons"][:n]) and np.array_equal(got["out"]["ops_out"][:m], want["ops_out"][:m])
    for name, out in zip(("D1", "D2"), g.outs):
        assert_same(out, ref[name]["out"], name)


def test_the_parent_pass_of_a_split_gathers(one_lane):
    """(f), second arrangement; see SPLIT_NOTE"""
    x, ref = one_lane
    order = ("D1", "S8", "D2")
    g = Gate(x, ref, order)
    try:
        made = g.gather(range(3))
    finally:
        g.close()
    assert made == [record([1, 3, 2])], made
    for name, out, rc in zip(order, g.outs, g.rcs):
        assert rc == 0
        assert_same(out, ref[name]["out"], name)


def test_the_sub_sessions_of_a_split_launch_alone(one_lane):
    """(f), second arrangement, with a split that has sub-problems: the parent pass gathers with its lane-mates; as soon as that
    launch is in the ledger the lane is held AGAIN, and the split's sub-sessions (which resume RNG streams and enter no gather)
    must finish under that hold, with nothing pending and no further call in the ledger"""
    x, ref = one_lane
    order = ("D1", "SR", "D2")
    seen = {}

    def hold_again(gate, before, threads):
        gate._wait("the gathered launch", lambda: api.lane_state(0)["launch_calls"] == before["launch_calls"] + 1)
        api.lane_hold(0, True)
        try:
            for t in threads:
                t.join(gate.deadline)
            seen.update(alive=[t.is_alive() for t in threads], state=api.lane_state(0))
        finally:
            api.lane_hold(0, False)

    g = Gate(x, ref, order)
    try:
        made = g.gather(range(3), after_release=hold_again)
    finally:
        g.close()
    assert seen["alive"] == [False] * 3, "a sub-session of the split waited for the hold"
    assert (seen["state"]["pending"], seen["state"]["in_pass"], seen["state"]["holds"]) == (0, 0, 1), seen["state"]
    assert made == [record([1, 1, 2])], made
    for name, out, rc in zip(order, g.outs, g.rcs):
        assert rc == 0
        assert_same(out, ref[name]["out"], name)


def test_hold_and_state_refuse_what_does_not_exist(one_lane):
    with pytest.raises(ffi.JtkError) as e:
        api.lane_hold(31, True)                      # JTK_LC_LANES=1: there is no lane 31
    assert e.value.status == -1
    with pytest.raises(ffi.JtkError) as e:
        api.lane_hold(0, True, device=15)
    assert e.value.status == -1
    with pytest.raises(ffi.JtkError) as e:
        api.lane_hold(0, False)                      # a release without a hold
    assert e.value.status == -1
    with pytest.raises(ffi.JtkError):
        api.lane_state(31)
    st = api.lane_state(0)
    assert (st["in_pass"], st["pending"], st["holds"]) == (0, 0, 0)
