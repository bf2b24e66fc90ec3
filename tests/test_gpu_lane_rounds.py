"""Merged polish rounds on gathers that are certain (jtk_amd/csrc/session_lanes.h: RoundGather; session.hip: launch_lane_rounds;
the round kernels reset_pass / band_prep / phmm / sum_final / select_edits / rethread / commit, each of which takes a table of
up to eight sessions' segments).  With JTK_LC_LANES=1 every session shares lane 0; the test holds the lane's ROUND gather
(api.round_hold), starts one thread per session, waits until all are parked, releases, and reads from the lane's round ledger
(api.round_state) which launches were made: per call the members, and per member its step (the opening or a polish round),
its chunks and its reads in phmm_kernel's item space -- read back from the segment table the kernels were given.  Every
case compares labels, posterior bits, result records, consensus and ops with each session ALONE (tests/test_gpu_lanes.py's
comparison; alone, a session goes through the same kernels as a table of one segment, which the reference tests pin), in two
passes, and asserts the merge it is about from the ledger.  No test passes on outputs alone.

Once every session of the lane that is in its polish phase is parked the launch is made, and a session leaves its polish phase
only when its own round counter says so, so after a common start the ledger is exact: a session whose slowest chunk needs R polish
rounds takes part in the opening and the rounds 0 .. R (one round is always queued ahead).

Band radius.  The pile-ups are the size tests/test_gpu_lanes.py uses (300 bp templates, 12 - 24 reads), but under its band
fraction of 0.03 their radius is 4, which is phmm_pair_kernel's (radius <= 14): such a session has pair items and does not merge
(case 5 uses exactly that).  phmm_kernel takes radius 15 .. 30, so the sessions here run under a band fraction of 0.12
(radius 18).  Polish rounds: chosen from the generator's pile-ups 800 .. 823 so that the sessions differ (template error 0.001:
1 - 3 rounds; 0.03: 3 - 10 rounds at 300 bp, so no longer template is needed); the `alone` fixture asserts from
result["polish_rounds"] that one pile-up converges in round 1 and one needs >= 4.

Not here, and why.  A chunk with take_num set inside a table of several: only the sub-sessions of the split branch and the
polish_chunks calls set it, and they enter no gather (case 5 has one beside a gather).  A pile-up deep enough for batch_needs_tables: more than 65,535 reads, not a matter of seconds; the plan's CPU test covers the
switch.
"""
import os
import threading
import time

import numpy as np
import pytest

from jtk_amd import api, batch as jb, ffi, synth
from test_gpu_lanes import assert_same, snapshot

pytestmark = [pytest.mark.gpu, pytest.mark.changes_env]

# Seeded faults, one at a time in an uncommitted build beside the product (a macro around the one changed line), one run each of
# the named tests (made when the table forms were kernels of their own beside single-session ones; the names are today's).
# Each was first checked to stay inside valid memory.
SEEDED_FAULTS = {
    "sum_final_kernel reads the state of segment 0 (where segment 0 has at least as many chunks, so that the index stays "
    "inside the array)":
        "test_nine_sessions_launch_as_eight_and_one fails on the ledger (39 member-launches for 32: sessions go on polishing on "
        "column totals summed for another session's template length).  test_three_sessions_released_together passes: there "
        "segment 0 is A with one chunk and the guard leaves B and C their own state -- the run says nothing about that test.",
    "commit_kernel stores a round's count in the slot of the next round (device counter and pinned mirror)":
        "test_three_sessions_released_together[1] fails on the ledger: every session stops after round 1.",
    "phmm_kernel takes only_active from segment 0":
        "NOT caught, by any test, and cannot be on outputs: every kernel of a round is idempotent on a chunk that is not active "
        "(the sweep of a converged chunk rewrites the row sums it already holds, band_prep its deltas), and in round 0, where "
        "only_active is 0, every chunk is active.  The fault costs time, not results; the ledger does not see a flag.",
    "a segment's first item off by one":
        "not run.  Shifted towards the next segment the last index of a segment is one past its reads (phmm_kernel and "
        "select_edits have no bound to stop it); shifted the other way band_prep and rethread return at their n_reads guard, "
        "but then reads keep uninitialised band words or ops lengths, which the next kernel uses as loop bounds and row "
        "indices.  No variant was found that stays inside valid memory, and a fault on a shared device is not a test.",
}

DEADLINE_SECONDS = 60.0   # a safety cap on every wait, no performance claim
BAND_FRAC = 0.12          # radius ceil(300 * 0.12) / 2 = 18: phmm_kernel's
PARAMS = jb.default_params(haploid_coverage=8.0, band_frac=BAND_FRAC)


def pile(chunk_id, rph, tmpl_err=1e-3, tmpl_len=300):
    cfg = dict(synth.CONFIGS["ont_diploid"], tmpl_len=tmpl_len, reads_per_hap=rph, tmpl_err=tmpl_err)
    return synth.make_pileup(chunk_id, cfg, min_variants=1)


def other_model():
    """PARAMS with another pair-HMM: a second hmm2 in the same launch"""
    h = ffi.default_hmm()
    h.mat_mat, h.mat_ins, h.mat_del = 0.94, 0.03, 0.03
    return jb.default_params(haploid_coverage=8.0, band_frac=BAND_FRAC, hmm=h)


def broken_ops():
    """two pile-ups, the second with a read whose ops do not consume its template: band_prep fails the chunk (status != 0)"""
    b = jb.pack([pile(806, 6), pile(803, 6)])
    first = int(b.chunks["read_first"][1])
    o = int(b.ops_off[first])
    k = o + int(np.flatnonzero(b.ops[o:int(b.ops_off[first + 1])] == 0)[0])
    b.ops[k] = 3   # a Match becomes a Del: one read base is left over
    return b


def inputs():
    """name -> (batch, params); the chunk counts of A, B, C differ so that the ledger shows who was where"""
    x = {
        "A": (jb.pack([pile(800, 6)]), PARAMS),                                        # 1 round: converges at once
        "B": (jb.pack([pile(801, 6), pile(806, 6)]), PARAMS),                          # 2 and 3 rounds
        "C": (jb.pack([pile(801, 6, 3e-2), pile(803, 6, 3e-2), pile(804, 6)]), PARAMS),  # 4, 5 and 1 rounds
        "LONG": (jb.pack([pile(802, 6, tmpl_len=420), pile(805, 10, tmpl_len=420)]), PARAMS),  # another max_tmpl / max_read
        "MODEL": (jb.pack([pile(807, 6), pile(809, 6), pile(810, 6), pile(811, 6)]), other_model()),
        "BROKEN": (broken_ops(), PARAMS),
        # sessions that must not merge
        "PAIR": (jb.pack([pile(812, 6), pile(813, 6), pile(814, 6), pile(815, 6), pile(816, 6)]),
                 jb.default_params(haploid_coverage=8.0, band_frac=0.03)),             # radius 4: pair items
        "WIDE": (jb.pack([pile(817 + i, 6) for i in range(6)]),
                 jb.default_params(haploid_coverage=8.0, band_frac=0.5)),              # radius 75: phmm_wide_kernel
    }
    for i in range(9):
        x["one%d" % i] = (jb.pack([pile(800 + i, 6)]), PARAMS)
    return x


def one_pass(session):
    session.run()
    out = session.fetch(raise_on_chunk_failure=False)
    return snapshot(out), out["rc"]


@pytest.fixture(scope="module")
def lib(jtk_lib):
    assert jtk_lib.jtk_lc_device_ok(0) == 1, "needs a gfx950 device"
    return jtk_lib


@pytest.fixture(scope="module")
def alone(lib):
    """every session alone, JTK_LC_LANES unset, two passes (computed once, never changed): name -> dict(out, rc, rounds)"""
    assert "JTK_LC_LANES" not in os.environ
    x, ref = inputs(), {}
    for name, (b, p) in x.items():
        with api.Session(p, b) as s:
            out, rc = one_pass(s)
            again, rc2 = one_pass(s)
        assert_same(again, out, (name, "second pass alone"))
        assert rc2 == rc
        ok = out["result"]["status"] == 0
        ref[name] = dict(out=out, rc=rc, rounds=int(out["result"]["polish_rounds"][ok].max()))
        print("ALONE %-7s chunks %d rc %d polish rounds %s status %s" % (name, b.n_chunks, rc, out["result"]["polish_rounds"].tolist(),
                                                                      out["result"]["status"].tolist()))
    every = np.concatenate([ref[n]["out"]["result"]["polish_rounds"] for n in ("A", "B", "C")])
    assert (every == 1).any() and (every >= 4).any(), every          # one converges in round 1, one needs >= 4
    assert ref["A"]["rounds"] == 1                                    # every chunk of A converges in round 0
    assert len({ref[n]["rounds"] for n in ("A", "B", "C")}) == 3      # the three sessions differ
    st = ref["BROKEN"]["out"]["result"]["status"]
    assert st[0] == 0 and st[1] != 0, st
    return x, ref


class Lane:
    """lane 0 of device 0 with JTK_LC_LANES=1: sessions made here share it"""

    def __init__(self, x, names, lanes=None):
        self.names = list(names)
        self.sessions = [api.Session(x[n][1], x[n][0]) for n in self.names]
        assert [s.lane() for s in self.sessions] == (lanes or [0] * len(self.names)), "the sessions' lanes"
        self.outs, self.rcs, self.errors = [None] * len(names), [None] * len(names), []
        self.threads = []

    def close(self):
        for s in self.sessions:
            s.close()

    def start(self, i):
        def work():
            try:
                self.outs[i], self.rcs[i] = one_pass(self.sessions[i])
            except BaseException as e:  # noqa: BLE001 -- handed to the main thread
                self.errors.append((self.names[i], e))
        t = threading.Thread(target=work)
        self.threads.append(t)
        t.start()

    def wait(self, what, done):
        until = time.monotonic() + DEADLINE_SECONDS
        while not done():
            assert not self.errors, self.errors
            assert time.monotonic() < until, (what, api.round_state(0))
            time.sleep(0.0005)

    def join(self):
        for t in self.threads:
            t.join(DEADLINE_SECONDS)
        assert not self.errors, self.errors
        assert not any(t.is_alive() for t in self.threads), "a session did not return"
        self.threads = []

    def together(self, order):
        """one pass of the sessions `order`, parked in that order under a hold and released together; the ledger's records"""
        before = api.round_state(0)
        assert (before["in_rounds"], before["parked"], before["holds"]) == (0, 0, 0), before
        api.round_hold(0, True)
        held = True
        try:
            for k, i in enumerate(order):
                self.start(i)
                self.wait((self.names[i], "parks"), lambda: api.round_state(0)["parked"] == k + 1)
            assert api.round_state(0)["launch_calls"] == before["launch_calls"], "a launch was made under the hold"
            api.round_hold(0, False)
            held = False
        finally:
            if held:
                api.round_hold(0, False)
            self.join()
        return since(before)


def since(before):
    after = api.round_state(0)
    assert (after["in_rounds"], after["parked"], after["holds"]) == (0, 0, 0), after
    made = after["launch_calls"] - before["launch_calls"]
    assert 0 <= made <= len(after["records"])
    return after["records"][len(after["records"]) - made:]


def steps_of(records, chunks):
    """the steps (None = the opening) of the member with `chunks` chunks, in launch order, with the members of each launch"""
    return [(r["round"][r["chunks"].index(chunks)], r["members"]) for r in records if chunks in r["chunks"]]


def expected_together(x, ref, names):
    """released together: in launch k (the opening, then round k - 1) every session with rounds >= k - 1 ... takes part"""
    want = []
    last = max(ref[n]["rounds"] for n in names)
    for step in [None] + list(range(last + 1)):
        members = [n for n in names if step is None or step <= ref[n]["rounds"]]
        want.append((step, sorted(x[n][0].n_chunks for n in members)))
    return want


def check_together(x, ref, names, records):
    got = [(r["round"][0] if len(set(r["round"])) == 1 else tuple(r["round"]), sorted(r["chunks"])) for r in records]
    assert got == expected_together(x, ref, names), (got, records)
    for r in records:
        assert r["merged"] == (r["members"] > 1), r
        for step, items in zip(r["round"], r["phmm_items"]):
            assert (items == 0) == (step is None), r       # phmm carried every member that was in a round, and no opening


@pytest.fixture
def one_lane(lib, alone, monkeypatch):
    monkeypatch.setenv("JTK_LC_LANES", "1")
    return alone


@pytest.mark.parametrize("lanes", ["1", "2"])
def test_three_sessions_released_together(lib, alone, monkeypatch, lanes):
    """case 1: all three are in every launch until the first converges; the survivors continue"""
    x, ref = alone
    monkeypatch.setenv("JTK_LC_LANES", lanes)
    names = ("A", "B", "C")
    # two lanes: A and C share lane 0, B has lane 1 to itself; lane 0's ledger shows A and C only
    g = Lane(x, names, [0, 0, 0] if lanes == "1" else [0, 1, 0])
    try:
        on_lane_0 = [0, 1, 2] if lanes == "1" else [0, 2]
        for p in range(2):
            if lanes == "2":
                g.start(1)   # B runs on its own lane meanwhile
            records = g.together(on_lane_0)
            check_together(x, ref, [names[i] for i in on_lane_0], records)
            for name, out, rc in zip(names, g.outs, g.rcs):
                assert rc == 0
                assert_same(out, ref[name]["out"], (name, "lanes " + lanes, "pass %d" % p))
    finally:
        g.close()


@pytest.mark.parametrize("late", ["A", "C"])
def test_members_in_different_rounds_in_one_launch(one_lane, late):
    """case 2: the early sessions take their opening by a step while `late` has not started; the next launch carries them in
    round 0 and `late` at its opening, and so on one round apart"""
    x, ref = one_lane
    names = ("A", "B", "C")
    early = [n for n in names if n != late]
    g = Lane(x, names)
    try:
        for p in range(2):
            before = api.round_state(0)
            api.round_hold(0, True)
            held = True
            try:
                for k, n in enumerate(early):
                    g.start(names.index(n))
                    g.wait((n, "parks"), lambda: api.round_state(0)["parked"] == k + 1)
                api.round_hold(0, "step")
                g.wait("the step's launch", lambda: api.round_state(0)["launch_calls"] == before["launch_calls"] + 1
                       and api.round_state(0)["parked"] == len(early))
                g.start(names.index(late))
                g.wait((late, "parks"), lambda: api.round_state(0)["parked"] == 3)
                api.round_hold(0, False)
                held = False
            finally:
                if held:
                    api.round_hold(0, False)
                g.join()
            records = since(before)
            assert records[0]["round"] == [None] * 2 and sorted(records[0]["chunks"]) == sorted(x[n][0].n_chunks for n in early)
            second = records[1]
            assert second["members"] == 3 and second["merged"], second
            by_chunks = dict(zip(second["chunks"], second["round"]))
            assert by_chunks == {x[n][0].n_chunks: (None if n == late else 0) for n in names}, second
            assert second["chunks"][2] == x[late][0].n_chunks              # arrival order is segment order
            for n in names:   # every member: the opening, then its rounds 0 .. R, each exactly once
                steps = [s for s, _ in steps_of(records, x[n][0].n_chunks)]
                assert steps == [None] + list(range(ref[n]["rounds"] + 1)), (n, steps)
            for name, out, rc in zip(names, g.outs, g.rcs):
                assert rc == 0
                assert_same(out, ref[name]["out"], (name, "late " + late, "pass %d" % p))
    finally:
        g.close()


def test_segments_that_differ(one_lane):
    """case 3: another max_tmpl / max_read, another pair-HMM, a chunk that fails in band_prep, a session that converges at once"""
    x, ref = one_lane
    names = ("LONG", "A", "MODEL", "BROKEN", "C")
    g = Lane(x, names)
    try:
        for p in range(2):
            records = g.together(range(5))
            check_together(x, ref, names, records)
            assert records[0]["members"] == 5 and records[1]["members"] == 5
            for name, out, rc in zip(names, g.outs, g.rcs):
                assert rc == ref[name]["rc"]
                assert_same(out, ref[name]["out"], (name, "pass %d" % p))
    finally:
        g.close()
    assert ref["BROKEN"]["rc"] != 0


def test_nine_sessions_launch_as_eight_and_one(one_lane):
    """case 4"""
    x, ref = one_lane
    names = ["one%d" % i for i in (3, 0, 8, 5, 1, 7, 2, 6, 4)]
    g = Lane(x, names)
    try:
        for p in range(2):
            records = g.together(range(9))
            assert [r["members"] for r in records[:4]] == [8, 1, 8, 1], records[:4]     # the opening and round 0
            assert records[0]["merged"] and not records[1]["merged"]
            assert records[0]["round"] == [None] * 8 and records[2]["round"] == [0] * 8
            carried = sum(r["members"] for r in records)
            assert carried == sum(ref[n]["rounds"] + 2 for n in names)
            for name, out, rc in zip(names, g.outs, g.rcs):
                assert rc == 0
                assert_same(out, ref[name]["out"], (name, "pass %d" % p))
    finally:
        g.close()


@pytest.mark.parametrize("names, n_gather, take_num", [(("B", "C", "PAIR", "WIDE"), 2, 0), (("B",), 1, 8)],
                         ids=["pair_wide_polish", "polish_take_num"])
def test_sessions_that_do_not_merge_run_beside_merging_ones(one_lane, names, n_gather, take_num):
    """case 5: a session with pair items, one with wide reads and a polish_chunks call on the lane while B and C are parked; the
    ledger shows B and C merged and nobody else.
    polish_take_num: two lane-mates, B and a polish_chunks call in which 8 of a pile-up's 12 reads vote (take_num) and whose
    product is the per-read tables' final pass (batch_needs_tables): its tables of one, with finalize_kernel beside them, are
    queued on the lane's stream while B is parked at the lane's gather.  Such a session has no gather and the ledger records
    none of its launches; what the ledger shows is that it joined nobody's table: every launch of the pass is B's alone
    (members 1, not merged, B's two chunks)."""
    x, ref = one_lane
    gathering = names[:n_gather]
    want_polish = api.polish_chunks(PARAMS, x["A"][0], take_num=take_num)
    n_cons, n_ops = int(want_polish["cons_off"][-1]), int(want_polish["ops_out_off"][-1])
    assert n_cons > 0 and n_ops > 0
    g = Lane(x, names)
    got = {}
    try:
        for p in range(2):
            before = api.round_state(0)
            api.round_hold(0, True)
            held = True
            try:
                for k in range(n_gather):
                    g.start(k)
                    g.wait((names[k], "parks"), lambda: api.round_state(0)["parked"] == k + 1)
                # polish-only: no gather at all, returns under the hold
                t = threading.Thread(target=lambda: got.update(out=api.polish_chunks(PARAMS, x["A"][0], take_num=take_num)))
                t.start()
                t.join(DEADLINE_SECONDS)
                assert not t.is_alive() and "out" in got, "the polish call waited for the round hold"
                for k in range(n_gather, len(names)):
                    g.start(k)   # (their chains wait for B and C, which are in their pass: they return after the release)
                st = api.round_state(0)
                assert st["parked"] == n_gather and st["launch_calls"] == before["launch_calls"], st
                api.round_hold(0, False)
                held = False
            finally:
                if held:
                    api.round_hold(0, False)
                g.join()
            records = since(before)
            check_together(x, ref, gathering, records)
            assert all(set(r["chunks"]) <= {2, 3} for r in records), records   # PAIR has 5 chunks, WIDE 6, the polish call 1
            if n_gather == 1:
                assert all(r["members"] == 1 and not r["merged"] and r["chunks"] == [2] for r in records), records
            for name, out, rc in zip(names, g.outs, g.rcs):
                assert rc == 0
                assert_same(out, ref[name]["out"], (name, "pass %d" % p))
            for k in ("cons_off", "ops_out_off", "result"):
                assert got["out"][k].tobytes() == want_polish[k].tobytes(), k
            assert got["out"]["cons"][:n_cons].tobytes() == want_polish["cons"][:n_cons].tobytes()
            assert got["out"]["ops_out"][:n_ops].tobytes() == want_polish["ops_out"][:n_ops].tobytes()
    finally:
        g.close()


def test_one_shot_call_in_three_slices(lib, alone, monkeypatch):
    """case 7: the one-shot call cut into three slices, against the resident session alone.  On one lane the call runs under a
    round hold until its three slices are parked: every launch from the opening to the round in which the first slice converges
    carries all three.  On three lanes every slice has a lane to itself and lane 0 shows single-session launches only."""
    x, ref = alone
    ps = [pile(800 + i, 6, 3e-2 if i % 3 == 0 else 1e-3) for i in range(9)]
    b = jb.pack(ps)
    with api.Session(PARAMS, b) as s:
        want, rc = one_pass(s)
    assert rc == 0
    # the call cuts 9 chunks into slices of 3; a slice is in the rounds 0 .. R of its slowest chunk
    last = [int(want["result"]["polish_rounds"][3 * k:3 * k + 3].max()) for k in range(3)]
    monkeypatch.setenv("JTK_LC_SLICES", "3")
    monkeypatch.setenv("JTK_LC_LANES", "1")
    for p in range(2):
        before = api.round_state(0)
        assert (before["in_rounds"], before["parked"], before["holds"]) == (0, 0, 0), before
        got, errors = {}, []

        def call():
            try:
                got["out"] = snapshot(api.cluster_chunks(PARAMS, b))
            except BaseException as e:  # noqa: BLE001 -- handed to the main thread
                errors.append(e)

        api.round_hold(0, True)
        held = True
        t = threading.Thread(target=call)
        try:
            t.start()
            until = time.monotonic() + DEADLINE_SECONDS
            while api.round_state(0)["parked"] < 3:
                assert not errors and t.is_alive() and time.monotonic() < until, (errors, api.round_state(0))
                time.sleep(0.0005)
            assert api.round_state(0)["launch_calls"] == before["launch_calls"], "a launch was made under the hold"
            api.round_hold(0, False)
            held = False
        finally:
            if held:
                api.round_hold(0, False)
            t.join(DEADLINE_SECONDS)
        assert not errors and not t.is_alive(), errors
        records = since(before)
        want_members = [3] + [sum(1 for r in last if step <= r) for step in range(max(last) + 1)]
        assert [r["members"] for r in records] == want_members, (records, last)
        assert [r["round"][0] for r in records] == [None] + list(range(max(last) + 1))
        for r in records:
            assert len(set(r["round"])) == 1 and r["chunks"] == [3] * r["members"] and r["merged"] == (r["members"] > 1), r
        assert records[0]["members"] == 3 and records[1]["members"] == 3 and records[1]["merged"]
        assert_same(got["out"], want, ("one-shot", "one lane", "pass %d" % p))
    monkeypatch.setenv("JTK_LC_LANES", "3")
    before = api.round_state(0)
    for p in range(2):
        out = snapshot(api.cluster_chunks(PARAMS, b))
        assert_same(out, want, ("one-shot", "three lanes", "pass %d" % p))
    records = since(before)
    assert records and all(r["members"] == 1 and not r["merged"] for r in records), records


def final_pass_inputs():
    """case 6: two pile-ups that take all 20 polish rounds (found with the CPU oracle among the generator's pile-ups 900 .. 939
    under this module's band fraction: 929 at 300 bp with a template error of 0.45, 927 at 420 bp with 0.3; every other one of
    those 240 converges in at most 19), each a session of its own, beside A, which converges in round 1"""
    f1 = jb.pack([pile(929, 6, 0.45), pile(804, 6)])
    f2 = jb.pack([pile(927, 6, 0.3, tmpl_len=420), pile(801, 6), pile(806, 6)])
    return {"F1": (f1, PARAMS), "F2": (f2, PARAMS)}


def test_a_final_pass_beside_sessions_that_converge_early(one_lane):
    """case 6: F1 and F2 are carried through round 20, the 21st and final pass of a session (final_pass = 1: select_edits only,
    no sum_final, rethread, commit or band_prep for that segment).  Pass 0: F1 runs one step ahead of A and F2, so one merged
    launch holds F1 in its final pass beside F2 in round 19 (a segment without width in four kernels beside one that has it).
    Pass 1: released together, F1 and F2 share the final pass."""
    x, ref = one_lane
    x = dict(x, **final_pass_inputs())
    names = ("F1", "A", "F2")
    final = {}
    for n in ("F1", "F2"):   # alone, outside the shared lane's gather: one session at a time
        with api.Session(x[n][1], x[n][0]) as s:
            out, rc = one_pass(s)
        assert rc == 0 and int(out["result"]["polish_rounds"].max()) == 20, (n, out["result"]["polish_rounds"])
        final[n] = out
    want = dict(F1=final["F1"], F2=final["F2"], A=ref["A"]["out"])
    chunks = {n: x[n][0].n_chunks for n in names}
    assert sorted(chunks.values()) == [1, 2, 3]
    g = Lane(x, names)
    try:
        # pass 0: F1 one step ahead
        before = api.round_state(0)
        api.round_hold(0, True)
        held = True
        try:
            g.start(0)
            g.wait("F1 parks", lambda: api.round_state(0)["parked"] == 1)
            api.round_hold(0, "step")
            g.wait("the step's launch", lambda: api.round_state(0)["launch_calls"] == before["launch_calls"] + 1
                   and api.round_state(0)["parked"] == 1)
            g.start(1)
            g.start(2)
            g.wait("A and F2 park", lambda: api.round_state(0)["parked"] == 3)
            api.round_hold(0, False)
            held = False
        finally:
            if held:
                api.round_hold(0, False)
            g.join()
        records = since(before)
        mixed = [r for r in records if r["merged"] and 20 in r["round"]]
        assert len(mixed) == 1, records
        by_chunks = dict(zip(mixed[0]["chunks"], mixed[0]["round"]))
        assert by_chunks == {chunks["F1"]: 20, chunks["F2"]: 19}, mixed
        assert [s for s, _ in steps_of(records, chunks["F1"])] == [None] + list(range(21))
        assert [s for s, _ in steps_of(records, chunks["F2"])] == [None] + list(range(21))
        assert [s for s, _ in steps_of(records, chunks["A"])] == [None, 0, 1]
        for name, out, rc in zip(names, g.outs, g.rcs):
            assert rc == 0
            assert_same(out, want[name], (name, "F1 one step ahead"))
        # pass 1: together
        records = g.together(range(3))
        assert [(r["round"][0], r["members"]) for r in records] == [(None, 3), (0, 3), (1, 3)] + [(k, 2) for k in range(2, 21)], records
        assert records[-1]["merged"] and records[-1]["round"] == [20, 20]
        for name, out, rc in zip(names, g.outs, g.rcs):
            assert rc == 0
            assert_same(out, want[name], (name, "released together"))
    finally:
        g.close()


def test_hold_and_state_refuse_what_does_not_exist(one_lane):
    with pytest.raises(ffi.JtkError) as e:
        api.round_hold(31, True)
    assert e.value.status == -1
    with pytest.raises(ffi.JtkError) as e:
        api.round_hold(0, False)     # a release without a hold
    assert e.value.status == -1
    with pytest.raises(ffi.JtkError):
        api.round_state(31)
    api.round_hold(0, "step")        # nobody parked: nothing happens
    st = api.round_state(0)
    assert (st["in_rounds"], st["parked"], st["holds"]) == (0, 0, 0)
