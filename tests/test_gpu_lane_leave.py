"""A session leaves a merged chain launch when its own chunks end (jtk_amd/csrc/session_lanes.h, "Leaving a merged chain
launch"; session.hip: run_batch, launch_lane_chains; mcmc_kernels.hip: the count at the end of mcmc_segment_body).

The merge is made certain with the chain hold of include/jtk_lc_debug.h, as tests/test_gpu_lane_segments.py does: with
JTK_LC_LANES=1 every session shares lane 0, the test holds it, starts one thread per session, waits until all pend, and
releases.  What happened is then read from the sessions' pass ledgers (api.Session.passes) and the lane's launch ledger --
never from the clock: how a pass ended (its word, or the launch's end event), whether that event was still pending, how many
lane-mates were still waiting, which of the lane's two streams carries its next rounds, and order stamps from one counter.

Sessions (300 bp templates; every session has one chunk without any variant, whose workgroups exit at once and must be counted):
 A  two diploid pile-ups of 12 reads with one variant column: chains of 20 x 2000 x 12 proposals.  The smallest that have a
    chain at all: the variant filter keeps no column of a pile-up of 8 or 10 reads (the CPU oracle, 6 pile-ups each at read
    error rates of 0.1 % and 3 %, divergences from 5e-4 to 2e-2 and haploid coverages from 1 to 16: n_variants = 0 in every
    one, so such a chunk is a third chunk without a variant), and from 12 reads on it keeps one in a third of them.
 B  one diploid pile-up of 60 reads: 20 x 2000 x 60 proposals per chain, five times A's by construction.
 E  a three-copy pile-up of 18 reads, generated with three or more planted differences, of which the filter keeps two columns
    (the fixture prints them) -- copy number 3 is the general kernel's whatever the columns:
    chains for k = 2 and k = 3 of 20 x 2000 x 18 proposals each -- next to A's two pile-ups (the light kernel's).
 B2 B's kind with 120 reads, E's lane-mate: twice B's chain.  E's LIGHT chunks are A's, which leave long before a 60-read chain
    ends; its general chunk runs longer than B2's chain (alone E takes 0.70 s a pass, B2 0.39 s: the one-proposal-per-iteration
    chain of a three-copy pile-up).

 (a) labels, posterior bits, scores, cluster counts, consensus and ops of A and B equal the same sessions run alone;
 (b) A left through its word while the launch's end event was pending and B was still waiting; B left with the launch (nobody
     was waiting any more);
 (c) A's fetch, and round 0 of A's next pass (which the opening of that pass precedes), completed before B's run returned;
 (d) a second pass of both gives the same outputs: the counter's target carried over;
 (e) E merged with B2, on its FIRST pass -- its label buffers have never been written: B2 leaves through its word while E still
     waits, although E's light chunks ended long before (case (b)); E leaves last, and its outputs equal E alone: it left only
     when the light and the general kernel had both counted it.
"""
import os
import threading
import time

import pytest

from jtk_amd import api, batch as jb, synth
from test_gpu_lanes import assert_same, diploid, no_variant, snapshot

pytestmark = [pytest.mark.gpu, pytest.mark.changes_env]

DEADLINE_SECONDS = 60.0   # a safety cap for a gather, no performance claim


def params(coverage):
    return jb.default_params(haploid_coverage=coverage, band_frac=synth.CONFIGS["ont_diploid"]["band_frac"])


def three_copies_of_six(chunk_id):
    cfg = dict(synth.CONFIGS["ont_4copy"], tmpl_len=300, n_haps=3, copy_num=3, reads_per_hap=6, divergence=4e-2)
    return synth.make_pileup(chunk_id, cfg, min_variants=3)


def inputs():
    """name -> (batch, params); the chunk without a variant is the last one of each"""
    return dict(A=(jb.pack([diploid(812, 6), diploid(816, 6), no_variant(860)]), params(6.0)),
                B=(jb.pack([diploid(820, 30), no_variant(861)]), params(30.0)),
                B2=(jb.pack([diploid(821, 60), no_variant(863)]), params(60.0)),
                E=(jb.pack([three_copies_of_six(832), diploid(812, 6), diploid(816, 6), no_variant(862)]), params(6.0)))


@pytest.fixture(scope="module")
def lib(jtk_lib):
    assert jtk_lib.jtk_lc_device_ok(0) == 1, "needs a gfx950 device"
    return jtk_lib


@pytest.fixture(scope="module")
def alone(lib):
    """every session alone, JTK_LC_LANES unset, two passes: name -> (first pass, seconds of one run)"""
    assert "JTK_LC_LANES" not in os.environ
    x, ref = inputs(), {}
    for name, (b, p) in x.items():
        with api.Session(p, b) as s:
            t0 = time.perf_counter()
            s.run()
            seconds = time.perf_counter() - t0
            first = snapshot(s.fetch())
            s.run()
            second = snapshot(s.fetch())
            passes = s.passes()
        assert_same(second, first, (name, "second pass alone"))
        # alone, a pass ends with its own launch's event and flips nothing
        assert [(q["how"], q["members"], q["still_waiting"]) for q in passes] == [("event", 1, 0)] * 2, passes
        assert all(q["round_stream"] == q["next_round_stream"] == passes[0]["round_stream"] for q in passes), passes
        r = first["result"]
        print("ALONE %s %.3f s  n_variants %s  k %s" % (name, seconds, r["n_variants"].tolist(), r["cluster_num"].tolist()))
        assert (r["status"] == 0).all(), name
        assert int(r["n_variants"][-1]) == 0 and (r["n_variants"][:-1] > 0).all(), (name, r["n_variants"])
        ref[name] = (first, seconds)
    ra, re = ref["A"][0]["result"], ref["E"][0]["result"]
    assert (ra["n_variants"][:2] <= 2).all() and (re["n_variants"][1:3] <= 2).all()   # the light kernel's chunks
    assert int(x["E"][0].chunks["copy_num"][0]) == 3 and int(re["n_variants"][0]) > 0     # the general kernel's
    return x, ref


def two_sessions_held(x, first_name, second_name, passes):
    """`passes` passes (run + fetch) of two sessions of lane 0, the first pass of both held into one merged launch; returns
    (outputs per session per pass, pass ledgers, the lane's launch records of the first release)"""
    names = (first_name, second_name)
    sessions = [api.Session(x[n][1], x[n][0]) for n in names]
    outs, errors = [[], []], []
    try:
        assert {s.lane() for s in sessions} == {0}
        before = api.lane_state(0)
        assert (before["in_pass"], before["pending"], before["holds"]) == (0, 0, 0), before

        def work(i):
            try:
                for _ in range(passes):
                    sessions[i].run()
                    outs[i].append(snapshot(sessions[i].fetch()))
            except BaseException as e:  # noqa: BLE001 -- handed to the main thread
                errors.append((names[i], e))

        threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        api.lane_hold(0, True)
        held = True
        try:
            until = time.monotonic() + DEADLINE_SECONDS
            for k, t in enumerate(threads):
                t.start()
                while api.lane_state(0)["pending"] != k + 1:
                    assert not errors, errors
                    assert t.is_alive() and time.monotonic() < until, (names[k], "did not arrive", api.lane_state(0))
                    time.sleep(0.0005)
            api.lane_hold(0, False)
            held = False
        finally:
            if held:
                api.lane_hold(0, False)
            for t in threads:
                t.join(DEADLINE_SECONDS)
        assert not errors, errors
        assert not any(t.is_alive() for t in threads)
        after = api.lane_state(0)
        made = after["launch_calls"] - before["launch_calls"]
        records = after["records"][len(after["records"]) - made:]
        return outs, [s.passes() for s in sessions], records
    finally:
        for s in sessions:
            s.close()


@pytest.fixture
def one_lane(lib, alone, monkeypatch):
    monkeypatch.setenv("JTK_LC_LANES", "1")
    return alone


def test_the_short_session_leaves_while_the_long_one_runs(one_lane):
    """(a) - (d)"""
    x, ref = one_lane
    outs, ledgers, records = two_sessions_held(x, "A", "B", passes=2)
    print("LEDGER A", ledgers[0])
    print("LEDGER B", ledgers[1])
    print("LAUNCHES", records)
    # the first release made ONE launch of both: A's three chunks and B's two in class 0
    assert records[0]["members"] == 2 and records[0]["seg_chunks"][0] == [3, 2], records
    # (a), (d)
    for name, per_pass in zip("AB", outs):
        for k, out in enumerate(per_pass):
            assert_same(out, ref[name][0], (name, "pass %d in the merged launch against alone" % (k + 1)))
    a1, a2 = ledgers[0]
    b1, b2 = ledgers[1]
    assert (a1["pass_"], a2["pass_"], b1["pass_"], b2["pass_"]) == (1, 2, 1, 2)
    # (b)
    assert a1["how"] == "word" and a1["event_pending"] and (a1["members"], a1["still_waiting"]) == (2, 1), a1
    assert (b1["members"], b1["still_waiting"]) == (2, 0) and b1["how"] in ("word", "event"), b1
    assert a1["stamp_left"] < b1["stamp_left"]
    # the stream rule: the merged light chain ran on the round stream of pass 1, A's fetch and next rounds went to the other
    assert a1["round_stream"] == b1["round_stream"] and a1["next_round_stream"] == 1 - a1["round_stream"], (a1, b1)
    assert a2["round_stream"] == a1["next_round_stream"] and b1["next_round_stream"] == a1["next_round_stream"], (a2, b1)
    # (c)
    assert 0 < a1["stamp_fetched"] < b1["stamp_returned"], (a1, b1)
    assert 0 < a2["stamp_round0"] < b1["stamp_returned"], (a2, b1)


def test_a_session_with_a_general_chunk_leaves_when_both_kernels_have_counted_it(one_lane):
    """(e)"""
    x, ref = one_lane
    outs, ledgers, records = two_sessions_held(x, "E", "B2", passes=1)
    print("LEDGER E", ledgers[0])
    print("LEDGER B2", ledgers[1])
    assert records[0]["members"] == 2 and records[0]["seg_chunks"][0] == [4, 2], records
    assert_same(outs[0][0], ref["E"][0], "E in the merged launch against alone")
    assert_same(outs[1][0], ref["B2"][0], "B2 in the merged launch against alone")
    e1, b1 = ledgers[0][0], ledgers[1][0]
    assert b1["how"] == "word" and b1["event_pending"] and (b1["members"], b1["still_waiting"]) == (2, 1), b1
    assert (e1["members"], e1["still_waiting"]) == (2, 0) and e1["how"] in ("word", "event"), e1
    assert b1["stamp_left"] < e1["stamp_left"]
