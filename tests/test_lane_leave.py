"""jtk_amd/csrc/session_lanes.h, leaving a merged chain launch -- the host pieces by which a session of a lane goes on when ITS
chunks of the lane's merged chain launch are done: which of the lane's two streams carries rounds (lane_round_stream), the
merged launches in view and where the general chain goes (LaneFlow), who may leave through its word (lane_member_may_leave),
the guard that takes a member out of its launch on every path (LaneFlightLeave), the host's side of the never-reset completion
counter (ChainDone) and the wait itself (lane_leave_wait: the word first, the launch's
end event second, an error if neither).  Compiled as plain C++ (tests/cpp/lane_leave_main.cpp, a program with its own main) and
run as a program, once plain and once under -fsanitize=address,undefined.  The program checks

 * the stream choice with the in-flight state given: a light chain in flight on either stream, both idle, and -- through a
   lane whose queues are mock but whose decisions are the functions session.hip calls -- a general chain still running on the
   stream a leaving member is sent to; over
   five passes from either starting stream the light chain follows the rounds, nothing is ever queued behind it, lane-mates
   released later join the first one's stream, and a launch of one member flips nothing;
 * who may leave: not a member with nothing of its own in the merged kernels, without a pinned page, or with chunks of the
   global-memory class, whose kernel is queued behind the launch -- such a member keeps its stream, its fetch lands behind
   that kernel, and it counts as in the launch until then; two members that come round and merge while the third still
   waits in the launch before, one of them in its next rounds when the third leaves: the round stream moves at a merged
   launch only, so whoever parks at one gather is on one stream (checked at every start of a pass); the guard;
 * the target over consecutive launches with different segment sets (one class in both kernels, two classes, one kernel, a
   single workgroup, a pass that launches nothing), from 0 and from just below 2^32: exactly one workgroup reports, the last;
 * the order of the fallback, by counting the looks at the word, at the event and the pauses."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jtk_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "cpp", "lane_leave_main.cpp")
MARKS = ("CHOICE ok", "PASSES ok", "ELIGIBLE ok", "FLIGHTS ok", "TARGETS ok from 0", "TARGETS ok from 4294967280", "IDS ok", "FALLBACK ok")


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("lane_leave")
    base = ["g++", "-std=c++17", "-Wall", "-Werror", "-g", "-O1", "-pthread", "-I", CSRC, MAIN, "-o"]
    subprocess.check_call(base + [str(d / "leave")])
    subprocess.check_call(base + [str(d / "leave_san"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    return {k: subprocess.run([str(d / exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
            for k, exe in (("plain", "leave"), ("sanitizer", "leave_san"))}


@pytest.mark.parametrize("which", ["plain", "sanitizer"])
def test_the_program_runs_clean(programs, which):
    run = programs[which]
    out = run.stdout.decode()
    assert run.returncode == 0, (out[-3000:], run.stderr.decode()[-3000:])
    assert run.stderr == b"", run.stderr.decode()[-3000:]   # (a sanitizer report that did not end the run)
    assert "FAIL " not in out and "FAILURES 0" in out
    for mark in MARKS:
        assert mark in out
