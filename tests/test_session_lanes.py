"""jtk_amd/csrc/session_lanes.h -- the lane table and the rule that gathers the chain launches of a lane's sessions -- compiled
as plain C++ with mock streams and a recording launch (tests/cpp/session_lanes_main.cpp, a program with its own main) and run
as a program.  Built with ThreadSanitizer (-fsanitize=thread), which the toolchain here links; should a toolchain not link it (or
its runtime refuse to start in the machine's address-space layout), the fallback is -fsanitize=address,undefined, and the test
says which one ran.  The program checks the threaded scenarios itself
(three sessions x four passes from three threads with seeded delays: every arrival launched exactly once, no launch while a
lane-mate is before its chain point, at most 8 members per launch; nine sessions: launches of 8 and 1; a session that leaves
through a failure path; a lone session launches from its own thread; a lane held by an outsider while 1, 3, 8, 9 and 17 members
arrive, a member that withdraws under the hold, a second hold taken while members pend) and prints the lane plans and assignments, which are
compared here with a restatement of the rules."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jtk_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "cpp", "session_lanes_main.cpp")
PAIRED = True       # JTK_LANE_FEW_QUEUES_PAIRED: below 8 queues, Q / 2 lanes with a side stream each
MAX_LANES = 32


def plan(q):
    if q >= 8:
        lanes, side = (q - 4) // 2, 1
    elif PAIRED:
        lanes, side = max(1, q // 2), int(q >= 2)
    else:
        lanes, side = max(1, q - 1), 0
    return min(lanes, MAX_LANES), side


def assign(max_lanes, live, made):
    """least loaded of the first max_lanes lanes, lowest index on a tie; a new lane only when all are taken and there is room"""
    have = min(made, max_lanes)
    best = min(range(have), key=lambda i: (live[i], i)) if have else None
    if (best is None or live[best] > 0) and made < max_lanes:
        best, made = made, made + 1
    live[best] += 1
    return best, made


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("session_lanes") / "lanes"
    base = ["g++", "-std=c++17", "-Wall", "-Werror", "-g", "-O1", "-pthread", "-I", CSRC, MAIN, "-o", str(exe)]
    sanitizer = "thread"
    if subprocess.run(base + ["-fsanitize=thread"], stdout=subprocess.PIPE, stderr=subprocess.PIPE).returncode != 0:
        sanitizer = "address,undefined"
        subprocess.check_call(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    if sanitizer == "thread" and run.returncode != 0 and b"unexpected memory mapping" in run.stderr:
        # the ThreadSanitizer runtime could not lay out its shadow memory in this address space (it never ran the program)
        sanitizer = "address,undefined"
        subprocess.check_call(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
        run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    print("session_lanes_main built with -fsanitize=" + sanitizer)
    return run, sanitizer


def test_the_program_runs_clean_under_the_sanitizer(program):
    run, sanitizer = program
    out = run.stdout.decode()
    assert run.returncode == 0, (sanitizer, out[-3000:], run.stderr.decode()[-3000:])
    assert run.stderr == b"", run.stderr.decode()[-3000:]   # (a sanitizer report that did not end the run)
    assert "FAIL " not in out and "FAILURES 0" in out
    assert "NINE 8 1" in out and "WITHDRAW ok" in out and "LONE 3" in out
    line = next(l for l in out.splitlines() if l.startswith("THREE_BY_FOUR")).split()
    assert int(line[4]) == 12 and 4 <= int(line[2]) <= 12   # 12 arrivals; between one launch per pass and one per arrival


def test_a_held_lane_gathers_every_arrival(program):
    """an outsider's enter() / withdraw() around N arrivals from N threads (the program asserts pending == N with no launch made,
    the members of each launch in arrival order, and the ring of member counts): one launch of the first min(N, 8), then the rest"""
    out = program[0].stdout.decode().splitlines()
    held = {int(l.split()[1]): [int(x) for x in l.split()[2:]] for l in out if l.startswith("HELD ")}
    assert held == {1: [1], 3: [3], 8: [8], 9: [8, 1], 17: [8, 8, 1]}
    assert "HELD_WITHDRAW ok" in out and "SECOND_HOLD ok" in out


def test_lane_plans(program):
    out = program[0].stdout.decode().splitlines()
    got = {int(l.split()[1]): (int(l.split()[2]), int(l.split()[3])) for l in out if l.startswith("PLAN ")}
    assert sorted(got) == [1, 2, 3, 4, 6, 7, 8, 9, 12, 16, 32, 100]
    for q, v in got.items():
        assert v == plan(q), q
    # one lane with a side stream per session while sessions <= (Q - 4) / 2: the four slices of a one-shot call at the
    # library's own 12 queues, the benchmark's six at its 16
    assert got[12] == (4, 1) and got[16] == (6, 1)
    forced = next(l for l in out if l.startswith("FORCED ")).split()[1:]
    assert [int(x) for x in forced] == [3, 0, 1, 1, 2, 1]   # (Q 4, lanes 3, side 0), (Q 12, lanes 1), (Q 4, side 1)


@pytest.mark.parametrize("q", [1, 4, 8, 12])
def test_assignment_is_least_loaded_and_stable(program, q):
    line = next(l for l in program[0].stdout.decode().splitlines() if l.startswith("ASSIGN %d " % q))
    first, second, tail = [part.split() for part in line[len("ASSIGN %d " % q):].split("|")]
    max_lanes = plan(q)[0]
    live, made, want = [0] * MAX_LANES, 0, []
    for _ in range(10):
        lane, made = assign(max_lanes, live, made)
        want.append(lane)
    assert [int(x) for x in first] == want
    if q >= 8:   # sessions <= lanes: a lane each, in order
        assert want[:max_lanes] == list(range(max_lanes))
    live[want[1]] -= 1
    live[want[4]] -= 1
    again = []
    for _ in range(2):
        lane, made = assign(max_lanes, live, made)
        again.append(lane)
    assert [int(x) for x in second] == again
    assert int(tail[1]) == made == min(max_lanes, 10)
