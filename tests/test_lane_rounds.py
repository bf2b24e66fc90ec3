"""jtk_amd/csrc/session_lanes.h, the round gather -- the rule by which the sessions of a lane put their polish rounds into one
launch -- compiled as plain C++ with a recording launch (tests/cpp/lane_rounds_main.cpp, a program with its own main) and run
as a program, once plain and once under ThreadSanitizer (-fsanitize=thread; should the toolchain not link it, or its runtime
refuse to start in the machine's address-space layout, under -fsanitize=address,undefined, and the test says which one ran).
The program checks every launch where it is made (at most 8 members, none twice, all of them parked, nobody in its rounds left
out unless a step asked for it) and the scenarios: 1, 2, 3, 8, 9 and 17 members that leave after different numbers of rounds;
the same numbers parked under a hold and released; a member that enters while others are parked, and a step that puts members
of different rounds into one launch; a member at its chain point while its mate still takes rounds, under a hold of the chain
gather; a member that returns early while its mate is parked; a release in a chosen arrival order under two holds."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jtk_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "cpp", "lane_rounds_main.cpp")


def _run(exe):
    return subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("lane_rounds")
    base = ["g++", "-std=c++17", "-Wall", "-Werror", "-g", "-O1", "-pthread", "-I", CSRC, MAIN, "-o"]
    plain = d / "rounds"
    subprocess.check_call(base + [str(plain)])
    exe = d / "rounds_san"
    sanitizer = "thread"
    if subprocess.run(base + [str(exe), "-fsanitize=thread"], stdout=subprocess.PIPE, stderr=subprocess.PIPE).returncode != 0:
        sanitizer = "address,undefined"
        subprocess.check_call(base + [str(exe), "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    run = _run(exe)
    if sanitizer == "thread" and run.returncode != 0 and b"unexpected memory mapping" in run.stderr:
        sanitizer = "address,undefined"
        subprocess.check_call(base + [str(exe), "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
        run = _run(exe)
    print("lane_rounds_main built with -fsanitize=" + sanitizer)
    return _run(plain), run, sanitizer


@pytest.mark.parametrize("which", ["plain", "sanitizer"])
def test_the_program_runs_clean(programs, which):
    run = programs[0] if which == "plain" else programs[1]
    out = run.stdout.decode()
    assert run.returncode == 0, (programs[2], out[-3000:], run.stderr.decode()[-3000:])
    assert run.stderr == b"", run.stderr.decode()[-3000:]   # (a sanitizer report that did not end the run)
    assert "FAIL " not in out and "FAILURES 0" in out
    for mark in ("STEP ok", "CHAIN ok", "WITHDRAW ok", "ORDER ok"):
        assert mark in out


def test_held_members_launch_in_groups_of_eight(programs):
    out = programs[1].stdout.decode().splitlines()
    held = {int(l.split()[1]): [int(x) for x in l.split()[2:]] for l in out if l.startswith("HELD ")}
    assert held == {1: [1], 2: [2], 3: [3], 8: [8], 9: [8, 1], 17: [8, 8, 1]}


def test_every_arrival_is_launched_once(programs):
    """members i = 0 .. n-1 take the opening and 1 + 3i mod 7 rounds: the launches carry exactly that many arrivals, in no more
    calls than arrivals and no fewer than the longest member's"""
    out = programs[1].stdout.decode().splitlines()
    got = {int(l.split()[1]): (int(l.split()[3]), int(l.split()[5])) for l in out if l.startswith("LENGTHS ")}
    assert sorted(got) == [1, 2, 3, 8, 9, 17]
    for n, (arrivals, launches) in got.items():
        lengths = [2 + (3 * i) % 7 for i in range(n)]
        assert arrivals == sum(lengths)
        assert max(lengths) <= launches <= arrivals
