"""jtk_amd/csrc/chain_layout.h compiled as plain C++ (no HIP): the chain's work area is ONE list of arrays, which the device's
carve and the host's sizes both expand.  The sizes the header computes -- mcmc_lds_bytes (what the session sorts chunks into
launch classes by), mcmc_ws_bytes (a chunk's slice of the global workspace) and the fixed head in front of the sized arrays --
against a restatement, written here, of the hand-written sum the host carried before the list existed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jtk_amd", "csrc")

NS = (1, 63, 64, 127, 128, 255, 256, 1023)
DS = (1, 2, 8, 9, 21)
KS = (0, 1, 2, 4, 7, 9)

PROGRAM = r'''
#include <stdio.h>
#include "batch_types.h"
#include "chain_layout.h"
#define PRINT_FIXED(member, type, bytes) printf("F %s\n", #member);
#define PRINT_SIZED(member, type, bytes) printf("S %s\n", #member);
int main() {
    JTK_CHAIN_FIXED_ARRAYS(PRINT_FIXED)
    JTK_CHAIN_SIZED_ARRAYS(PRINT_SIZED)
    printf("H %zu\n", mcmc_lds_fixed());
    const unsigned ns[] = {@NS}, ds[] = {@DS}, ks[] = {@KS};
    for (unsigned n : ns)
        for (unsigned d : ds)
            for (unsigned k : ks) printf("G %u %u %u %zu %zu\n", n, d, k, mcmc_lds_bytes(n, d, k), mcmc_ws_bytes(n, d, k));
    return 0;
}
'''.replace("@NS", ", ".join(map(str, NS))).replace("@DS", ", ".join(map(str, DS))).replace("@KS", ", ".join(map(str, KS)))


def al(b):
    return (b + 15) & ~15


def expected(n, d, k):
    """(fixed head, LDS bytes, workspace bytes): the 16-byte-rounded sum the host spelt out by hand"""
    rn = 128 << 4
    k = min(max(k, 2), 7)
    npad = (n + 63) & ~63
    fixed = al(32) + al(8 * rn) + al(4 * rn) + al(24 * 8)
    total = (fixed + al(8 * n * d) + 2 * al(8 * (n + 1)) + 2 * al(8 * 7 * d) + 5 * al(n) + 3 * al(d) + al(8 * k * npad) + al(4 * npad)
             + al(32 * k) + al(16 * d * k) + al(16 * d))
    return fixed, total, (total - fixed + 255) & ~255


def test_chain_layout_sizes_follow_from_one_list_of_arrays(tmp_path):
    src = tmp_path / "layout.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "layout"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])  # JTK_MAX_COPY: batch_types.h
    rows = [line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines()]
    fixed_names = [r[1] for r in rows if r[0] == "F"]
    sized_names = [r[1] for r in rows if r[0] == "S"]
    assert fixed_names == ["ctl", "ring", "rec", "k2_stats"]
    assert len(sized_names) == 18
    assert len(set(fixed_names + sized_names)) == 4 + 18       # no member twice
    (head,) = [int(r[1]) for r in rows if r[0] == "H"]
    got = {(int(r[1]), int(r[2]), int(r[3])): (int(r[4]), int(r[5])) for r in rows if r[0] == "G"}
    assert sorted(got) == sorted((n, d, k) for n in NS for d in DS for k in KS)
    want = {p: expected(*p) for p in got}
    assert {f for f, _, _ in want.values()} == {head}
    for p in sorted(got):
        assert got[p] == want[p][1:], p
    # the grid has points on both sides of the launch-class boundaries the session uses (80 KiB: two workgroups per CU; 160 KiB:
    # LDS or the global workspace) -- asked of the restatement, so the grid cannot silently miss them
    lds = [t for _, t, _ in want.values()]
    for bound in (80 * 1024, 160 * 1024):
        assert any(t <= bound for t in lds) and any(t > bound for t in lds)
