"""jtk_amd/csrc/kmer_plan.h compiled as plain C++ (no HIP, no GPU) with AddressSanitizer and UBSan: the tile table and the k-mer
offsets that mask.hip and map.hip hand to their kernels, and the bit length their sort keys are sized by, against a restatement
written here from the rules: a sequence of `len` bases has max(len - k + 1, 0) k-mer positions; its tiles start at the multiples
of `tile` below len (mask: a tile counts bases, and a read shorter than k is still copied) or below its k-mer positions (map);
the tiles of a sequence are adjacent and ascending, the sequences in their order.  Everything the program prints is compared
exactly."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jtk_amd", "csrc")

PROGRAM = r'''
#include <inttypes.h>
#include <stdio.h>
#include <iostream>
#include <string>
#include "kmer_plan.h"

template <class T> static void row(const char *tag, const std::vector<T> &v) {
    printf("%s", tag);
    for (auto x : v) printf(" %" PRIu64, (uint64_t)x);
    printf("\n");
}
int main() {
    std::string what;
    while (std::cin >> what) {
        if (what == "BITS") {
            uint64_t v;
            std::cin >> v;
            printf("BITS %" PRIu64 " %u\n", v, jtk_bits(v));
            continue;
        }
        std::string name;
        uint32_t k, tile;
        int unit;
        size_t n;
        std::cin >> name >> k >> tile >> unit >> n;
        std::vector<uint64_t> off(n + 1, 0);   // exactly n + 1 entries: a read past them is the sanitizer's to find
        for (size_t r = 0; r < n; r++) {
            uint64_t len;
            std::cin >> len;
            off[r + 1] = off[r] + len;
        }
        const KmerPlan P = jtk_plan_kmers(n, off.data(), k, tile, unit ? KMER_TILE_POSITIONS : KMER_TILE_BASES);
        printf("CASE %s\n", name.c_str());
        row("KOFF", P.kmer_off);
        row("NK", std::vector<uint64_t>{P.n_kmers});
        row("TSEQ", P.tile_seq);
        row("TSTART", P.tile_start);
    }
    return 0;
}
'''

BASES, POSITIONS = 0, 1
BITS_AT = (0, 1, 2, 3, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 63, 2 ** 64 - 1)


def lengths(k, tile):
    return [0, k - 1, k, k + 1, tile - 1, tile, tile + 1, tile + k - 2, tile + k - 1, tile + k, 2 * tile + k]


def cases():
    out = {}
    for k in (1, 12, 31):
        for tile in (1024, 2048):
            for unit in (BASES, POSITIONS):
                tag = "k%d_t%d_u%d" % (k, tile, unit)
                out[tag + "_mixed"] = (k, tile, unit, lengths(k, tile))
                out[tag + "_empty"] = (k, tile, unit, [])
                for i, n in enumerate(lengths(k, tile)):
                    out["%s_alone%d" % (tag, i)] = (k, tile, unit, [n])
    return out


CASES = cases()


def expected(k, tile, unit, lens):
    kmer_off, tile_seq, tile_start = [0], [], []
    for r, n in enumerate(lens):
        n_pos = max(n - k + 1, 0)
        kmer_off.append(kmer_off[-1] + n_pos)
        for s in range(0, n if unit == BASES else n_pos, tile):
            tile_seq.append(r)
            tile_start.append(s)
    return dict(KOFF=kmer_off, NK=[kmer_off[-1]], TSEQ=tile_seq, TSTART=tile_start)


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("kmer_plan")
    src, exe = tmp / "plan.cpp", tmp / "plan"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-I", CSRC,
                           str(src), "-o", str(exe)])
    stdin = "".join("PLAN %s %d %d %d %d %s\n" % (name, k, tile, unit, len(lens), " ".join(map(str, lens))) for name, (k, tile, unit, lens) in CASES.items())
    stdin += "".join("BITS %d\n" % v for v in BITS_AT)
    run = subprocess.run([str(exe)], input=stdin.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert run.returncode == 0, run.stderr.decode()[-4000:]
    assert run.stderr == b"", run.stderr.decode()[-4000:]   # (a sanitizer report that did not end the run)
    got, bits, cur = {}, {}, None
    for line in run.stdout.decode().splitlines():
        tag, *rest = line.split()
        if tag == "CASE":
            cur = got.setdefault(rest[0], {})
        elif tag == "BITS":
            bits[int(rest[0])] = int(rest[1])
        else:
            cur[tag] = [int(x) for x in rest]
    return got, bits


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_plan_equals_the_restatement(name, program_output):
    assert program_output[0][name] == expected(*CASES[name])


def test_every_case_came_back(program_output):
    assert sorted(program_output[0]) == sorted(CASES) and len(CASES) == 3 * 2 * 2 * 13


def test_the_two_tile_kinds_differ_where_they_should():
    """a read shorter than k: tiles of bases (the mask copies it), none of positions; TILE + k - 1 bases are one tile of positions
    and two of bases; an empty read has no tile of either kind"""
    k, tile = 12, 2048
    assert expected(k, tile, BASES, [k - 1])["TSTART"] == [0] and expected(k, tile, POSITIONS, [k - 1])["TSTART"] == []
    assert expected(k, tile, BASES, [tile + k - 1])["TSTART"] == [0, tile] and expected(k, tile, POSITIONS, [tile + k - 1])["TSTART"] == [0]
    assert expected(k, tile, POSITIONS, [tile + k])["TSTART"] == [0, tile]
    assert expected(k, tile, BASES, [0, 5])["TSEQ"] == [1] and expected(k, tile, POSITIONS, [0])["TSEQ"] == []


def test_bit_lengths(program_output):
    assert program_output[1] == {v: max(v.bit_length(), 1) for v in BITS_AT}
    assert [program_output[1][v] for v in BITS_AT] == [1, 1, 2, 2, 31, 32, 32, 64, 64]
