"""Diagnostic (GPU box): the two figures of DESIGN section 5, "Settle" -- (1) the HIP-event kernel time of one
jtk_lc_settle_nodes call (mode BY_CHUNK_POS) on 10,000 synthetic reads of 40 nodes of about 2,000 ops, a few of them duplicates
and contained nodes, after three warm-up calls, over 20 calls: median and spread, with the time of the whole call on its stream
and the host clock beside it; tests/settle_reference.py runs on every 50th read, is compared with the device's answer for those
reads, and its time is reported scaled by 50 -- a sanity figure, not a baseline.  (2) The wall time of dataset.correct_deletion
on the fixture of tests/deletion_fixture.py split by primitive (one warm-up run, then the median of five), with the time
of tests/deletion_reference.py on the same fixture.
`python scripts/settle_timing.py [--reads N] [--nodes N] [--out profiles/settle_timing.txt]`"""
import argparse
import copy
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import settle_cases as K  # noqa: E402
import settle_reference as R  # noqa: E402
from jtk_amd import api, dataset, ffi  # noqa: E402


def read_set(n_reads, n_nodes, seed):
    rng = random.Random(seed)
    reads = []
    for _ in range(n_reads):
        nodes, pos = [], rng.randrange(0, 2000)
        for k in range(n_nodes):
            cigar = []
            for _ in range(rng.randrange(3, 9)):
                cigar.append(("M", rng.randrange(150, 400)))
                cigar.append((rng.choice("ID"), rng.randrange(1, 6)))
            cigar.append(("M", rng.randrange(150, 400)))
            node = K.N(rng.randrange(0, 2500), pos, cigar, fwd=rng.random() < 0.5)
            nodes.append(node)
            if rng.random() < 0.05:      # a second encoding of the same chunk, or a short node inside this one
                nodes.append(K.N(node["chunk"] if rng.random() < 0.5 else 2500 + k, pos + rng.randrange(0, 40),
                                 [("M", node["qlen"] // 2)], fwd=node["fwd"]))
            pos += node["qlen"] + rng.randrange(-30, 400)
        rng.shuffle(nodes)               # as after the append of :344
        reads.append(nodes[:n_nodes])
    return reads


def flatten(reads):
    node_off = np.zeros(len(reads) + 1, dtype=np.uint64)
    node_off[1:] = np.cumsum([len(r) for r in reads])
    flat = [n for r in reads for n in r]
    nodes = np.array([(n["chunk"], n["pos"], 1 if n["fwd"] else 0, n["qlen"]) for n in flat], dtype=ffi.SETTLE_NODE_DT)
    code = {"M": 0, "I": 2, "D": 3}
    runs = [(code[op], l) for n in flat for op, l in n["cigar"]]
    ops = np.repeat(np.array([c for c, _ in runs], dtype=np.uint8), np.array([l for _, l in runs], dtype=np.int64))
    ops_off = np.zeros(len(flat) + 1, dtype=np.uint64)
    ops_off[1:] = np.cumsum([sum(l for _, l in n["cigar"]) for n in flat])
    return node_off, nodes, ops, ops_off


def spread(xs):
    return "median %.3f min %.3f max %.3f" % (statistics.median(xs), min(xs), max(xs))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--nodes", type=int, default=40)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--sample", type=int, default=50)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if ffi.lib().jtk_lc_device_ok(0) != 1:
        sys.exit("no gfx950 device: nothing is measured here")
    lines = []
    reads = read_set(args.reads, args.nodes, 5)
    arrays = flatten(reads)
    lines.append("settle_nodes: %d reads, %d nodes, %d ops (%.1f MB of ops)" % (len(reads), len(arrays[1]), len(arrays[2]), len(arrays[2]) / 1e6))
    for _ in range(3):
        out = api.settle_nodes(*arrays)
    kernel, call, host = [], [], []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        out = api.settle_nodes(*arrays)
        host.append((time.perf_counter() - t0) * 1e3)
        t = api.settle_timing()
        kernel.append(t["kernel_ms"])
        call.append(t["call_ms"])
    lines.append("kernel ms (HIP events, %d calls after 3 warm-up calls): %s" % (args.calls, spread(kernel)))
    lines.append("whole call on its stream ms (upload to last copy back): %s" % spread(call))
    lines.append("host clock around api.settle_nodes ms (with the Python packing of the results): %s" % spread(host))
    lines.append("nodes kept: %d of %d" % (int(out["n_kept"].sum()), len(arrays[1])))
    sample = list(range(0, len(reads), args.sample))
    t0 = time.perf_counter()
    want = R.settle([reads[r] for r in sample], R.BY_CHUNK_POS)
    ref_s = time.perf_counter() - t0
    assert [out["order"][r].tolist() for r in sample] == want["order"], "the device and the reference differ"
    lines.append("tests/settle_reference.py on every %dth read: %.3f s, x %d = %.1f s for all (the same answer as the device)"
                 % (args.sample, ref_s, args.sample, ref_s * args.sample))
    # ---- the fixture stage by primitive
    import deletion_fixture  # noqa: E402
    import deletion_reference as DR  # noqa: E402
    fixture = deletion_fixture.fixture()
    dataset.correct_deletion(copy.deepcopy(fixture))
    runs, walls = [], []
    for _ in range(5):
        dataset._stage_timing = timing = {}
        t0 = time.perf_counter()
        dataset.correct_deletion(copy.deepcopy(fixture))
        walls.append(time.perf_counter() - t0)
        runs.append(timing)
    dataset._stage_timing = None
    lines.append("dataset.correct_deletion on the test fixture (12 reads, 5 chunks of 200 bases), wall ms, median of 5 after one warm-up run: %.1f"
                 % (statistics.median(walls) * 1e3))
    for key in runs[0]:
        lines.append("  %-20s %.2f" % (key, statistics.median(r[key] for r in runs) * 1e3))
    lines.append("  %-20s %.2f" % ("host (the rest)", (statistics.median(walls) - sum(statistics.median(r[k] for r in runs) for k in runs[0])) * 1e3))
    t0 = time.perf_counter()
    DR.correct_deletion(fixture)
    lines.append("tests/deletion_reference.py on the same fixture: %.1f ms" % ((time.perf_counter() - t0) * 1e3))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
