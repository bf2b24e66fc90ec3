"""Diagnostic (GPU box): time of jtk_lc_fill_candidates on a synthetic read set in the shape of the headline data -- 2,500
chunks in a line, 60-fold coverage, reads of 10-40 nodes on both strands, 1-3 clusters per chunk, a share of the nodes dropped.
After a warm-up call: the host-clock time of 20 calls (each ends in a device synchronise), the median and the spread, the
HIP-event time of the whole call and of the pair kernels (jtk_lc_debug_fill_timing), and aligned pairs per second.
The same process then runs tests/fill_reference.py on every 100th read as the target (against all reads), checks that the device
gave the same answer for those reads, and reports the reference's time scaled by 100: a sanity figure, not a baseline -- nobody
has timed JTK's own get_pileup here.
`python scripts/fill_candidates_timing.py [--chunks N] [--coverage C] [--dropout P] [--out profiles/fill_candidates_timing.txt]`"""
import argparse
import hashlib
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fill_cases as K  # noqa: E402
import fill_reference as R  # noqa: E402
from jtk_amd import api, ffi  # noqa: E402


def read_set(n_chunks, coverage, dropout, seed):
    rng = random.Random(seed)
    n_clusters = [rng.randrange(1, 4) for _ in range(n_chunks)]
    reads, nodes_wanted, n_nodes = [], n_chunks * coverage, 0
    while n_nodes < nodes_wanted:
        length, hap = rng.randrange(10, 41), rng.randrange(0, 3)
        first = rng.randrange(-length + 1, n_chunks)
        nodes, pos = [], rng.randrange(0, 2000)
        for c in range(max(first, 0), min(first + length, n_chunks)):
            q = 2000 + rng.randrange(-40, 41)
            if rng.random() >= dropout:
                nodes.append((c, hap % n_clusters[c], True, q, pos))
            pos += q + rng.randrange(-50, 500)
        if not nodes:
            continue
        n_nodes += len(nodes)
        reads.append(K.reverse(nodes, pos + 100) if rng.random() < 0.5 else nodes)
    return reads


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--chunks", type=int, default=2500)
    ap.add_argument("--coverage", type=int, default=60)
    ap.add_argument("--dropout", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--sample", type=int, default=100, help="the reference runs on every N-th read as the target (0: skip it)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if ffi.lib().jtk_lc_device_ok(0) != 1:
        sys.exit("no gfx950 device: nothing is measured here")
    reads = read_set(args.chunks, args.coverage, args.dropout, args.seed)
    node_off, flat = K.flatten(reads)
    nodes = np.array(flat, dtype=ffi.FILL_NODE_DT)
    out = api.fill_candidates(node_off, nodes)          # warm-up: code objects, rocprim's kernels, the candidate capacity
    cap = len(out["cands"])
    wall, dev, pair = [], [], []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        again = api.fill_candidates(node_off, nodes, cand_cap=cap)
        wall.append((time.perf_counter() - t0) * 1e3)
        t = api.fill_timing()
        dev.append(t["device_ms"])
        pair.append(t["pair_ms"])
        assert all(again[k].tobytes() == out[k].tobytes() for k in ("coverage", "ins_thr", "cand_off", "cands"))
    with open(ffi.LIB_PATH, "rb") as f:
        lib_hash = hashlib.sha256(f.read()).hexdigest()[:16]
    med = float(np.median(wall))
    lines = ["jtk_lc_fill_candidates on a synthetic read set, library sha256[:16] %s" % lib_hash,
             "reads %d, nodes %d, chunks %d, coverage %d, node drop-out %.2f, seed %d" % (len(reads), len(nodes), args.chunks, args.coverage,
                                                                                        args.dropout, args.seed),
             "pairs aligned per call %d, insertion records %d, candidates %d (head %d, tail %d)" % (
                 t["n_pairs"], t["n_records"], cap, int((out["cands"]["side"] == 0).sum()), int((out["cands"]["side"] == 1).sum())),
             "host clock per call, ms: median %.2f, min %.2f, max %.2f over %d calls after a warm-up" % (med, min(wall), max(wall), len(wall)),
             "HIP events, ms: whole call on its stream median %.2f, pair kernels median %.2f" % (float(np.median(dev)), float(np.median(pair))),
             "pairs per second: %.3g by the host clock, %.3g by the pair kernels' time" % (t["n_pairs"] / (med * 1e-3),
                                                                                          t["n_pairs"] / (float(np.median(pair)) * 1e-3))]
    if args.sample:
        mask = [int(r % args.sample == 0) for r in range(len(reads))]
        t0 = time.perf_counter()
        ref = R.fill_candidates(reads, mask)
        ref_s = time.perf_counter() - t0
        got = api.fill_candidates(node_off, nodes, target=mask)
        same = (got["coverage"].tolist() == ref["coverage"] and got["ins_thr"].tolist() == ref["ins_thr"]
                and got["cand_off"].tolist() == ref["cand_off"]
                and [tuple(int(c[k]) for k in ("read", "slot", "side", "chunk", "cluster", "is_forward", "count", "position"))
                     for c in got["cands"]] == ref["cands"])
        lines.append("sanity figure, NOT a baseline: the Python reference on a 1/%d sample (%d targets against all reads) took %.1f s, "
                     "i.e. about %.0f s for every read on one CPU thread; its answer for the sample %s the device's" % (
                         args.sample, sum(mask), ref_s, ref_s * args.sample, "equals" if same else "DIFFERS FROM"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
