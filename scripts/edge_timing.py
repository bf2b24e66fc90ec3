"""Diagnostic (GPU box): time of jtk_lc_encode_edges and of its guided pass on a synthetic set of trials in the shape of
dense_encoding's -- by default 2,000 trials, 2 kbp contigs in 2 chunks (50 trials share one), 2.6 kbp windows on both strands that
carry a copy of the contig at 8 % error, radius 100, sim_thr 0.25.
After 2 warm-up calls: the median host-clock time of 10 calls (each ends in a device synchronise), the HIP-event time of the
guided pass and of the cut and pack kernels, and the host clock of the two infix alignments (jtk_lc_debug_edges_timing).  Nobody
has timed JTK's own encode_edge here, and there is no earlier figure of this call: no speed-up and no threshold is stated.
`python scripts/edge_timing.py [--trials N] [--contig-len L] [--error E] [--radius R] [--out profiles/encode_edges_timing.txt]`"""
import argparse
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from jtk_amd import api, ffi  # noqa: E402
from scripts.guided_timing import ACGT, mutate, revcomp  # noqa: E402


def trial_set(n_trials, contig_len, n_chunks, window_len, error, radius, sim_thr, per_contig, seed):
    rng = np.random.default_rng(seed)
    reads, contigs, breaks, rows = [], [], [], []
    read_at = contig_at = 0
    for t in range(n_trials):
        if t % per_contig == 0:
            contig = rng.integers(0, 4, contig_len)
            contig_off, break_first = contig_at, len(breaks)
            contigs.append(contig)
            contig_at += contig_len
            breaks += [contig_len * (k + 1) // n_chunks for k in range(n_chunks)]
        node = mutate(rng, contig, error)
        flank = max(window_len - len(node), 0)
        window = np.concatenate([rng.integers(0, 4, flank // 2), node, rng.integers(0, 4, flank - flank // 2)])
        forward = t % 2 == 0
        reads.append(window if forward else revcomp(window))
        rows.append((read_at, 0, len(window), int(forward), radius, contig_off, contig_len, n_chunks, break_first, sim_thr))
        read_at += len(window)
    flat = lambda parts: ACGT[np.concatenate(parts)]      # noqa: E731
    return np.array(rows, dtype=ffi.EDGE_TRIAL_DT), flat(reads), flat(contigs), np.array(breaks, dtype=np.uint32)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--trials", type=int, default=2000)
    ap.add_argument("--contig-len", type=int, default=2000)
    ap.add_argument("--chunks", type=int, default=2)
    ap.add_argument("--window-len", type=int, default=2600)
    ap.add_argument("--error", type=float, default=0.08)
    ap.add_argument("--radius", type=int, default=100)
    ap.add_argument("--sim-thr", type=float, default=0.25)
    ap.add_argument("--per-contig", type=int, default=50)
    ap.add_argument("--seed", type=int, default=17)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if ffi.lib().jtk_lc_device_ok(0) != 1:
        sys.exit("no gfx950 device: nothing is measured here")
    trials, reads, contigs, breaks = trial_set(args.trials, args.contig_len, args.chunks, args.window_len, args.error, args.radius, args.sim_thr,
                                               args.per_contig, args.seed)
    for _ in range(args.warmup):                          # code objects, the first allocations
        first = api.encode_edges(trials, reads, contigs, breaks)
    wall, guided, cut, infix = [], [], [], []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        again = api.encode_edges(trials, reads, contigs, breaks)
        wall.append((time.perf_counter() - t0) * 1e3)
        t = api.edges_timing()
        guided.append(t["pass_ms"])
        cut.append(t["cut_ms"])
        infix.append(t["infix_host_ms"])
        assert again["nodes"].tobytes() == first["nodes"].tobytes() and again["ops"].tobytes() == first["ops"].tobytes()
    verdict = first["nodes"]["verdict"]
    with open(ffi.LIB_PATH, "rb") as f:
        lib_hash = hashlib.sha256(f.read()).hexdigest()[:16]
    lines = ["jtk_lc_encode_edges on a synthetic trial set, library sha256[:16] %s" % lib_hash,
             "trials %d (%d per contig), contig %d bases in %d chunks, windows about %d, error %.2f, radius %d, sim_thr %.2f, seed %d" % (
                 len(trials), args.per_contig, args.contig_len, args.chunks, int(np.mean(trials["end"] - trials["start"])), args.error, args.radius,
                 args.sim_thr, args.seed),
             "nodes: accepted %d, rejected %d, not reached %d; statuses not 0: %d" % (
                 int((verdict == ffi.EDGE_ACCEPTED).sum()), int((verdict == ffi.EDGE_REJECTED).sum()), int((verdict == ffi.EDGE_NOT_REACHED).sum()),
                 int((first["result"]["status"] != 0).sum())),
             "host clock per call, ms: median %.1f, min %.1f, max %.1f over %d calls after %d warm-ups (the Python wrapper's node lists included)" % (
                 float(np.median(wall)), min(wall), max(wall), len(wall), args.warmup),
             "of which the two infix alignments (jtk_lc_align_reads_mode, host clock), ms: medians %.1f and %.1f" % (
                 float(np.median([v[0] for v in infix])), float(np.median([v[1] for v in infix]))),
             "HIP events, ms: the guided pass %.2f (median; rows, fill and walk kernels of %d slices), edge_cut_kernel and edge_pack_kernel %.3f" % (
                 float(np.median(guided)), t["slices"], float(np.median(cut))),
             "cells filled per call: %.3g; %.3g cells per second by the guided kernels' time" % (
                 t["pass_cells"], t["pass_cells"] / (float(np.median(guided)) * 1e-3)),
             "no time of JTK's own encode_edge and no earlier figure of this call exist here: no speed-up and no threshold is stated"]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
