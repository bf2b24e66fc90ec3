"""Diagnostic (GPU box): time of jtk_lc_encode_nodes and of its guided passes on a synthetic set of trials in the shape of
correct_deletion's -- by default 6,000 trials, 2 kbp consensi (60 trials share one), 2.4 kbp windows on both strands that carry a
copy of the consensus at 10 % error, sim_thr 0.25 (band 180); `--unrelated` of the windows carry an unrelated sequence instead,
what a wrong candidate looks like, so that the verdict rejects some.
After a warm-up call: the host-clock time of 20 calls (each ends in a device synchronise), the HIP-event time of the three
guided passes (jtk_lc_debug_encode_timing), cells per second, the traceback bytes the mapping writes (one per cell) against
HBM's rate as its floor, and the share of the third pass spent on trials the verdict then rejects (the third pass of a call
on the accepted trials alone against that of all).  Nobody has timed JTK's own encode_node here: no speed-up is stated.
`python scripts/guided_timing.py [--trials N] [--cons-len L] [--error E] [--sim-thr S] [--out profiles/guided_timing.txt]`"""
import argparse
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from jtk_amd import api, ffi  # noqa: E402

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
HBM_MEASURED_TBS, HBM_SPEC_TBS = 6.29, 8.0      # MI355X: float4 copy measured, datasheet peak


def mutate(rng, codes, rate):
    """substitutions, deletions and insertions at rate / 3 each, on base codes 0 ..= 3"""
    r = rng.random(len(codes))
    sub, dele, ins = r < rate / 3, (r >= rate / 3) & (r < 2 * rate / 3), (r >= 2 * rate / 3) & (r < rate)
    codes = np.where(sub, (codes + rng.integers(1, 4, len(codes))) % 4, codes)
    counts = np.where(dele, 0, np.where(ins, 2, 1))
    out = np.repeat(codes, counts)
    at = (np.cumsum(counts) - counts)[ins]
    out[at] = rng.integers(0, 4, len(at))
    return out


def revcomp(codes):
    return (3 - codes)[::-1]


def trial_set(n_trials, cons_len, error, sim_thr, unrelated, per_cons, seed):
    rng = np.random.default_rng(seed)
    flank = cons_len // 10
    reads, conses, chunks, rows = [], [], [], []
    read_at = cons_at = chunk_at = 0
    for t in range(n_trials):
        if t % per_cons == 0:
            cons = rng.integers(0, 4, cons_len)
            chunk = mutate(rng, cons, 0.01)
            cons_off, chunk_off = cons_at, chunk_at
            conses.append(cons)
            chunks.append(chunk)
            cons_at += len(cons)
            chunk_at += len(chunk)
        node = rng.integers(0, 4, cons_len) if rng.random() < unrelated else mutate(rng, cons, error)
        window = np.concatenate([rng.integers(0, 4, flank), node, rng.integers(0, 4, flank)])
        forward = t % 2 == 0
        reads.append(window if forward else revcomp(window))
        rows.append((read_at, 0, len(window), int(forward), len(cons), cons_off, chunk_off, len(chunk), 0, sim_thr))
        read_at += len(window)
    flat = lambda parts: ACGT[np.concatenate(parts)]
    return np.array(rows, dtype=ffi.ENCODE_TRIAL_DT), flat(reads), flat(conses), flat(chunks)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--trials", type=int, default=6000)
    ap.add_argument("--cons-len", type=int, default=2000)
    ap.add_argument("--error", type=float, default=0.10)
    ap.add_argument("--sim-thr", type=float, default=0.25)
    ap.add_argument("--unrelated", type=float, default=0.10)
    ap.add_argument("--per-cons", type=int, default=60)
    ap.add_argument("--seed", type=int, default=13)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if ffi.lib().jtk_lc_device_ok(0) != 1:
        sys.exit("no gfx950 device: nothing is measured here")
    trials, reads, conses, chunks = trial_set(args.trials, args.cons_len, args.error, args.sim_thr, args.unrelated, args.per_cons, args.seed)
    first = api.encode_nodes(trials, reads, conses, chunks)            # warm-up: code objects, the first allocations
    wall, passes, infix = [], [], []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        again = api.encode_nodes(trials, reads, conses, chunks)
        wall.append((time.perf_counter() - t0) * 1e3)
        t = api.encode_timing()
        passes.append(t["pass_ms"])
        infix.append(t["infix_host_ms"])
        assert again["result"].tobytes() == first["result"].tobytes() and again["ops"].tobytes() == first["ops"].tobytes()
    res = first["result"]
    accepted = res["verdict"] == ffi.ENCODE_ACCEPTED
    third_all = float(np.median([p[2] for p in passes]))
    third_acc = []
    if accepted.any() and not accepted.all():
        for _ in range(5):
            api.encode_nodes(trials[accepted], reads, conses, chunks)
            third_acc.append(api.encode_timing()["pass_ms"][2])
    with open(ffi.LIB_PATH, "rb") as f:
        lib_hash = hashlib.sha256(f.read()).hexdigest()[:16]
    med = float(np.median(wall))
    pass_ms = [float(np.median([p[k] for p in passes])) for k in range(3)]
    cells = t["pass_cells"]
    guided_ms, all_cells = sum(pass_ms), sum(cells)
    lines = ["jtk_lc_encode_nodes on a synthetic trial set, library sha256[:16] %s" % lib_hash,
             "trials %d (%d per consensus), consensus %d bases, windows about %d, error %.2f, sim_thr %.2f (band %d), unrelated windows %.2f, seed %d" % (
                 len(trials), args.per_cons, args.cons_len, int(np.mean(trials["end"] - trials["start"])), args.error, args.sim_thr,
                 int(res["band"][0]), args.unrelated, args.seed),
             "verdicts: accepted %d, lower bound %d, rejected %d; statuses not 0: %d" % (
                 int(accepted.sum()), int((res["verdict"] == ffi.ENCODE_LOWER_BOUND).sum()), int((res["verdict"] == ffi.ENCODE_REJECTED).sum()),
                 int((res["status"] != 0).sum())),
             "host clock per call, ms: median %.1f, min %.1f, max %.1f over %d calls after a warm-up" % (med, min(wall), max(wall), len(wall)),
             "of which the infix alignment (jtk_lc_align_reads_mode, host clock), ms: median %.1f" % float(np.median(infix)),
             "HIP events, ms: guided pass 1 %.1f, pass 2 %.1f, pass 3 %.1f (medians; rows, fill and walk kernels of every slice)" % tuple(pass_ms),
             "cells filled per call: %d + %d + %d = %.3g; %.3g cells per second by the guided kernels' time" % (
                 cells[0], cells[1], cells[2], all_cells, all_cells / (guided_ms * 1e-3)),
             "traceback bytes written per call %.3g (one per cell): at HBM's measured %.2f TB/s that is %.2f ms, at the datasheet's %.1f TB/s "
             "%.2f ms -- the floor of this mapping; the kernels take %.1f x the measured-rate floor" % (
                 all_cells, HBM_MEASURED_TBS, all_cells / (HBM_MEASURED_TBS * 1e9), HBM_SPEC_TBS, all_cells / (HBM_SPEC_TBS * 1e9),
                 guided_ms / (all_cells / (HBM_MEASURED_TBS * 1e9)))]
    if third_acc:
        acc = float(np.median(third_acc))
        lines.append("third pass, ms: %.1f for every trial past the filter, %.1f for the accepted ones alone: %.0f %% of it is spent on "
                     "trials the verdict then rejects" % (third_all, acc, 100.0 * (1.0 - acc / third_all)))
    else:
        lines.append("third pass, ms: %.1f; the verdict rejects none (or all) of the trials here, so no share is stated" % third_all)
    lines.append("no time of JTK's own encode_node exists here: no speed-up is stated")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
