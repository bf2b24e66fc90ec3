"""Diagnostic (GPU box): one measurement of jtk_lc_polish_guided on pile-ups of the headline's size -- by default 2,500 pile-ups x
60 reads x 2 kbp (jtk_synth's ont_diploid), radius 60, every read voting.
After a warm-up call on a few pile-ups: the host-clock time of one call (it ends in a device synchronise), the HIP-event time of
its rounds' kernels (jtk_lc_debug_gpolish_timing: events around synchronised work), per round, band cells per second, and the bytes
of the F table the kernels write (2 per cell of every fill) and read (the table of a voting read reads F rows p .. p + 3 at every
position: 8 per cell) over the kernel time, against HBM's rate.  Alongside, as context only, the host-clock time of
jtk_lc_polish_chunks (the pair-HMM polish, another algorithm) on the same pile-ups in the same process.  Nobody has timed JTK's
own polish_until_converge here: no speed-up is stated.
`python scripts/gpolish_timing.py [--chunks N] [--radius R] [--out profiles/gpolish_timing.txt]`"""
import argparse
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from jtk_amd import api, ffi, synth  # noqa: E402
from jtk_amd.batch import default_params, pack  # noqa: E402

HBM_MEASURED_TBS, HBM_SPEC_TBS = 6.29, 8.0      # MI355X: float4 copy measured, datasheet peak


def _pileup(job):
    chunk_id, cfg = job
    return synth.make_pileup(chunk_id, cfg, sort=False)      # the order of pileup_nodes plays no part in a polish


def make_batch(config, n_chunks, jobs):
    """jtk_synth's pile-ups, made by `jobs` processes that never open the device (this one has not yet either)"""
    import multiprocessing
    cfg = dict(synth.CONFIGS[config])
    work = [(c, cfg) for c in range(n_chunks)]
    if jobs > 1 and n_chunks > 1:
        with multiprocessing.get_context("fork").Pool(jobs) as pool:
            piles = pool.map(_pileup, work, chunksize=max(1, n_chunks // (4 * jobs)))
    else:
        piles = [_pileup(w) for w in work]
    return pack(piles), cfg


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--chunks", type=int, default=2500)
    ap.add_argument("--radius", type=int, default=60)
    ap.add_argument("--config", default="ont_diploid")
    ap.add_argument("--jobs", type=int, default=16, help="processes that make the pile-ups")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    batch, cfg = make_batch(args.config, args.chunks, args.jobs)
    if ffi.lib().jtk_lc_device_ok(0) != 1:
        sys.exit("no gfx950 device: nothing is measured here")
    warm = batch.subset(range(min(8, args.chunks)))
    api.polish_guided(warm, args.radius)                     # warm-up: code objects, the first allocations
    t0 = time.perf_counter()
    out = api.polish_guided(batch, args.radius)
    wall = (time.perf_counter() - t0) * 1e3
    t = api.gpolish_timing()
    rounds = out["result"]["polish_rounds"]
    params = default_params(cfg["coverage"], band_frac=cfg["band_frac"])
    api.polish_chunks(params, warm, radius=args.radius)
    t0 = time.perf_counter()
    hmm = api.polish_chunks(params, batch, radius=args.radius)
    hmm_wall = (time.perf_counter() - t0) * 1e3
    same = sum(bytes(out["cons"][int(out["cons_off"][c]):int(out["cons_off"][c + 1])]) ==
               bytes(hmm["cons"][int(hmm["cons_off"][c]):int(hmm["cons_off"][c + 1])]) for c in range(batch.n_chunks))
    with open(ffi.LIB_PATH, "rb") as f:
        lib_hash = hashlib.sha256(f.read()).hexdigest()[:16]
    written, read = 2.0 * t["cells"], 8.0 * t["vote_cells"]
    sec = t["kernel_ms"] * 1e-3
    lines = ["jtk_lc_polish_guided on synthetic pile-ups, library sha256[:16] %s" % lib_hash,
             "%d pile-ups (%s), %d reads, template %d bases, radius %d, every read votes; statuses not 0: %d" % (
                 batch.n_chunks, args.config, t["n_reads"], cfg["tmpl_len"], args.radius, int((out["result"]["status"] != 0).sum())),
             "rounds per pile-up: min %d, median %d, max %d; rounds the host enqueued %d, then the closing fill; %d slices of the work area per pass" % (
                 int(rounds.min()), int(np.median(rounds)), int(rounds.max()), t["rounds"], t["slices"]),
             "host clock of the call, ms: %.1f (one call after a warm-up on %d pile-ups; uploads, the rounds, the pack and the copies back)" % (
                 wall, warm.n_chunks),
             "HIP events around the rounds' kernels, ms: %.1f in all, %.1f per enqueued round" % (t["kernel_ms"], t["kernel_ms"] / max(t["rounds"], 1)),
             "band cells filled forward %.4g (%.4g by voting reads, which also fill them backward): %.3g cells per second of kernel time" % (
                 t["cells"], t["vote_cells"], t["cells"] / sec),
             "F table: %.4g bytes written, %.4g bytes read by the tables (rows p .. p + 3 at every p): %.3g TB/s over the kernel time, against HBM's "
             "measured %.2f TB/s (datasheet %.1f): %.1f %% of the measured rate" % (
                 written, read, (written + read) / sec / 1e12, HBM_MEASURED_TBS, HBM_SPEC_TBS, 100.0 * (written + read) / sec / 1e12 / HBM_MEASURED_TBS),
             "context only -- jtk_lc_polish_chunks (pair-HMM polish, another algorithm, radius %d) on the same pile-ups in this process: host clock %.1f ms; "
             "%d of %d consensus sequences are byte-identical between the two" % (args.radius, hmm_wall, same, batch.n_chunks),
             "no time of JTK's own polish_until_converge exists here: no speed-up is stated"]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
