"""Diagnostic (GPU box): host-clock time of jtk_lc_align_reads on the headline-shaped batch (2,500 x 60 reads x 2 kbp, the
generator's ops discarded) after a warm-up call, median of 5 calls with the spread, and from the same process (a) the CPU
oracle's jo_edit_ops over a 200-read sample on the usable CPUs scaled to the batch, (b) the pair-HMM + polish kernel time
jtk_lc_last_timing reports for one jtk_lc_cluster_chunks call on the same batch: the polishing these ops feed.  Band cells
per second come from the lengths and the final t of every pair (the schedule of DESIGN section 5).
`python scripts/align_timing.py [--chunks N] [--out profiles/align_timing.txt]`; `--align-only` for a rocprofv3 run.
`--mode infix|prefix --flank N [--out profiles/align_modes_timing.txt]`: jtk_lc_align_reads_mode with the template whole and,
as the free sequence, the batch's read with N random bases added on each side; the same process then times the global call
on the unflanked batch, and the file gives both calls' time and band cells per second, their ratio, and the move-code
scratch per pair of the final band."""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
from jtk_amd import api, batch as jb  # noqa: E402


def band_cells(tl, rl, d):
    """cells of every band the schedule fills for a pair of distance d -> (cells of all tries, tries)"""
    longest, delta = max(tl, rl), abs(tl - rl)
    t = min(longest, delta + max(32, (tl + rl) // 12))
    cells, tries = 0, 0
    while True:
        e = (t - delta) // 2
        klo, khi = max(min(rl - tl, 0) - e, -tl), min(max(rl - tl, 0) + e, rl)
        cells += (khi - klo + 1) * (tl + rl) // 2
        tries += 1
        if t >= d:
            return cells, tries
        t = min(2 * t, longest)


def scratch_bytes(tl, rl, w):
    """move codes of one pair with a band of w diagonals: 16 bytes per 8 anti-diagonals and group of 8 same-parity cells"""
    return ((tl + rl) // 8 + 1) * (((w + 1) // 2 + 7) // 8) * 16


def mode_band_cells(tl, rl, d, mode):
    """the same for infix / prefix with the read free -> (cells of all tries, tries, scratch bytes of the last band)"""
    t = min(tl, max(tl - rl, 0) + max(32, tl // 6))
    cells, tries = 0, 0
    while True:
        klo, khi = -t, rl - tl + t
        if mode == "prefix":
            klo, khi = max(klo, -t), min(khi, t)
        klo, khi = max(klo, -tl), min(khi, rl)
        w = khi - klo + 1
        cells += w * (tl + rl) // 2
        tries += 1
        if t >= d:
            return cells, tries, scratch_bytes(tl, rl, w)
        t = min(2 * t, tl)


def flanked(b, n, seed=7):
    """the batch with n random bases in front of and behind every read (no ops)"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    none = np.zeros(0, np.uint8)
    piles = []
    for c in range(b.n_chunks):
        reads = [np.concatenate([acgt[rng.integers(0, 4, n)], b.read(r), acgt[rng.integers(0, 4, n)]]) for r in b.chunk_reads(c)]
        piles.append((int(b.chunks["chunk_id"][c]), int(b.chunks["copy_num"][c]), b.template(c), reads, [none] * len(reads),
                      [1] * len(reads), None))
    return jb.pack(piles)


def timed(fn, calls):
    fn()                                                     # warm-up at size: first touch of the host buffers
    times = []
    for _ in range(calls):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    times.sort()
    return out, times


def modes_main(args, b):
    fb = flanked(b, args.flank)
    api.align_reads(b.subset([0]))                           # warm-up: context, code objects
    api.align_reads(fb.subset([0]), mode=args.mode, free="read")
    out, times = timed(lambda: api.align_reads(fb, mode=args.mode, free="read"), args.calls)
    gout, gtimes = timed(lambda: api.align_reads(b), args.calls)
    tl = np.repeat(b.chunks["tmpl_len"].astype(np.int64), b.chunks["n_reads"]).tolist()
    cells = tries = scratch = gcells = gtries = 0
    for a, c, d in zip(tl, np.diff(fb.read_off.astype(np.int64)).tolist(), out["dist"].tolist()):
        x, y, z = mode_band_cells(a, c, d, args.mode)
        cells, tries, scratch = cells + x, tries + y, scratch + z
    for a, c, d in zip(tl, np.diff(b.read_off.astype(np.int64)).tolist(), gout["dist"].tolist()):
        x, y = band_cells(a, c, d)
        gcells, gtries = gcells + x, gtries + y
    med, gmed = times[len(times) // 2], gtimes[len(gtimes) // 2]
    # the first global band: |delta| + 2 * ((t - |delta|) / 2) + 1 diagonals
    g_scratch = sum(scratch_bytes(a, c, abs(a - c) + (min(max(a, c), abs(a - c) + max(32, (a + c) // 12)) - abs(a - c)) // 2 * 2 + 1)
                    for a, c in zip(tl, np.diff(b.read_off.astype(np.int64)).tolist()))
    lines = ["jtk_lc_align_reads_mode, mode %s, the read free with %d random bases on each side; %d chunks x %d reads, templates of %d bases"
             % (args.mode, args.flank, b.n_chunks, b.n_reads // b.n_chunks, int(np.median(tl))),
             "%s: host clock per call: median %.1f ms, min %.1f, max %.1f (%d calls after two warm-ups)"
             % (args.mode, 1e3 * med, 1e3 * times[0], 1e3 * times[-1], len(times)),
             "%s: distance: median %d, max %d; tries per pair %.3f; band cells filled %.3e -> %.3e cells/s of call time"
             % (args.mode, int(np.median(out["dist"])), int(out["dist"].max()), tries / b.n_reads, cells, cells / med),
             "%s: move-code scratch of the final band: %.0f bytes per pair" % (args.mode, scratch / b.n_reads),
             "global (jtk_lc_align_reads, the unflanked batch, same process): median %.1f ms, min %.1f, max %.1f"
             % (1e3 * gmed, 1e3 * gtimes[0], 1e3 * gtimes[-1]),
             "global: distance: median %d, max %d; tries per pair %.3f; band cells filled %.3e -> %.3e cells/s of call time"
             % (int(np.median(gout["dist"])), int(gout["dist"].max()), gtries / b.n_reads, gcells, gcells / gmed),
             "global: move-code scratch of the first band: %.0f bytes per pair" % (g_scratch / b.n_reads),
             "%s / global: time %.2f, cells %.2f, cells per second %.2f" % (args.mode, med / gmed, cells / gcells, (cells / med) / (gcells / gmed))]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=2500)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--align-only", action="store_true", help="warm-up + one call, nothing else (for rocprofv3 --kernel-trace)")
    ap.add_argument("--out", default="")
    ap.add_argument("--mode", default="global", choices=("global", "infix", "prefix"))
    ap.add_argument("--flank", type=int, default=200, help="random bases added on each side of every read (--mode infix / prefix)")
    args = ap.parse_args()
    b, cfg = bench.make_batch_parallel("ont_diploid", np.arange(args.chunks), threads=16)
    if args.mode != "global":
        return modes_main(args, b)
    small = b.subset([0])
    api.align_reads(small)                                   # warm-up: context, code objects
    if args.align_only:
        api.align_reads(b)
        return
    api.align_reads(b)                                       # warm-up at size: first-touch of the host buffers
    times = []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        out = api.align_reads(b)
        times.append(time.perf_counter() - t0)
    times.sort()
    tl = np.repeat(b.chunks["tmpl_len"].astype(np.int64), b.chunks["n_reads"])
    rl = np.diff(b.read_off.astype(np.int64))
    cells = tries = 0
    for a, c, d in zip(tl.tolist(), rl.tolist(), out["dist"].tolist()):
        x, y = band_cells(a, c, d)
        cells, tries = cells + x, tries + y
    lines = ["jtk_lc_align_reads, %d chunks x %d reads, %d bases of reads" % (b.n_chunks, b.n_reads // b.n_chunks, len(b.read_bases)),
             "host clock per call: median %.1f ms, min %.1f, max %.1f (%d calls after two warm-ups)"
             % (1e3 * times[len(times) // 2], 1e3 * times[0], 1e3 * times[-1], len(times)),
             "distance: median %d, max %d; tries per pair %.3f; band cells filled %.3e -> %.3e cells/s of call time"
             % (int(np.median(out["dist"])), int(out["dist"].max()), tries / b.n_reads, cells, cells / times[len(times) // 2])]
    # (a) the CPU oracle on a sample
    import oracle_ffi as O
    sample = np.random.default_rng(1).choice(b.n_reads, 200, replace=False)
    chunk_of = np.repeat(np.arange(b.n_chunks), b.chunks["n_reads"])
    O.edit_ops(b.template(0), b.read(0))
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=16) as ex:          # ctypes releases the GIL inside jo_edit_ops
        ref = list(ex.map(lambda r: O.edit_ops(b.template(int(chunk_of[r])), b.read(int(r))), sample))
    cpu = time.perf_counter() - t0
    same = all(bytes(ref[k]) == bytes(out["ops"][int(out["ops_off"][r]):int(out["ops_off"][r + 1])]) for k, r in enumerate(sample))
    lines.append("CPU oracle jo_edit_ops (full matrix), 200 reads on 16 threads: %.3f s -> %.1f s for the batch; ops identical: %s"
                 % (cpu, cpu * b.n_reads / 200, same))
    # (b) the polishing the ops feed
    p = jb.default_params(haploid_coverage=30.0, band_frac=cfg["band_frac"])
    api.cluster_chunks(p, b)
    tm = api.last_timing()
    lines.append("jtk_lc_cluster_chunks on the same batch: kernel_ms phmm %.1f + polish %.1f = %.1f ms (total %.1f ms)"
                 % (tm["kernel_ms"]["phmm"], tm["kernel_ms"]["polish"], tm["kernel_ms"]["phmm"] + tm["kernel_ms"]["polish"], tm["total_ms"]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
