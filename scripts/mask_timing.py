"""Diagnostic (GPU box): the figures of DESIGN section 5, "Repeat masking" -- one jtk_lc_mask_repeats call on synthetic reads of
100 Mbases (a random genome of 5 Mbases with a 5 kbase repeat planted 40 times, 10,000-base reads from both strands with 1 %
substitutions) at k = 12 (32-bit keys) and at k = 21 (64-bit keys): one warm-up call, then three; per phase of
jtk_lc_debug_mask_timing the HIP-event milliseconds (median, spread) and the bytes per second that DESIGN's traffic estimate of
the phase comes to, beside the HBM rate of the micro-architecture guide.  Before any device call, the CPU yardstick: the
algorithm of tests/mask_reference.py restated with numpy (numpy.unique per worker, merged) on 16 processes, whose report must
equal the device's.
`python scripts/mask_timing.py [--mbases N] [--out profiles/mask_timing.txt]`"""
import argparse
import math
import multiprocessing
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from jtk_amd import api, ffi  # noqa: E402

HBM_TBS = 6.3        # achievable, MI355X (8 TB/s peak)
READ_LEN = 10000
WORKERS = 16
FWD = np.zeros(256, dtype=np.uint64)
CMP = np.zeros(256, dtype=np.uint64)
for _b, _f, _c in ((65, 0, 3), (67, 1, 2), (71, 2, 1), (84, 3, 0)):
    FWD[_b] = FWD[_b + 32] = _f
    CMP[_b] = CMP[_b + 32] = _c


def traffic(k, distinct_share):
    """DESIGN's estimate, bytes per base and phase, for keys of K bytes: emit reads a base and writes a key; the sort reads the keys
    once for its histograms and reads and writes them once per pass of 8 bits; counting clears and writes the counts, reads the
    sorted keys, writes a key and a count per distinct k-mer and reads both twice for the selections; apply reads and writes a base"""
    K = 4 if 2 * k <= 32 else 8
    passes = (2 * k + 7) // 8
    return dict(emit_ms=1 + K, sort_ms=K + passes * 2 * K, select_ms=4 + K + distinct_share * 3 * (K + 4), apply_ms=2)


def synth(mbases, seed=7):
    rng = np.random.default_rng(seed)
    n = mbases * 1000000
    genome = rng.integers(0, 4, size=max(n // 20, 4 * READ_LEN), dtype=np.uint8)
    repeat = rng.integers(0, 4, size=5000, dtype=np.uint8)
    for at in rng.integers(0, len(genome) - 5000, size=40):
        genome[at:at + 5000] = repeat
    reads = []
    for at in rng.integers(0, len(genome) - READ_LEN, size=n // READ_LEN):
        r = genome[at:at + READ_LEN]
        reads.append(3 - r[::-1] if rng.random() < 0.5 else r)
    flat = np.concatenate(reads)
    errors = rng.random(len(flat)) < 0.01
    flat[errors] = rng.integers(0, 4, size=int(errors.sum()), dtype=np.uint8)
    flat = np.frombuffer(b"ACGT", dtype=np.uint8)[flat]
    return [flat[i:i + READ_LEN].tobytes() for i in range(0, len(flat), READ_LEN)]


_reads, _k, _mask = None, 0, None


def kmers_of(read, k):
    b = np.frombuffer(read, dtype=np.uint8)
    if len(b) < k:
        return np.zeros(0, dtype=np.uint64)
    f, c, n = FWD[b], CMP[b], len(b) - k + 1
    fwd, rev = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    for j in range(k):
        fwd |= f[j:j + n] << np.uint64(2 * j)
        rev |= c[k - 1 - j:k - 1 - j + n] << np.uint64(2 * j)
    return np.minimum(fwd, rev)


def count_part(part):
    return np.unique(np.concatenate([kmers_of(r, _k) for r in _reads[part::WORKERS]] or [np.zeros(0, np.uint64)]), return_counts=True)


def cover_part(part):
    lower = 0
    for r in _reads[part::WORKERS]:
        km = kmers_of(r, _k)
        at = np.searchsorted(_mask, km)
        hits = np.flatnonzero((at < len(_mask)) & (_mask[np.minimum(at, len(_mask) - 1)] == km)) if len(_mask) else np.zeros(0, np.int64)
        d = np.zeros(len(r) + 1, dtype=np.int64)
        np.add.at(d, hits, 1)
        np.add.at(d, hits + _k, -1)
        lower += int((np.cumsum(d)[:len(r)] > 0).sum())
    return lower


def cpu_yardstick(reads, k, freq, min_count):
    """tests/mask_reference.py's algorithm with numpy on WORKERS processes: (seconds, the report's fields it computes)"""
    global _reads, _k, _mask
    _reads, _k = reads, k
    t0 = time.perf_counter()
    with multiprocessing.get_context("fork").Pool(WORKERS) as pool:
        parts = pool.map(count_part, range(WORKERS))
    u, inv = np.unique(np.concatenate([p[0] for p in parts]), return_inverse=True)
    c = np.bincount(inv, weights=np.concatenate([p[1] for p in parts]).astype(np.float64)).astype(np.int64)
    repeated = np.sort(c[c > 1])
    percentile, below = int(math.floor(float(len(repeated)) * (1.0 - freq))), int(np.searchsorted(repeated, min_count, side="right"))
    if percentile < below:
        thr, takes_all, _mask = 0, 1, u[c > 1]
    else:
        thr, takes_all = int(repeated[percentile]), 0
        _mask = u[c > thr]
    with multiprocessing.get_context("fork").Pool(WORKERS) as pool:
        lower = sum(pool.map(cover_part, range(WORKERS)))
    seconds = time.perf_counter() - t0
    return seconds, dict(n_distinct=len(u), n_singleton=int((c == 1).sum()), n_masked_kmers=len(_mask), n_lower=lower, thr=thr, takes_all=takes_all)


def spread(xs):
    return "median %.3f min %.3f max %.3f" % (statistics.median(xs), min(xs), max(xs))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mbases", type=int, default=100)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    reads = synth(args.mbases)
    n_bases = sum(len(r) for r in reads)
    lines = ["mask_repeats: %d reads, %d bases, freq 0.001, min_count 10" % (len(reads), n_bases)]
    cpu = {k: cpu_yardstick(reads, k, 0.001, 10) for k in (12, 21)}      # forks: before the first device call
    if ffi.lib().jtk_lc_device_ok(0) != 1:
        sys.exit("no gfx950 device: nothing is measured here")
    for k in (12, 21):
        api.mask_repeats(reads[:100], k, 0.001, 10)
        _, report, _ = api.mask_repeats(reads, k, 0.001, 10)             # the warm-up call at this shape
        phases, host = {}, []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            _, report, _ = api.mask_repeats(reads, k, 0.001, 10)
            host.append(time.perf_counter() - t0)
            for name, ms in api.mask_timing().items():
                phases.setdefault(name, []).append(ms)
        est = traffic(k, report["n_distinct"] / max(report["n_kmers"], 1))
        lines.append("k = %d (%d-bit keys): rc %d, %s" % (k, 32 if 2 * k <= 32 else 64, report["rc"], ", ".join("%s %d" % (f, report[f]) for f in ffi.MASK_REPORT_DT.names)))
        total = 0.0
        for name in ("emit_ms", "sort_ms", "select_ms", "apply_ms"):
            ms = statistics.median(phases[name])
            total += ms
            lines.append("  %-10s %s ms; estimate %.1f B/base -> %.2f TB/s (HBM %.1f TB/s achievable)"
                         % (name[:-3], spread(phases[name]), est[name], est[name] * n_bases / (ms * 1e-3) / 1e12, HBM_TBS))
        lines.append("  the four phases %.3f ms = %.2f Gbases/s; host clock around api.mask_repeats (upload, copy back, Python packing): %s s"
                     % (total, n_bases / (total * 1e-3) / 1e9, spread(host)))
        seconds, want = cpu[k]
        same = all(report[f] == v for f, v in want.items())
        lines.append("  numpy.unique restatement on %d processes: %.2f s (%s report as the device)" % (WORKERS, seconds, "the same" if same else "A DIFFERENT"))
        if not same:
            lines.append("    numpy: %r" % (want,))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
