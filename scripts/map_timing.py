"""Diagnostic (GPU box): the figures of DESIGN section 5, "Mapping" -- one jtk_lc_map_reads call that maps reads at 60x onto the
2,500 chunks of 2 kbases that tile a random genome of 5 Mbases (10,000-base reads from both strands with 10 % errors:
substitutions, insertions and deletions in equal parts) at the defaults k = 15, w = 10, max_occ = 200, max_gap = 100,
min_seeds = 4: one warm-up call, then three; per phase of jtk_lc_debug_map_timing the HIP-event milliseconds (median, spread)
and the bytes per second that DESIGN's traffic estimate of the phase comes to, beside the HBM rate of the micro-architecture
guide.  Before any device call, the CPU yardstick: the algorithm of tests/map_reference.py restated with numpy (sorts,
searchsorted, reduceat) on 16 processes, whose placements must equal the device's.  It is a yardstick for scale, not minimap2's
time.
`python scripts/map_timing.py [--coverage N] [--out profiles/map_timing.txt]`"""
import argparse
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
READ_LEN, CHUNK_LEN, N_CHUNKS = 10000, 2000, 2500
WORKERS = 16
K, W, MAX_OCC, MAX_GAP, MIN_SEEDS = 15, 10, 200, 100, 4
C0, C1, C2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
CODE = np.full(256, 4, dtype=np.uint64)
for _i, _b in enumerate(b"ACGT"):
    CODE[_b] = CODE[_b + 32] = _i
LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)


def traffic(n_bases, n_min, n_hits):
    """DESIGN's estimate, bytes per phase: the sketch reads a base and writes 16 bytes per minimizer; the index and the queries'
    order are radix sorts of 16-byte pairs (one read for the histograms, a read and a write per pass of 8 bits: 4 passes over 2k =
    30 bits, 6 over the 48 bits of a location), the run lengths and their scan touch 20 bytes per target minimizer; the hits read
    16 bytes and write 4 per query minimizer twice and write 12 per hit; the order reads and writes 8 bytes per hit and pass (8
    passes at most); the chain reads 12 and writes 8 per hit for the flags and their scan, reads 12 and writes 8 in the reduction,
    sorts 8-byte keys (6 passes) and reads them once; the compaction is per cluster and small beside the rest."""
    t_min, q_min = n_min
    return dict(sketch_ms=n_bases + 16 * (t_min + q_min), index_ms=16 * t_min * (1 + 2 * 4) + 16 * q_min * (1 + 2 * 6) + 20 * t_min,
                hits_ms=2 * 20 * q_min + 12 * n_hits, order_ms=8 * n_hits * (1 + 2 * 8), chain_ms=n_hits * (20 + 20 + 8 * (1 + 2 * 6) + 8),
                compact_ms=0)


def synth(coverage, seed=11):
    """-> (chunks, reads) as lists of bytes"""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, size=CHUNK_LEN * N_CHUNKS, dtype=np.uint8)
    chunks = [LETTERS[genome[i:i + CHUNK_LEN]].tobytes() for i in range(0, len(genome), CHUNK_LEN)]
    reads = []
    for at in rng.integers(0, len(genome) - READ_LEN, size=coverage * len(genome) // READ_LEN):
        r = genome[at:at + READ_LEN]
        if rng.random() < 0.5:
            r = 3 - r[::-1]
        u = rng.random(READ_LEN)
        sub, ins, dele = u < 1 / 30, (u >= 1 / 30) & (u < 2 / 30), (u >= 2 / 30) & (u < 0.1)
        r = np.where(sub, (r + rng.integers(1, 4, size=READ_LEN, dtype=np.uint8)) % 4, r).astype(np.uint8)
        count = np.where(dele, 0, np.where(ins, 2, 1))
        out = np.repeat(r, count)
        first = (np.cumsum(count) - count)[ins]                       # an insertion: a random base in front of the base
        out[first] = rng.integers(0, 4, size=len(first), dtype=np.uint8)
        reads.append(LETTERS[out].tobytes())
    return chunks, reads


def np_hash(x, k):
    m = np.uint64((1 << (2 * k)) - 1)
    h = (x ^ C0) & m
    h = (h * C1) & m
    h ^= h >> np.uint64(k)
    h = (h * C2) & m
    h ^= h >> np.uint64(k)
    return h


def np_sketch(seq, k, w):
    """tests/map_reference.py's sketch: (pos, hash, strand) arrays"""
    c = CODE[np.frombuffer(seq, dtype=np.uint8)]
    n = len(c) - k + 1
    if n <= 0:
        return np.zeros(0, np.int64), np.zeros(0, np.uint64), np.zeros(0, np.int64)
    f, r = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    low = c & np.uint64(3)
    for j in range(k):
        f |= low[j:j + n] << np.uint64(2 * j)
        r |= (np.uint64(3) - low[k - 1 - j:k - 1 - j + n]) << np.uint64(2 * j)
    bad = np.concatenate([[0], np.cumsum(c > 3)])
    valid = (bad[k:k + n] == bad[:n]) & (f != r)
    h = np.where(valid, np_hash(np.minimum(f, r), k), NONE)
    width = min(w, n)
    view = np.lib.stride_tricks.sliding_window_view
    minima = view(h, width).min(axis=1)
    pad = np.zeros(width - 1, dtype=np.uint64)                         # 0 never wins a maximum over a window that holds the position
    largest = view(np.concatenate([pad, minima, pad]), width).max(axis=1)
    keep = np.flatnonzero(valid & (largest == h))
    return keep, h[keep], (f > r)[keep].astype(np.int64)


_index, _reads = None, None
PLACEMENT_FIELDS = ffi.MAP_PLACEMENT_DT.names


def map_part(part):
    """the placements of reads part, part + WORKERS, ..: rows of (query, the fields of a placement)"""
    hashes, occ_first, occ_count, t_target, t_pos, t_strand = _index
    rows = []
    for qi in range(part, len(_reads), WORKERS):
        qlen = len(_reads[qi])
        pos, h, strand = np_sketch(_reads[qi], K, W)
        at = np.searchsorted(hashes, h)
        at[at == len(hashes)] = 0
        n = np.where((hashes[at] == h) & (occ_count[at] <= MAX_OCC), occ_count[at], 0)
        if not n.sum():
            continue
        which = np.repeat(np.arange(len(pos)), n)
        rec = np.repeat(occ_first[at], n) + (np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n))
        rev = strand[which] ^ t_strand[rec]
        oq = np.where(rev == 1, qlen - (pos[which] + K), pos[which])
        tpos, target = t_pos[rec], t_target[rec]
        diag = oq - tpos
        order = np.lexsort((tpos, diag, rev, target))
        target, rev, diag, tpos, oq = target[order], rev[order], diag[order], tpos[order], oq[order]
        head = np.ones(len(order), dtype=bool)
        head[1:] = (target[1:] != target[:-1]) | (rev[1:] != rev[:-1]) | (diag[1:] - diag[:-1] > MAX_GAP)
        first = np.flatnonzero(head)
        cid = np.cumsum(head) - 1
        seeds = np.bincount(np.unique(cid * 65536 + tpos) // 65536, minlength=len(first))
        tmin, tmax = np.minimum.reduceat(tpos, first), np.maximum.reduceat(tpos, first) + K
        qmin, qmax = np.minimum.reduceat(oq, first), np.maximum.reduceat(oq, first) + K
        dlo, dhi = np.minimum.reduceat(diag, first), np.maximum.reduceat(diag, first)
        for c in np.flatnonzero(seeds >= MIN_SEEDS):
            rv = int(rev[first[c]])
            rows.append((qi, int(target[first[c]]), 1 - rv, int(seeds[c]), int(qlen - qmax[c] if rv else qmin[c]), int(qlen - qmin[c] if rv else qmax[c]),
                         int(qmin[c]), int(qmax[c]), int(tmin[c]), int(tmax[c]), int(dlo[c]), int(dhi[c])))
    return rows


def cpu_yardstick(chunks, reads):
    """tests/map_reference.py's algorithm with numpy on WORKERS processes: (seconds, the placements)"""
    global _index, _reads
    t0 = time.perf_counter()
    parts = [np_sketch(c, K, W) for c in chunks]
    t_target = np.concatenate([np.full(len(p[0]), t, dtype=np.int64) for t, p in enumerate(parts)])
    t_pos, t_hash, t_strand = (np.concatenate([p[i] for p in parts]) for i in range(3))
    order = np.argsort(t_hash, kind="stable")
    hashes, occ_first, occ_count = np.unique(t_hash[order], return_index=True, return_counts=True)
    _index, _reads = (hashes, occ_first, occ_count, t_target[order], t_pos[order], t_strand[order]), reads
    with multiprocessing.get_context("fork").Pool(WORKERS) as pool:
        rows = sorted((r for part in pool.map(map_part, range(WORKERS)) for r in part), key=lambda r: r[0])   # (stable: a read's rows stay in order)
    return time.perf_counter() - t0, np.array(rows, dtype=ffi.MAP_PLACEMENT_DT)


def spread(xs):
    return "median %.3f min %.3f max %.3f" % (statistics.median(xs), min(xs), max(xs))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--coverage", type=int, default=60)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    chunks, reads = synth(args.coverage)
    n_bases = sum(len(r) for r in reads) + sum(len(c) for c in chunks)
    lines = ["map_reads: %d chunks of %d bases, %d reads, %d bases in all, k %d w %d max_occ %d max_gap %d min_seeds %d"
             % (len(chunks), CHUNK_LEN, len(reads), n_bases, K, W, MAX_OCC, MAX_GAP, MIN_SEEDS)]
    seconds, want = cpu_yardstick(chunks, reads)                          # forks: before the first device call
    if ffi.lib().jtk_lc_device_ok(0) != 1:
        sys.exit("no gfx950 device: nothing is measured here")
    api.map_reads(chunks[:10], reads[:10])
    got = api.map_reads(chunks, reads, cap=len(want) + 16)                # the warm-up call at this shape
    phases, host = {}, []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        got = api.map_reads(chunks, reads, cap=len(want) + 16)
        host.append(time.perf_counter() - t0)
        for name, v in api.map_timing().items():
            phases.setdefault(name, []).append(v)
    n_min, n_hits = phases["n_minimizers"][0], phases["n_hits"][0]
    t_min = len(api.sketch(chunks, K, W, cap=2 * len(chunks) * CHUNK_LEN // W)["hash"])
    est = traffic(n_bases, (t_min, n_min - t_min), n_hits)
    lines.append("  %d placements, %d minimizers (%d of the chunks: 1 in %.2f positions), %d hits"
                 % (len(got), n_min, t_min, (n_bases - (K - 1) * (len(chunks) + len(reads))) / n_min, n_hits))
    total = 0.0
    for name in ("sketch_ms", "index_ms", "hits_ms", "order_ms", "chain_ms", "compact_ms"):
        ms = statistics.median(phases[name])
        total += ms
        rate = " estimate %.2f B/base -> %.2f TB/s (HBM %.1f TB/s achievable)" % (est[name] / n_bases, est[name] / (ms * 1e-3) / 1e12, HBM_TBS) if est[name] else ""
        lines.append("  %-8s %s ms;%s" % (name[:-3], spread(phases[name]), rate))
    lines.append("  the two sketch kernels alone %s ms: %.2f TB/s of bases read; the rest of the sketch phase is the upload from pageable memory and a wait"
                 % (spread(phases["sketch_kernel_ms"]), n_bases / (statistics.median(phases["sketch_kernel_ms"]) * 1e-3) / 1e12))
    lines.append("  the six phases %.3f ms = %.2f Gbases/s; host clock around api.map_reads (packing, upload, the waits, copy back): %s s"
                 % (total, n_bases / (total * 1e-3) / 1e9, spread(host)))
    same = len(got) == len(want) and all((got[f] == want[f]).all() for f in PLACEMENT_FIELDS)
    lines.append("  numpy restatement on %d processes: %.2f s (%s placements as the device)" % (WORKERS, seconds, "the same" if same else "DIFFERENT"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
