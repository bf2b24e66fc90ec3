"""The cases of jtk_lc_sketch and jtk_lc_map_reads: the smallest shapes at which the kernels of map.hip can go wrong.  A workgroup
owns TILE = 1,024 k-mer positions of a sequence, so a sequence of TILE + k - 1 bases is exactly one tile.  Everything is drawn
from seeded generators; nothing here comes from the device."""
import random

import map_reference as R

TILE = 1024
_RC = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def rc(s):
    return s.translate(_RC)[::-1]


def rand_seq(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def mutate(seg, rate, rng):
    """substitutions, insertions and deletions in equal parts; -> (the read, where[i] = the read position of base i of seg,
    where[len(seg)] = the read's length)"""
    out, where = bytearray(), []
    for b in seg:
        where.append(len(out))
        u = rng.random()
        if u < rate / 3:
            out.append(rng.choice([c for c in b"ACGT" if c != b]))
        elif u < 2 * rate / 3:
            out.append(rng.choice(b"ACGT"))
            out.append(b)
        elif u < rate:
            pass
        else:
            out.append(b)
    where.append(len(out))
    return bytes(out), where


def planted(seed, rates=(0.0, 0.05, 0.10), n_reads=12, genome_len=20000, chunk_len=2000, n_chunks=5):
    """Five 2,000-base chunks cut from a random 20 kbase genome and twelve reads of 5-7 kbases from either strand.
    -> dict(chunks, reads, truth, unrelated): truth[r] = {chunk: (start, end, is_forward)} for every chunk that lies wholly inside
    read r, the span in the read's own coordinates; unrelated = a read drawn from another genome; origin[r] = the genome interval
    read r was drawn from, starts[c] = where chunk c begins in the genome."""
    rng = random.Random(seed)
    genome = rand_seq(rng, genome_len)
    starts = [1000 + i * (genome_len // n_chunks) for i in range(n_chunks)]
    chunks = [genome[s:s + chunk_len] for s in starts]
    reads, truth, origin = [], [], []
    for r in range(n_reads):
        length = rng.randrange(5000, 7001)
        at = rng.randrange(0, genome_len - length + 1)
        read, where = mutate(genome[at:at + length], rates[r % len(rates)], rng)
        forward = r % 2 == 0
        spans = {}
        for c, s in enumerate(starts):
            if at <= s and s + chunk_len <= at + length:
                lo, hi = where[s - at], where[s + chunk_len - at]
                spans[c] = (lo, hi, 1) if forward else (len(read) - hi, len(read) - lo, 0)
        reads.append(read if forward else rc(read))
        truth.append(spans)
        origin.append((at, at + length))
    other = random.Random(seed + 7919)
    return dict(chunks=chunks, reads=reads, truth=truth, unrelated=rand_seq(other, 6000), origin=origin, starts=starts)


PLANTED_SEEDS = {0.0: 11, 0.05: 12, 0.10: 13}     # one planted set per error rate (test_map_reference.py checks the conditions on each)


def planted_at(rate):
    return planted(PLANTED_SEEDS[rate], rates=(rate,))


def _sketch_seqs(k, w, rng):
    seam = bytearray(rand_seq(rng, 2 * TILE + 40))
    unit = rand_seq(rng, 6)
    for i in range(TILE - 30, TILE + 30):               # a period-6 repeat across the seam: hashes tie inside a window
        seam[i] = unit[i % 6]
    n_run = bytearray(rand_seq(rng, TILE + 200))
    for i in range(TILE - 9, TILE + 12):                # a run of N across the seam
        n_run[i] = ord("N")
    homo_seam = bytearray(rand_seq(rng, TILE + 300))
    for i in range(TILE - 40, TILE + 60):               # every position ties, across the seam
        homo_seam[i] = ord("A")
    lower = bytearray(rand_seq(rng, 700))
    lower[100:400] = bytes(lower[100:400]).lower()
    seqs = [b"", rand_seq(rng, k - 1), rand_seq(rng, k), rand_seq(rng, k + w - 2), rand_seq(rng, k + w - 1),
            rand_seq(rng, TILE + k - 1), rand_seq(rng, TILE + k - 2), rand_seq(rng, TILE + k), rand_seq(rng, 2 * TILE + k),
            bytes(seam), bytes(n_run), bytes(homo_seam), bytes(lower), b"A" * 300, b"ACGT" * 80, b"NNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNN",
            rand_seq(rng, 50) + b"n" + rand_seq(rng, 50) + b"[" + rand_seq(rng, 50)]
    return seqs


SKETCH_CASES = []
for _k, _w in ((15, 1), (15, 5), (15, 10), (15, 20), (17, 1), (17, 5), (17, 10), (17, 64), (16, 10), (1, 1), (31, 3)):
    SKETCH_CASES.append(dict(name="k%d_w%d" % (_k, _w), k=_k, w=_w, seqs=_sketch_seqs(_k, _w, random.Random(1000 * _k + _w))))
# The one case that stages all of a tile's span: a middle tile with w - 1 positions of halo on both sides needs a sequence of
# 2 * TILE + w k-mer positions or more (the longest above has 2 * TILE + 10 at k = 31).  Its last sequence is the long one.
_rng = random.Random(1000 * 31 + 64)
SKETCH_CASES.append(dict(name="k31_w64", k=31, w=64, seqs=_sketch_seqs(31, 64, _rng) + [rand_seq(_rng, 3 * TILE + 31)]))

DEFAULTS = dict(k=15, w=10, max_occ=200, max_gap=100, min_seeds=4, skip_self=False)


def _case(name, targets, queries, **params):
    return dict(name=name, targets=list(targets), queries=list(queries), params=dict(DEFAULTS, **params))


def _map_cases():
    cases = []
    rng = random.Random(4242)
    p5 = planted_at(0.05)
    lowered = list(p5["reads"])
    lowered[1] = lowered[1][:900] + lowered[1][900:2500].lower() + lowered[1][2500:]
    lowered[4] = lowered[4].lower()
    for rate in (0.0, 0.05, 0.10):
        p = planted_at(rate)
        cases.append(_case("planted_%d" % round(100 * rate), p["chunks"], p["reads"] + [p["unrelated"]]))
    cases.append(_case("planted_k17", p5["chunks"], p5["reads"], k=17))
    cases.append(_case("planted_w1", p5["chunks"][:2], p5["reads"][:4], w=1))
    cases.append(_case("planted_w5_k17", p5["chunks"], p5["reads"][:6], k=17, w=5))
    cases.append(_case("planted_w20", p5["chunks"], p5["reads"][:6], w=20))
    cases.append(_case("lower_case", [p5["chunks"][0].lower()] + p5["chunks"][1:], lowered))
    # queries without a hit first, in the middle and last; a target without one too
    none = [rand_seq(rng, 3000) for _ in range(3)]
    cases.append(_case("no_hit_queries", p5["chunks"] + [rand_seq(rng, 2000)], [none[0], p5["reads"][0], none[1], p5["reads"][1], none[2], b"", b"ACGT"]))
    cases.append(_case("no_hit_at_all", p5["chunks"][:2], none))
    cases.append(_case("empty_sides", [b"", b"ACG"], [b"", b"ACGTAC"]))
    # the same chunk twice in tandem on one strand: two placements
    chunk = rand_seq(rng, 600)
    tandem = rand_seq(rng, 500) + chunk + chunk + rand_seq(rng, 500)
    cases.append(_case("tandem", [chunk], [tandem, rc(tandem)]))
    # two copies whose diagonals lie exactly max_gap and max_gap + 1 apart: one cluster (whose seeds are counted once), then two
    short = rand_seq(rng, 80)
    for gap in (100, 101):
        read = rand_seq(rng, 200) + short + rand_seq(rng, gap - 80) + short + rand_seq(rng, 200)
        cases.append(_case("diagonals_%d_apart" % gap, [short], [read, rc(read)], w=5))
    # a homopolymer: every position ties and every k-mer is the same one; max_occ at its occurrence count and one below.  With it
    # one cluster of 286 x 286 hits: more than a wave, more than a workgroup
    homo = b"A" * 300
    cases.append(_case("homopolymer_kept", [homo], [homo, rc(homo), homo.lower()], max_occ=286))
    cases.append(_case("homopolymer_dropped", [homo], [homo], max_occ=285))
    cases.append(_case("more_than_a_wave", [p5["chunks"][0][:400]], [p5["chunks"][0][:400] + rand_seq(rng, 50)], w=1, min_seeds=1))
    # a cluster with min_seeds - 1 seeds is not reported, one with min_seeds is
    piece = p5["chunks"][1][:120]
    read =rand_seq(rng, 300) + piece + rand_seq(rng, 300)
    seeds = max(f["n_seeds"] for f in R.map_reads([piece], [read], **dict(DEFAULTS, min_seeds=1)))
    cases.append(_case("one_seed_short", [piece], [read], min_seeds=seeds + 1))
    cases.append(_case("just_enough_seeds", [piece], [read], min_seeds=seeds))
    # chunk against chunk: overlapping pieces of one genome, skip_self on and off
    genome = rand_seq(rng, 6000)
    pieces = [genome[s:s + 2000] for s in (0, 1000, 2000, 3500)] + [rc(genome[500:2500])]
    cases.append(_case("skip_self", pieces, pieces, skip_self=True))
    cases.append(_case("not_skip_self", pieces, pieces))
    cases.append(_case("max_gap_0", p5["chunks"][:2], p5["reads"][:3], max_gap=0, min_seeds=1))
    return cases


MAP_CASES = _map_cases()
