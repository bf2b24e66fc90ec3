"""The inputs of the repeat-masking tests: small and deterministic (the stdlib's random with fixed seeds), each at most about
200,000 bases.  CASES is a list of dicts: name, reads (bytes), k, freq, min_count, and `expect`: "normal" (the percentile branch,
some but not all bases masked), "takes_all", or "panic" (the reference indexes out of range).  test_mask_reference.py checks on
the CPU, with the reference alone, that every case is what it says it is; test_gpu_mask.py runs the device on all of them.
REP_CASES are (name, seqs, k, kmers) for repetitiveness."""
import random

KS = (1, 2, 12, 15, 16, 17, 31)     # 16 / 17: 32-bit and 64-bit keys; even k has reverse-complement palindromes
TILE = 2048                         # bases per workgroup of mask.hip; a wave ballots 64 positions

_COMP = {65: 84, 67: 71, 71: 67, 84: 65}


def rnd(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def revcomp(seq):
    return bytes(_COMP[b] for b in reversed(seq))


def case(name, reads, k, freq, min_count, expect):
    assert sum(len(r) for r in reads) <= 220_000, name
    return dict(name=name, reads=[bytes(r) for r in reads], k=k, freq=freq, min_count=min_count, expect=expect)


def shapes(k):
    """every read length that matters, bytes that are no bases, both strands, N against A; units planted 8 and 3 times so that
    the counts differ"""
    rng = random.Random(1000 + k)
    unit8, unit3 = rnd(rng, max(60, 2 * k + 10)), rnd(rng, max(60, 2 * k + 10))
    reads = [rnd(rng, n) for n in (0, k - 1, k, k + 1, 63, 64, 65, 127, 128, 129)]
    long = b"".join(rnd(rng, 400) + u for u in [unit8] * 6 + [unit3] * 2) + rnd(rng, 500)      # about 5,000 bases: three tiles
    reads.append(long)
    odd = bytearray(rnd(rng, 80) + unit8 + rnd(rng, 80) + unit3 + rnd(rng, 80))
    for pos, b in ((5, 78), (6, 78), (40, 110), (41, 0), (42, 255), (60, 91), (100, 78), (200, 110), (len(odd) - 1, 78)):   # N n 0x00 0xFF [
        odd[pos] = b
    reads.append(bytes(odd))
    reads.append((rnd(rng, 70) + unit8 + rnd(rng, 70)).lower())                               # lower-case input
    strand = rnd(rng, 300)
    reads += [strand, revcomp(strand)]
    reads += [b"N" * 100, b"A" * 100, b"n" * 40 + b"t" * 40]                                   # all of them k-mer 0
    freq = {1: 1.0, 2: 0.5}.get(k, 0.25)
    return case("shapes_k%d" % k, reads, k, freq, 0, "normal")


def boundaries(k):
    """one unit of exactly k bases is the whole mask (freq = 1.0: thr is the smallest repeated count, the decoy's); it is put
    where the cover has to cross a ballot word, a tile, or nothing at all"""
    rng = random.Random(2000 + k)
    unit, decoy = rnd(rng, k), rnd(rng, k)
    reads = [unit] * 6 + [decoy] * 2                                             # reads of one k-mer each (two random 12-mers of
                                                                                 # the 40,000 bases below can be equal: thr is 2)
    reads.append(rnd(rng, 63) + unit + rnd(rng, 70))                             # a hit at position 63: the cover spills k - 1 bases into the next word
    reads.append(rnd(rng, 40) + unit + unit + rnd(rng, 40))                      # hits at idx and idx + k: the reference merges the ranges
    reads.append(unit + rnd(rng, 50))                                            # a hit at position 0
    reads.append(rnd(rng, 50) + unit)                                            # at the last k-mer of a read
    for at in (TILE - k - 1, TILE - k, TILE - k + 1, TILE - 18 if k > 18 else TILE - 1, TILE - 1, TILE, TILE + 1, 2 * TILE - 1):
        reads.append(rnd(rng, at) + unit + rnd(rng, 5000 - at - k))              # around the tile boundary, about 5,000 bases each
    reads.append(rnd(rng, 64 - k) + unit + rnd(rng, 64 - k) + unit)             # hits that end exactly with a word, and with the read
    reads.append(rnd(rng, 100) + unit)                                           # the last k-mer of the last read
    return case("boundaries_k%d" % k, reads, k, 1.0, 0, "normal")


def planted_units(rng, k, copies):
    """reads that hold a unit of 40 + k bases `c` times for every c of copies, random bases between"""
    reads = []
    for c in copies:
        unit = rnd(rng, 40 + k)
        reads += [rnd(rng, 30) + unit + rnd(rng, 30) for _ in range(c)]
    return reads


def thresholds():
    out = []
    rng = random.Random(3000)
    # every repeated k-mer is counted at most 10 times: all are "below min", percentile = floor(M * 0.999) < M = below_min
    out.append(case("takes_all", planted_units(rng, 12, (2, 3, 5, 9)), 12, 0.001, 10, "takes_all"))
    # units counted 2, 4, 4 and 9 times: below_min is the first unit's k-mers, the percentile falls among the k-mers counted 4
    # times -- dozens tied at thr -- and only the last unit is masked
    out.append(case("ties_at_thr", planted_units(rng, 12, (2, 4, 4, 9)), 12, 0.4, 2, "normal"))
    out.append(case("min_count_0", planted_units(rng, 15, (2, 3, 7)), 15, 0.5, 0, "normal"))
    out.append(case("freq_1", planted_units(rng, 17, (2, 2, 6)), 17, 1.0, 0, "normal"))
    out.append(case("freq_1_min_above_some", planted_units(rng, 16, (2, 5, 6)), 16, 1.0, 2, "takes_all"))
    out.append(case("panic_no_repeat", [rnd(rng, 200)], 15, 0.001, 10, "panic"))
    out.append(case("panic_freq_0", planted_units(rng, 12, (2, 4, 9)), 12, 0.0, 2, "panic"))
    out.append(case("panic_freq_tiny", planted_units(rng, 12, (2, 4)), 12, 1e-300, 0, "panic"))
    out.append(case("panic_no_reads", [], 12, 0.001, 10, "panic"))
    out.append(case("panic_short_reads", [b"ACGT", b"", b"ACGTACGTACG"], 12, 0.5, 0, "panic"))
    return out


def planted_genome():
    """a random genome of 3 kbp with a 60-base repeat planted 8 times, about 300 reads from both strands with 1 % substitutions"""
    rng = random.Random(4000)
    repeat = rnd(rng, 60)
    genome = b"".join(rnd(rng, 315) + repeat for _ in range(8)) + rnd(rng, 315)
    reads = []
    for _ in range(300):
        n = rng.randrange(150, 400)
        at = rng.randrange(0, len(genome) - n)
        r = bytearray(genome[at:at + n])
        for i in range(n):
            if rng.random() < 0.01:
                r[i] = rng.choice(b"ACGT")
        reads.append(bytes(r) if rng.random() < 0.5 else revcomp(bytes(r)))
    return case("planted_genome", reads, 12, 0.02, 10, "normal")


CASES = [shapes(k) for k in KS] + [boundaries(k) for k in (2, 12, 16, 17, 31)] + thresholds() + [planted_genome()]


def rep_cases():
    rng = random.Random(5000)
    out = []
    for k in (8, 12, 16, 17, 31):
        from_set, other = rnd(rng, k), rnd(rng, k)
        seqs = [
            rnd(rng, 20) + from_set + rnd(rng, 15) + from_set + rnd(rng, 9) + revcomp(from_set) + rnd(rng, 20),   # twice forward, once reverse: 3
            rnd(rng, 10) + from_set + rnd(rng, 10),          # a member, once: nothing
            rnd(rng, 50) + other + rnd(rng, 5) + other,      # no member, though a k-mer repeats
            rnd(rng, k - 1), b"",                            # shorter than k: 0 / 1
            rnd(rng, 2500) + from_set * 2 + rnd(rng, 2500),  # across tiles
            b"N" * 70,                                       # k-mer 0, which the second set holds
        ]
        members = {min(_fwd(from_set), _fwd_rc(from_set))}
        out.append(("one_member_k%d" % k, seqs, k, sorted(members)))
        out.append(("with_zero_k%d" % k, seqs, k, sorted(members | {0})))
        out.append(("empty_set_k%d" % k, seqs, k, []))
    out.append(("no_sequences", [], 12, [5, 9]))
    return out


def _fwd(w):
    return sum(b"ACGT".index(b) << (2 * i) for i, b in enumerate(w))


def _fwd_rc(w):
    return _fwd(revcomp(w))


REP_CASES = rep_cases()
