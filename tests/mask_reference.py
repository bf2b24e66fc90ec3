"""Repeat masking restated in plain Python from haplotyper/src/repeat_masking.rs: the rolling KMers iterator, to_idx, the counts,
create_mask with both of its branches (and its out-of-range index as an exception), mask_repeats with the range list as the
reference keeps it, get_repetitive_kmer and RepeatAnnot::repetitiveness.  No numpy, nothing of jtk_amd: this is what the
device's answers are compared with, byte for byte.

A worked example, k = 3, on the 20 bases

    position  0  1  2  3  4  5  6  7  8  9 10 11 12 13 14 15 16 17 18 19
    base      A  C  G  A  C  G  A  C  G  T  T  T  N  A  A  C  G  T  A  C

Codes: A C G T = 0 1 2 3 forward and 3 2 1 0 complement, N = 0 in both.  Window 0 `ACG`: forward 0 + 1*4 + 2*16 = 36; reverse
(the complement of the last base lowest) cmp(G) + cmp(C)*4 + cmp(A)*16 = 1 + 8 + 48 = 57; the k-mer is 36.  `CGA`: forward
1 + 8 + 0 = 9, reverse 3 + 4 + 32 = 39 -> 9.  `GAC`: forward 2 + 0 + 16 = 18, reverse 2 + 12 + 16 = 30 -> 18.  `CGT`: forward
1 + 8 + 48 = 57, reverse 0 + 4 + 32 = 36 -> 36, the same k-mer as `ACG`, its reverse complement.  The 18 windows give

    36 9 18 36 9 18 36 36 | GTT 62/16 -> 16 | TTT 63/0 -> 0 | TTN 15/0 -> 0 | TNA 3/48 -> 3 | NAA 0/60 -> 0 | AAC 16/62 -> 16 |
    ACG 36 | CGT 36 | GTA 14/19 -> 14 | TAC 19/14 -> 14

(`TTN`: forward 3 + 12 + 0, reverse cmp(N) + cmp(T)*4 + cmp(T)*16 = 0: the reverse strand of a window with an N is NOT the
complement of its forward strand.)  Counts: 36 x 6, 0 x 3, and 9, 18, 16, 14 twice each, 3 once: total 7 distinct, 1 singleton,
M = 6.  With freq = 0.3 and min = 1: percentile = floor(6 * 0.7) = 4, below_min = 0, the counts above min in ascending order
are 2 2 2 2 3 6, thr = 3, and the mask is {36} -- the k-mer 0, counted exactly thr times, stays out.  Its hits are the windows
0, 3, 6, 7, 14, 15: the ranges (0, 0), then (0, 10) as 3, 6 and 7 extend it, then (14, 18): 14 bases,

    acgacgacgtTTNAacgtAC

With min = 3 the five k-mers counted 2 or 3 times are "below min", 4 < 5, and all six are taken.

test_mask_reference.py pins these numbers."""

BASE2BIT = [0] * 256
BASE2BITCMP = [0] * 256
for _b, _f, _c in (("A", 0, 3), ("C", 1, 2), ("G", 2, 1), ("T", 3, 0)):
    for _ch in (_b, _b.lower()):
        BASE2BIT[ord(_ch)] = _f
        BASE2BITCMP[ord(_ch)] = _c


class ReferencePanic(Exception):
    """where the reference indexes out of range (create_mask's counts[percentile])"""


def to_idx(w):
    """to_idx (:196-208) of the bytes w"""
    forward = sum(BASE2BIT[b] << (2 * i) for i, b in enumerate(w))
    reverse = sum(BASE2BITCMP[b] << (2 * i) for i, b in enumerate(reversed(w)))
    return min(forward, reverse)


def kmers(seq, k):
    """the KMers iterator (:39-85): the first window summed, every further one rolled"""
    assert 1 <= k <= 32
    if len(seq) < k:
        return
    forward = sum(BASE2BIT[b] << (2 * i) for i, b in enumerate(seq[:k]))
    reverse = sum(BASE2BITCMP[b] << (2 * i) for i, b in enumerate(reversed(seq[:k])))
    yield min(forward, reverse)
    mask = (1 << (2 * k)) - 1
    for base in seq[k:]:
        forward = (forward >> 2) | (BASE2BIT[base] << (2 * (k - 1)))
        reverse = (mask & (reverse << 2)) | BASE2BITCMP[base]
        yield min(forward, reverse)


def kmer_counting(reads, k):
    counts = {}
    for read in reads:
        for kmer in kmers(read, k):
            counts[kmer] = counts.get(kmer, 0) + 1
    return counts


def create_mask(reads, k, freq, min_count):
    """create_mask (:255-285): (the mask, thr, takes_all, total, num_singleton); ReferencePanic, with the last two as its
    arguments, where counts[percentile] is out of range"""
    counts = kmer_counting(reads, k)
    total = len(counts)
    num_singleton = sum(1 for c in counts.values() if c == 1)
    counts = {kmer: c for kmer, c in counts.items() if c != 1}
    percentile = int(float(len(counts)) * (1.0 - freq) // 1)
    below_min = sum(1 for c in counts.values() if c <= min_count)
    if percentile < below_min:
        return set(counts), 0, 1, total, num_singleton
    percentile -= below_min
    above = sorted(c for c in counts.values() if min_count < c)
    if percentile >= len(above):
        raise ReferencePanic(total, num_singleton)
    thr = above[percentile]
    return {kmer for kmer, c in counts.items() if c > thr}, thr, 0, total, num_singleton


def ascii_upper(seq):
    return bytes(b - 32 if 97 <= b <= 122 else b for b in seq)


def mask_repeats(seq, mask, k):
    """mask_repeats (:287-325) on a bytearray, in place, with its list of ranges; returns the sum of their lengths"""
    start, end = 0, 0
    ranges = []
    for idx, kmer in enumerate(kmers(bytes(seq), k)):
        if kmer in mask:
            if end < idx:
                ranges.append((start, end))
                start, end = idx, idx + k
            else:
                end = idx + k
    ranges.append((start, end))
    for s, e in ranges:
        for i in range(s, min(e, len(seq))):
            if 65 <= seq[i] <= 90:
                seq[i] += 32
    return sum(e - s for s, e in ranges)


def mask_repeat(reads, k, freq, min_count):
    """mask_repeat (:135-158) on a list of bytes: (the masked reads, the report, the mask as an ascending list, rc).  rc is 0, or
    -6 where the reference panics: the reads are then upper-cased and no more, and the report has its counts."""
    upper = [ascii_upper(r) for r in reads]
    report = dict(n_bases=sum(len(r) for r in reads), n_kmers=sum(max(len(r) - k + 1, 0) for r in reads), n_distinct=0, n_singleton=0,
                  n_masked_kmers=0, n_lower=0, thr=0, takes_all=0)
    try:
        mask, thr, takes_all, total, num_singleton = create_mask(upper, k, freq, min_count)
    except ReferencePanic as panic:
        report["n_distinct"], report["n_singleton"] = panic.args
        return upper, report, [], -6
    out, n_lower = [], 0
    for r in upper:
        seq = bytearray(r)
        n_lower += mask_repeats(seq, mask, k)
        out.append(bytes(seq))
    report.update(n_distinct=total, n_singleton=num_singleton, n_masked_kmers=len(mask), n_lower=n_lower, thr=thr, takes_all=takes_all)
    return out, report, sorted(mask), 0


def get_repetitive_kmer(reads, k):
    """get_repetitive_kmer (:109-134): to_idx of the windows whose bytes are all ASCII lower case, as an ascending list"""
    found = set()
    for r in reads:
        for i in range(len(r) - k + 1):
            w = r[i:i + k]
            if all(97 <= b <= 122 for b in w):
                found.add(to_idx(w))
    return sorted(found)


def repetitiveness(seq, k, kmer_set):
    """RepeatAnnot::repetitiveness (:90-105) as (numerator, denominator); the reference returns their f64 quotient"""
    counts = {}
    for kmer in kmers(seq, k):
        if kmer in kmer_set:
            counts[kmer] = counts.get(kmer, 0) + 1
    return sum(c for c in counts.values() if 1 < c), max(len(seq) - k, 0) + 1
