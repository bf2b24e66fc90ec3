"""tests/map_reference.py against properties that do not come from it: the hash is a bijection, a sequence and its reverse
complement select the same k-mers, w = 1 keeps every valid k-mer, a brute-force definition of "attains a window's minimum"
agrees, and on the planted set every chunk that lies inside a read is placed on the right strand with a window that holds it."""
import random

import pytest

import map_cases as K
import map_reference as R


def test_the_worked_example_of_the_docstring():
    assert [R.canonical(b"ACGGT", p, 3) for p in range(3)] == [(36, 0), (37, 1), (20, 1)]
    assert R.canonical(b"ACNGT", 0, 3) is None and R.canonical(b"ACGT", 0, 4) is None and R.canonical(b"acgGt", 1, 3) == (37, 1)


@pytest.mark.parametrize("k", (1, 2, 3, 5, 7))
def test_the_hash_is_a_bijection(k):
    assert sorted(R.hash_kmer(x, k) for x in range(4 ** k)) == list(range(4 ** k))


def test_the_hash_stays_in_2k_bits_and_spreads():
    rng = random.Random(5)
    for k in (15, 17, 31):
        xs = [rng.randrange(4 ** k) for _ in range(2000)]
        hs = [R.hash_kmer(x, k) for x in xs]
        assert all(0 <= h < 4 ** k for h in hs) and len(set(hs)) == len(set(xs))
        assert 800 < sum(h >> (2 * k - 1) for h in hs) < 1200             # the top bit is a coin


def special_sequences(rng):
    mixed = bytearray(K.rand_seq(rng, 400))
    mixed[50:60] = b"NNNNNNNNNN"
    mixed[200:300] = bytes(mixed[200:300]).lower()
    return [K.rand_seq(rng, 500), bytes(mixed), b"A" * 120, b"ACGT" * 40, b"AC" * 60, b"N" * 50, b"", b"ACG", K.rand_seq(rng, 16), K.rand_seq(rng, 25)]


def brute_force(seq, k, w):
    """the definition, O(n w): every window, its minimum over the valid k-mers, every position of the window that attains it"""
    hs = R.hashes(seq, k)
    n = len(hs)
    if n <= 0:
        return []
    windows = [range(0, n)] if n < w else [range(j, j + w) for j in range(n - w + 1)]
    keep = set()
    for win in windows:
        valid = [hs[p][0] for p in win if hs[p] is not None]
        if valid:
            keep.update(p for p in win if hs[p] is not None and hs[p][0] == min(valid))
    return [(p, hs[p][0], hs[p][1]) for p in sorted(keep)]


@pytest.mark.parametrize("k,w", [(15, 10), (17, 5), (16, 10), (4, 3), (15, 1), (15, 20), (9, 64)])
def test_sketch_against_the_definition_and_the_reverse_complement(k, w):
    rng = random.Random(100 * k + w)
    for seq in special_sequences(rng):
        got = R.sketch(seq, k, w)
        assert got == brute_force(seq, k, w)
        back = R.sketch(K.rc(seq), k, w)
        assert sorted((len(seq) - k - p, h, 1 - s) for p, h, s in back) == got
        if w == 1:
            assert [p for p, _, _ in got] == [p for p, h in enumerate(R.hashes(seq, k)) if h is not None]
    if k == 16:
        hs = R.hashes(b"ACGT" * 40, k)                           # ACGT.. and GTAC.. are their own reverse complements: no strand
        assert all((h is None) == (p % 2 == 0) for p, h in enumerate(hs)) and all(p % 2 for p, _, _ in R.sketch(b"ACGT" * 40, k, w))
        assert R.sketch(b"AT" * 40, k, w) == [] and R.sketch(b"AT" * 40, 15, w) != []
    assert R.sketch(b"N" * 50, k, w) == [] and R.sketch(b"ACG", 4, w) == []


def test_the_full_span_case_stages_a_full_span():
    """k31_w64: from the lengths alone, a sequence whose middle tile has w - 1 staged positions on both sides (the existing cases
    have none: their longest have 2,058 positions at k = 31 and 2,072 at (17, 64), the threshold is 2,112); on that sequence
    the reference agrees with the definition"""
    case = next(c for c in K.SKETCH_CASES if c["name"] == "k31_w64")
    k, w, seq = case["k"], case["w"], case["seqs"][-1]
    assert (k, w, len(seq)) == (31, 64, 3 * K.TILE + 31) and len(case["seqs"]) == 18
    assert max(len(s) - k + 1 for s in case["seqs"]) == len(seq) - k + 1 >= 2 * K.TILE + w
    assert R.sketch(seq, k, w) == brute_force(seq, k, w)


def test_occurrence_cut_and_skip_self():
    homo = b"A" * 300
    assert [p["n_seeds"] for p in R.map_reads([homo], [homo], max_occ=286)] == [286] and R.map_reads([homo], [homo], max_occ=285) == []
    rng = random.Random(9)
    seqs = [K.rand_seq(rng, 800) for _ in range(3)]
    assert [(p["query"], p["target"]) for p in R.map_reads(seqs, seqs)] == [(0, 0), (1, 1), (2, 2)]
    assert R.map_reads(seqs, seqs, skip_self=True) == []
    for p in R.map_reads(seqs, [K.rc(s) for s in seqs]):
        assert p["is_forward"] == 0 and (p["qstart"], p["qend"]) == (800 - p["oq_end"], 800 - p["oq_start"]) and p["diag_lo"] == p["diag_hi"] == 0


@pytest.mark.parametrize("rate", sorted(K.PLANTED_SEEDS))
def test_the_planted_set(rate):
    p = K.planted_at(rate)
    reads = p["reads"] + [p["unrelated"]]
    got = R.map_reads(p["chunks"], reads)
    trials = {t[0]: t for t in R.map_trials(got, [len(r) for r in reads], [len(c) for c in p["chunks"]], 0.3)}
    n_true, least = 0, None
    for r, spans in enumerate(p["truth"]):
        for c, (lo, hi, forward) in spans.items():
            hits = [i for i, g in enumerate(got) if (g["query"], g["target"], g["is_forward"]) == (r, c, forward) and i in trials]
            holds = [i for i in hits if trials[i][1] <= lo and hi <= trials[i][2]]
            assert holds, (r, c)
            n_true += 1
            least = min([got[i]["n_seeds"] for i in holds] + ([least] if least is not None else []))
    assert n_true >= 10 and least >= 2 * 4                        # (the defaults' min_seeds is 4)
    assert not any(g["query"] == len(reads) - 1 for g in got)
    assert {f for g in got for f in g} == set(R.FIELDS)
