"""tests/mask_reference.py against values worked by hand -- the cases of the reference's own unit test (repeat_masking.rs:333-371)
and the 20-base example of its docstring -- and tests/mask_cases.py against what each case claims to exercise, with the reference
alone: a degenerate case must not hide a failure of the device test that runs on it."""
import pytest

import mask_cases as K
import mask_reference as R


def test_the_reference_unit_test():
    assert len(list(R.kmers(b"AAAA", 1))) == 4 and all(x == 0 for x in R.kmers(b"AAAA", 1)) and all(x == 0 for x in R.kmers(b"AAAA", 2))
    assert len(list(R.kmers(b"TTTT", 1))) == 4 and all(x == 0 for x in R.kmers(b"TTTT", 1)) and all(x == 0 for x in R.kmers(b"TTTT", 2))
    seq = b"CAGTGCAT"
    # CA: 1 + 0 / TG -> 3 + 2*4 = 11 -> 1; AG: 0 + 8 / CT -> 1 + 12 -> 8; GT: 2 + 12 / AC -> 0 + 4 -> 4; TG: 11 / CA: 1 -> 1;
    # GC: 2 + 4 = 6, its own reverse complement; CA -> 1; AT: 0 + 12, its own reverse complement
    assert list(R.kmers(seq, 2)) == [1, 8, 4, 1, 6, 1, 12]
    for k in (1, 2, 3, 8):
        got = list(R.kmers(seq, k))
        assert got == [R.to_idx(seq[i:i + k]) for i in range(len(seq) - k + 1)] and all(x < 1 << (2 * k) for x in got)
    assert list(R.kmers(seq, 9)) == [] and list(R.kmers(b"", 1)) == []


def test_a_byte_that_is_no_base_is_zero_on_both_strands():
    assert R.to_idx(b"TTN") == 0 and R.to_idx(b"TTA") == min(3 + 12 + 0, 3 + 0 + 0) and R.to_idx(b"TTC") == min(3 + 12 + 16, 2 + 0 + 0)
    assert R.to_idx(b"N[\x00\xff") == 0 and R.to_idx(b"nnnn") == 0 and R.to_idx(b"acgt") == R.to_idx(b"ACGT") == min(0 + 4 + 32 + 192, 0 + 4 + 32 + 192)


def test_the_worked_example_of_the_docstring():
    seq = b"ACGACGACGTTTNAACGTAC"
    assert list(R.kmers(seq, 3)) == [36, 9, 18, 36, 9, 18, 36, 36, 16, 0, 0, 3, 0, 16, 36, 36, 14, 14]
    mask, thr, takes_all, total, singletons = R.create_mask([seq], 3, 0.3, 1)
    assert (mask, thr, takes_all, total, singletons) == ({36}, 3, 0, 7, 1)
    out, report, mask_list, rc = R.mask_repeat([seq.lower()], 3, 0.3, 1)
    assert out == [b"acgacgacgtTTNAacgtAC"] and mask_list == [36] and rc == 0
    assert report == dict(n_bases=20, n_kmers=18, n_distinct=7, n_singleton=1, n_masked_kmers=1, n_lower=14, thr=3, takes_all=0)
    # min = 3: the k-mers counted 2, 2, 2, 2 and 3 times are "below min", 4 < 5: all six are taken
    assert R.create_mask([seq], 3, 0.3, 3)[:3] == ({36, 9, 18, 16, 0, 14}, 0, 1)
    # get_repetitive_kmer reads the case, not the mask: `cga` (9) and `gac` (18) were never masked, but lie in the run
    assert R.get_repetitive_kmer(out, 3) == [9, 18, 36]
    assert R.repetitiveness(out[0], 3, {36, 9, 18}) == (6 + 2 + 2, 18)
    assert R.repetitiveness(b"AC", 3, {36}) == (0, 1) and R.repetitiveness(b"", 3, {36}) == (0, 1)
    with pytest.raises(R.ReferencePanic):
        R.create_mask([seq], 3, 0.0, 1)
    with pytest.raises(R.ReferencePanic):
        R.create_mask([b"ACGTTGCA"], 5, 0.5, 0)


def test_the_range_list_is_the_union_of_the_hits():
    seq = bytearray(b"ACGACGACGTTTNAACGTAC")
    assert R.mask_repeats(seq, {36}, 3) == 14
    seq = bytearray(b"TTTACGTTTTACGACGTTT")   # hits at 3, 10, 13 (and CGT at 4, 14): (0, 0) is pushed, 10 + 3 == 13 merges
    assert R.mask_repeats(seq, {36}, 3) == 4 + 7 and bytes(seq) == b"TTTacgtTTTacgacgtTT"


@pytest.fixture(scope="module")
def answers():
    return {c["name"]: R.mask_repeat(c["reads"], c["k"], c["freq"], c["min_count"]) for c in K.CASES}


@pytest.mark.parametrize("case", K.CASES, ids=[c["name"] for c in K.CASES])
def test_a_case_exercises_what_it_claims(case, answers):
    out, report, mask, rc = answers[case["name"]]
    upper = [R.ascii_upper(r) for r in case["reads"]]
    assert [o.upper() for o in out] == [u.upper() for u in upper] and report["n_bases"] == sum(len(r) for r in case["reads"])
    if case["expect"] == "panic":
        assert rc == -6 and out == upper and mask == [] and report["n_lower"] == 0
        return
    assert rc == 0 and report["n_masked_kmers"] == len(mask) > 0
    counts = R.kmer_counting(upper, case["k"])
    if case["expect"] == "takes_all":
        assert report["takes_all"] == 1 and report["thr"] == 0 and len(mask) == report["n_distinct"] - report["n_singleton"]
        return
    assert report["takes_all"] == 0 and 0 < report["n_lower"] < report["n_bases"]
    assert sum(1 for c in counts.values() if c == report["thr"]) >= 1 and report["thr"] > case["min_count"]
    lower = sum(1 for o in out for b in o if 97 <= b <= 122)
    assert lower <= report["n_lower"]    # the sum counts covered bytes that are no letters too


def test_the_named_cases(answers):
    by_name = {c["name"]: c for c in K.CASES}
    out, report, mask, _ = answers["ties_at_thr"]
    counts = R.kmer_counting(by_name["ties_at_thr"]["reads"], 12)
    assert report["thr"] == 4 and sum(1 for c in counts.values() if c == 4) >= 20 and all(counts[m] > 4 for m in mask)
    assert sum(1 for m in mask if counts[m] == 9) >= 40                  # the unit planted 9 times
    assert sum(1 for c in counts.values() if 1 < c <= 2) > 0           # below_min is not empty, and the percentile is past it
    for k in (12, 31):     # the mask of a boundaries case is its unit, and the few windows of k - 1 of its bases and one more
        c = by_name["boundaries_k%d" % k]
        out, report, mask, _ = answers[c["name"]]
        assert R.to_idx(c["reads"][0]) in mask and len(mask) < 12 and report["thr"] == 2
        at63 = out[8]
        assert at63[:50].isupper() and at63[63:63 + k].islower() and at63[63 + k + 13:].isupper()
        merged = out[9]
        assert merged[40:40 + 2 * k].islower() and merged[:27].isupper() and merged[40 + 2 * k + 13:].isupper()
        assert out[10][:k].islower() and out[11][-k:].islower() and out[-1][-k:].islower()
    for k in K.KS:                                                         # N and A collide on k-mer 0
        c = by_name["shapes_k%d" % k]
        counts = R.kmer_counting(c["reads"], k)
        assert counts[0] >= 2 * (100 - k + 1) and {len(r) for r in c["reads"]} >= {0, k - 1, k, k + 1, 63, 64, 65, 127, 128, 129}
        assert any(len(r) > 2 * K.TILE for r in c["reads"])
    assert answers["planted_genome"][1]["thr"] > 10


@pytest.mark.parametrize("case", K.REP_CASES, ids=[c[0] for c in K.REP_CASES])
def test_repetitiveness_cases(case):
    name, seqs, k, kmers = case
    got = [R.repetitiveness(s, k, set(kmers)) for s in seqs]
    assert all(den == max(len(s) - k, 0) + 1 for (_, den), s in zip(got, seqs))
    if name.startswith("empty_set") or not seqs:
        assert all(num == 0 for num, _ in got)
        return
    assert got[0][0] == 3 and got[1][0] == 0 and got[2][0] == 0 and got[3] == (0, 1) and got[4] == (0, 1) and got[5][0] >= 2
    assert got[6][0] == (70 - k + 1 if name.startswith("with_zero") else 0)
