"""jtk_lc_mask_repeats, jtk_lc_repetitive_kmers and jtk_lc_repetitiveness on the device against tests/mask_reference.py on every case
of tests/mask_cases.py: the masked bytes, every field of the report, the mask, rc, the repetitive k-mers and the numerators and
denominators are EQUAL -- everything is an integer or a byte, so there is no tolerance."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mask_cases as K
import mask_reference as R
from jtk_amd import api, ffi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [c["name"] for c in K.CASES]
FIELDS = ffi.MASK_REPORT_DT.names


@pytest.fixture(scope="module")
def reference():
    return {c["name"]: R.mask_repeat(c["reads"], c["k"], c["freq"], c["min_count"]) for c in K.CASES}


@pytest.fixture(scope="module")
def device(jtk_lib):
    return {c["name"]: api.mask_repeats(c["reads"], c["k"], c["freq"], c["min_count"]) for c in K.CASES}


@pytest.mark.parametrize("case", K.CASES, ids=IDS)
def test_mask_repeats_equals_the_reference(case, reference, device):
    want_reads, want_report, want_mask, want_rc = reference[case["name"]]
    got_reads, got_report, got_mask = device[case["name"]]
    assert got_report["rc"] == want_rc
    assert {f: got_report[f] for f in FIELDS} == want_report
    assert got_mask.dtype == np.uint64 and got_mask.tolist() == want_mask
    assert len(got_reads) == len(want_reads)
    for i, (g, w) in enumerate(zip(got_reads, want_reads)):
        assert g == w, (i, len(w))


@pytest.mark.parametrize("case", K.CASES, ids=IDS)
def test_repetitive_kmers_and_repetitiveness_equal_the_reference(case, reference, device):
    k = case["k"]
    for reads in (device[case["name"]][0], case["reads"]):     # the masked reads, and the input as given (lower case, n, [ in it)
        want = R.get_repetitive_kmer(reads, k)
        got = api.repetitive_kmers(reads, k, cap=4)             # too small wherever there is more to return: the second call
        assert got.dtype == np.uint64 and got.tolist() == want
        num, den = api.repetitiveness(reads, k, got, parts=True)
        pairs = [R.repetitiveness(r, k, set(want)) for r in reads]
        assert num.tolist() == [p[0] for p in pairs] and den.tolist() == [p[1] for p in pairs]
        ratio = api.repetitiveness(reads, k, got)
        assert ratio.dtype == np.float64 and ratio.tolist() == [p[0] / p[1] for p in pairs]


@pytest.mark.parametrize("case", K.REP_CASES, ids=[c[0] for c in K.REP_CASES])
def test_repetitiveness_cases(case, jtk_lib):
    _, seqs, k, kmers = case
    num, den = api.repetitiveness(seqs, k, kmers, parts=True)
    pairs = [R.repetitiveness(s, k, set(kmers)) for s in seqs]
    assert num.tolist() == [p[0] for p in pairs] and den.tolist() == [p[1] for p in pairs]


def flat(reads):
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads], dtype=np.uint64)
    return np.frombuffer(b"".join(reads), dtype=np.uint8).copy(), off


def test_in_place_and_a_mask_capacity_that_is_too_small(jtk_lib, reference):
    case = next(c for c in K.CASES if c["name"] == "ties_at_thr")
    want_reads, want_report, want_mask, _ = reference[case["name"]]
    bases, off = flat(case["reads"])
    report = np.zeros(1, dtype=ffi.MASK_REPORT_DT)
    small = np.full(3, 7, dtype=np.uint64)
    assert len(want_mask) > 3
    out = np.zeros(len(bases), dtype=np.uint8)
    rc = jtk_lib.jtk_lc_mask_repeats(len(case["reads"]), ffi.u8p(bases), ffi.u64p(off), case["k"], case["freq"], case["min_count"], ffi.u8p(out),
                                     ffi.u64p(small), 3, report.ctypes.data, 0)
    assert rc == -1 and int(report["n_masked_kmers"][0]) == len(want_mask) and small.tolist() == [7, 7, 7]
    assert out.tobytes() == b"".join(want_reads) and {f: int(report[f][0]) for f in FIELDS} == want_report     # the rest is valid
    # the second call, in place, without asking for the mask, then with room for it
    rc = jtk_lib.jtk_lc_mask_repeats(len(case["reads"]), ffi.u8p(bases), ffi.u64p(off), case["k"], case["freq"], case["min_count"], ffi.u8p(bases),
                                     None, 0, report.ctypes.data, 0)
    assert rc == 0 and bases.tobytes() == b"".join(want_reads) and int(report["n_masked_kmers"][0]) == len(want_mask)
    mask = np.zeros(len(want_mask), dtype=np.uint64)
    rc = jtk_lib.jtk_lc_mask_repeats(len(case["reads"]), ffi.u8p(bases), ffi.u64p(off), case["k"], case["freq"], case["min_count"], ffi.u8p(bases),
                                     ffi.u64p(mask), len(mask), report.ctypes.data, 0)
    assert rc == 0 and mask.tolist() == want_mask and bases.tobytes() == b"".join(want_reads)   # masking a masked read again changes nothing
    assert api.mask_repeats(case["reads"], case["k"], case["freq"], case["min_count"], mask_cap=1)[2].tolist() == want_mask
    timing = api.mask_timing()
    assert set(timing) == {"emit_ms", "sort_ms", "select_ms", "apply_ms"} and all(v > 0 for v in timing.values())


def test_a_set_that_is_not_ascending_is_refused(jtk_lib):
    for kmers in ([5, 5], [9, 2], [1, 2, 3, 3, 4]):
        with pytest.raises(ffi.JtkError) as err:
            api.repetitiveness([b"ACGTACGTACGTACGT"], 4, kmers)
        assert err.value.status == -1
    assert api.repetitiveness([b"ACGTACGTACGTACGT"], 4, [R.to_idx(b"ACGT")], parts=True)[0].tolist() == [4]


def data_set(reads):
    hmm = {n: 0.0 for n in ("mat_mat", "mat_ins", "mat_del", "ins_mat", "ins_ins", "ins_del", "del_mat", "del_ins", "del_del")}
    hmm.update(mat_emit=[0.0] * 16, ins_emit=[0.0] * 20)
    return {"input_file": "reads.fa", "masked_kmers": {"k": 15, "thr": 77}, "coverage": "NotAvailable",
            "raw_reads": [{"name": "r%d" % i, "desc": "", "id": i, "seq": r.decode("latin-1")} for i, r in enumerate(reads)], "hic_pairs": [],
            "selected_chunks": [], "encoded_reads": [], "hic_edges": [], "read_type": "CLR", "model_param": {"forward": hmm, "reverse": dict(hmm)},
            "error_rate": {n: 0.0 for n in ("del", "del_sd", "ins", "ins_sd", "mismatch", "mism_sd", "total", "total_sd")}, "processed_stages": []}


def test_the_stage_gives_the_reference_json(tmp_path, reference):
    case = next(c for c in K.CASES if c["name"] == "planted_genome")
    reads = [r for r in case["reads"][:150]]
    want_reads, want_report, want_mask, rc = R.mask_repeat(reads, 12, 0.02, 10)
    assert rc == 0 and 0 < want_report["n_lower"] < want_report["n_bases"]
    ds = data_set(reads)
    src, dst = tmp_path / "in.json", tmp_path / "out.json"
    src.write_text(json.dumps(ds))
    run = subprocess.run([sys.executable, "-m", "jtk_amd.dataset", "--stage", "mask_repeat", "--kmersize", "12", "--top-freq", "0.02", "--min-count",
                          "10", "-v", str(src), str(dst)], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stderr
    want = data_set(want_reads)
    want["masked_kmers"]["k"] = 12
    assert json.loads(dst.read_text()) == want
    assert [l for l in run.stderr.splitlines() if l.startswith("MASKREPEAT")] == [
        "MASKREPEAT\tMaskLen\t12\t%d" % len(want_mask), "MASKREPEAT\tTotalMask\t%d\t%d" % (want_report["n_lower"], want_report["n_bases"]),
        "MASKREPEAT\tMaskedKmers\t%d\t12" % len(want_mask)]
