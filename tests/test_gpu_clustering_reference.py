"""jtk_lc_cluster_features (mcmc_kernels.hip) against tests/clustering_reference.py, the independent Python restatement of the
read clustering, on the problems of tests/clustering_cases.py: labels and cluster count equal as arrays, score and posterior rows
equal by their bits (the reference ran with the project's exp / log), failure statuses where the reference panics with the other
chunks of the same call still clustered.

The reference's outputs come from tests/golden/clustering_reference.json (tests/golden/make_clustering_reference.py writes it,
tests/test_clustering_reference.py recomputes every case on the CPU and compares): the Python chain costs minutes, and this
module runs in one process.  Nothing here reads the reference checkout.

Shapes, from mcmc_chain_dispatch / chain_split_kernel (jtk_lc_cluster_features launches with the split buffer, so both chain
kernels run).  chain_split_kernel sends copy_num == 2 && n <= 127 && D <= 2 to mcmc_kernel_light, everything else to mcmc_kernel.
  CASES, n <= 63:  copy number 2 with 1 or 2 columns (mcmc_chain_k2<1, 1>, <2, 1>) and the early returns in the light kernel; in the
      full one copy number 2 with D = 3, 4, 6 (<3, 1>, <4, 1>, <8, 1>), D = 9 (mcmc_chain_tab<2>), copy numbers 3 and 4
      (mcmc_chain_tab<3> / <4>), all of them SMALL.  Cases of one haploid coverage go into one call (the coverage is a parameter of
      the call); the call of coverage 4 holds the panics of value next to chunks that succeed.
  LARGE_CASES, 64 <= n <= 256 (clustering_cases.device_path restates the dispatch, and tests/test_clustering_reference.py asserts
      the set of paths): the light kernel's <1, 2> (n = 64) and <2, 2> (n = 65, 127, 80 with weak columns, 81 with all-zero
      rows at 68 .. 80); the full kernel's <4, 2> (D = 3 at n = 64 and at the headline's 120 reads split 70 / 50, D = 4 at n = 88)
      and <8, 2> (D = 6 at n = 80, D = 8 at n = 127); mcmc_chain_tab<2> not SMALL by n = 128 and by D = 9 at n = 70, with its
      tables in registers at n = 255 and in LDS at n = 256 (big); mcmc_chain_tab<3> at n = 66 and <4> at n = 68.  Every case runs
      twice: in the call of its haploid coverage (five calls; in three of them both kernels run, and every work area is laid out
      for the call's largest n, D and copy number) and in a call of its own.
Not pinned to the reference, at any size: mcmc_kernel_huge (more than 1,023 reads, or a work area beyond 160 KiB: 41 M proposals
per tried k at 1,024 reads, more than half an hour of Python) and clustering_recursive's split for copy numbers of 8 and more.
Both stay pinned to the oracle (tests/test_gpu_parity.py, tests/test_gpu_shapes.py), which tests/test_clustering_reference.py pins
to the reference up to 256 reads.

Pile-ups (clustering_cases.PILEUPS: ont_diploid, hifi_diploid, a reduced ont_4copy, `planted`, whose reads carry one variant per
filter: inside MASK_LENGTH of either end, an Ins and a Del in a run of four, a single-strand one, a weak one, and
ont_diploid_80_reads, 40 reads per haplotype on 200 bp with three picked columns: the session path, which classifies chains by
their LDS need, above 63 reads):
jtk_lc_cluster_polished's labels, cluster count, score and posteriors, and the TOTAL / CAND rows of Session.trace
(column_filter_fused_kernel decides them), against the reference's.  That each planted column was dropped by its own filter is
asserted from the restatement in tests/test_clustering_reference.py; here the device must produce the reference's candidate set.

Duration of `pytest tests -m gpu` on one MI355X: GPU_SUITE_SECONDS below, `this` from the one full run made with these tests in
place.  The new tests take 0.1 to 1.6 s each, but for the two that hold tab4_68_reads (4.1 s: three tried k of 20 restarts each,
8.2 M proposals of which a quarter are taken, in mcmc_chain_tab<4>, which pays for every taken move).

Seeded fault, in an uncommitted copy of mcmc_kernels.hip (one run): KERNEL_SEEDED_FAULTS below.
"""
import json

import numpy as np
import pytest

import clustering_cases as K
from helpers import bits
from jtk_amd import api, batch as jb, ffi
from clustering_cases import GOLDEN, PILEUPS, pileup

pytestmark = pytest.mark.gpu
GPU_SUITE_SECONDS = dict(parent=(861.8, "183 passed, 1 skipped"), this=(899.1, "231 passed, 1 skipped"))
KERNEL_SEEDED_FAULTS = {
    "mcmc_chain_k2<D, 2> takes the picked read's flipped likelihood and signed row from table register 0 whatever its index":
        "test_large_feature_chunks_against_the_reference[20.0, 32.0, 40.0, 60.0], test_large_feature_chunk_on_its_own[every case with a "
        "read of index 64 or more whose k = 2 round runs the diploid chain: all but light_64_reads_1_column, k2_64_reads_3_columns, "
        "tab2_70_reads_9_columns, tab2_128_reads_3_columns, tab2_255_reads, tab2_256_reads], "
        "test_pileup_against_the_reference[ont_diploid_80_reads]: labels, score bits, or the chunk fails the chain's closing "
        "self-check; the 22 other tests of this module, every one of at most 63 reads among them, pass",
}


def _groups(cases=K.CASES):
    groups = {}
    for name, make in cases.items():
        c = make()
        groups.setdefault(repr(c["coverage"]), []).append((name, c))
    return groups


def _pack(cases):
    chunks = np.zeros(len(cases), dtype=ffi.FEATURE_CHUNK_DT)
    var, vts, voff, vtoff, first = [np.zeros(0)], [np.zeros(0, np.uint32)], 0, 0, 0
    for i, (_, c) in enumerate(cases):
        n, dim = c["x"].shape
        chunks[i] = (c["chunk_id"], c["copy_num"], n, dim, 0, voff, vtoff, first, c["local_coverage"])
        var.append(c["x"].ravel())
        vts.append(c["vt"].ravel().astype(np.uint32))
        voff, vtoff, first = voff + n * dim, vtoff + dim, first + n
    return chunks, np.concatenate(var + [np.zeros(1)]), np.concatenate(vts + [np.zeros(2, np.uint32)]), max(c["copy_num"] for _, c in cases)


@pytest.mark.parametrize("coverage", sorted(_groups()))
def test_feature_chunks_against_the_reference(jtk_lib, coverage):
    gold = json.load(open(GOLDEN))["cases"]
    cases = _groups()[coverage]
    chunks, var, vts, stride = _pack(cases)
    out = api.cluster_features(jb.default_params(cases[0][1]["coverage"]), chunks, var, vts, stride, raise_on_chunk_failure=False)
    want_fail = [gold[name]["status"] != 0 for name, _ in cases]
    if coverage == repr(4.0):   # the panics of value (zero band, NaN, all-zero weights) sit next to chunks that succeed
        assert sum(want_fail) == 4 and len(want_fail) - sum(want_fail) >= 10
    assert out["rc"] == (-6 if any(want_fail) else 0)
    _compare(cases, chunks, out, gold)


def _compare(cases, chunks, out, gold):
    for i, (name, c) in enumerate(cases):
        ref, res = gold[name], out["result"][i]
        if ref["status"] != 0:
            assert int(res["status"]) == -6, name
            continue
        n, k = c["x"].shape[0], ref["cluster_num"]
        rows = slice(int(chunks["read_first"][i]), int(chunks["read_first"][i]) + n)
        assert int(res["status"]) == 0 and int(res["cluster_num"]) == k, name
        assert out["label"][rows].tolist() == ref["label"], name
        assert "%016x" % int(bits([res["score"]])[0]) == ref["score"], name
        got = [["%016x" % int(b) for b in bits(row[:k])] for row in out["log_post"][rows]]
        assert got == ref["post"], name


@pytest.mark.parametrize("coverage", sorted(_groups(K.LARGE_CASES)))
def test_large_feature_chunks_against_the_reference(jtk_lib, coverage):
    """the cases of 64 reads and more, one call per haploid coverage: mcmc_kernel_light and mcmc_kernel run side by side, every
    chain in a work area laid out for the group's largest (lds_n, lds_d, lds_k)"""
    gold = json.load(open(GOLDEN))["large_cases"]
    cases = _groups(K.LARGE_CASES)[coverage]
    chunks, var, vts, stride = _pack(cases)
    out = api.cluster_features(jb.default_params(cases[0][1]["coverage"]), chunks, var, vts, stride)
    assert out["rc"] == 0
    _compare(cases, chunks, out, gold)


@pytest.mark.parametrize("name", list(K.LARGE_CASES))
def test_large_feature_chunk_on_its_own(jtk_lib, name):
    """each of them once more in a call of its own: a work area laid out for its own n, D and copy number gives the same bits"""
    gold = json.load(open(GOLDEN))["large_cases"]
    cases = [(name, K.LARGE_CASES[name]())]
    chunks, var, vts, stride = _pack(cases)
    out = api.cluster_features(jb.default_params(cases[0][1]["coverage"]), chunks, var, vts, stride)
    assert out["rc"] == 0
    _compare(cases, chunks, out, gold)


def test_large_groups_mix_the_kernels():
    """what the grouped calls are for, from the cases alone: every group but those of one path holds chains of both kernels or
    of different sizes, and every large case has a peer that differs from it in n or D in some call"""
    groups = {cov: [K.device_path(c) + c["x"].shape for _, c in cases] for cov, cases in _groups(K.LARGE_CASES).items()}
    assert len(groups) == 5 and all(len(set(g)) == len(g) >= 2 for g in groups.values())
    both = [cov for cov, g in groups.items() if {"mcmc_kernel_light", "mcmc_kernel"} <= {p[0] for p in g}]
    assert len(both) == 3


@pytest.mark.parametrize("config", list(PILEUPS))
def test_pileup_against_the_reference(jtk_lib, config):
    ref = json.load(open(GOLDEN))["pileups"][config]
    b, p = pileup(config)
    out = api.cluster_polished(p, b)
    n, k = int(b.chunks["n_reads"][0]), ref["cluster_num"]
    assert ref["status"] == 0 and int(out["result"]["status"][0]) == 0 and int(out["result"]["cluster_num"][0]) == k
    assert out["label"].tolist() == ref["label"]
    assert "%016x" % int(bits(out["result"]["score"])[0]) == ref["score"]
    assert [["%016x" % int(v) for v in bits(row[:k])] for row in out["log_post"][:n]] == ref["post"]
    with api.Session(p, b) as s:
        s.run(skip_polish=True)
        rows = s.trace(0)
    assert rows[0] == "TOTAL\t%d" % len(ref["cands"])
    assert [r.split("\t")[1:] for r in rows if r.startswith("CAND\t")] == ref["cands"]
