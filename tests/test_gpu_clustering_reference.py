"""jtk_lc_cluster_features (mcmc_kernels.hip) against tests/clustering_reference.py, the independent Python restatement of the
read clustering, on the problems of tests/clustering_cases.py: labels and cluster count equal as arrays, score and posterior rows
equal by their bits (the reference ran with the project's exp / log), failure statuses where the reference panics with the other
chunks of the same call still clustered.

The reference's outputs come from tests/golden/clustering_reference.json (tests/golden/make_clustering_reference.py writes it,
tests/test_clustering_reference.py recomputes every case on the CPU and compares): the Python chain costs minutes, and this
module runs in one process.  Nothing here reads the reference checkout.

Shapes, from mcmc_chain_dispatch / chain_split_kernel (jtk_lc_cluster_features launches with the split buffer, so both chain
kernels run): every case has n <= 63 reads.  chain_split_kernel sends copy_num == 2 && n <= 127 && D <= 2 to mcmc_kernel_light:
the cases of copy number 2 with 1 or 2 columns (mcmc_chain_k2<1, 1>, <2, 1>) and the early returns.  Everything else runs in
mcmc_kernel, the full one: copy number 2 with D = 3, 4, 6 (mcmc_chain_k2<3, 1>, <4, 1>, <8, 1>), D = 9 (mcmc_chain_tab<2>), copy
numbers 3 and 4 (mcmc_chain_tab<3> / <4>).  Cases of one haploid coverage go into one call (the coverage is a parameter of the
call); the call of coverage 4 holds the panics of value next to chunks that succeed.  No <D, 2> case (n in 64..127): the Python
chain needs 2000 n 20 proposals at about 13 us each, six minutes for n = 64 and one tried k.  That range, mcmc_kernel_huge, more
than 127 reads and the recursive split stay pinned to the oracle (tests/test_gpu_parity.py, tests/test_gpu_shapes.py), which
tests/test_clustering_reference.py pins to the reference at these small sizes: kernel == oracle at every size, oracle ==
reference at small sizes.

Pile-ups (clustering_cases.PILEUPS: ont_diploid, hifi_diploid, a reduced ont_4copy, and `planted`, whose reads carry one variant per
filter: inside MASK_LENGTH of either end, an Ins and a Del in a run of four, a single-strand one, a weak one):
jtk_lc_cluster_polished's labels, cluster count, score and posteriors, and the TOTAL / CAND rows of Session.trace
(column_filter_fused_kernel decides them), against the reference's.  That each planted column was dropped by its own filter is
asserted from the restatement in tests/test_clustering_reference.py; here the device must produce the reference's candidate set.

Duration of `pytest tests -m gpu` on one MI355X: GPU_SUITE_SECONDS below.  The parent commit's suite was measured; NOBODY HAS
MEASURED this commit's suite yet (`this` is None), nor run the pile-up tests of this module on a device: the feature tests ran
there (16 s, 13 s of it the library's first load) before the pile-up tests and the planted pile-up were added.
"""
import json

import numpy as np
import pytest

import clustering_cases as K
from helpers import bits
from jtk_amd import api, batch as jb, ffi
from clustering_cases import GOLDEN, PILEUPS, pileup

pytestmark = pytest.mark.gpu
GPU_SUITE_SECONDS = dict(parent=(861.8, "183 passed, 1 skipped"), this=None)


def _groups():
    groups = {}
    for name, make in K.CASES.items():
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
