"""The polishing kernels (select_edits_kernel, rethread_kernel, commit_kernel and the column totals that feed them) against the
polishing of tests/phmm_reference.py, without the oracle in the loop.  The pile-ups are those of tests/test_polish_reference.py,
whose census assertions (run there, on the CPU) show which path each one takes.

  jtk_lc_polish_chunks   finalize_kernel + the unfused totals; one call per radius class: 8 (phmm_pair_kernel), 20 (phmm_kernel),
                         40 (phmm_wide_kernel), and one per take_num / ignore_edge variant
  jtk_lc_cluster_chunks  sum_final_kernel from row sums, polish at (band_width / 2, take_num = n, ignore_edge = 3): the fetched
                         consensus, ops_out and polish_rounds only

Compared are outcomes: consensus bytes, every read's ops, the number of rounds."""
import math
import os

import numpy as np
import pytest

import phmm_reference as R
import test_phmm_reference as T
import test_polish_reference as P
from test_gpu_phmm_reference import device_params
from jtk_amd import api, batch as jb

pytestmark = pytest.mark.gpu

SUBSET = sorted(n for n, c in P.CASES.items() if c["cluster"] and n != "long_many_edits")


@pytest.fixture(scope="module")
def lib(jtk_lib):
    assert os.environ.get("JTK_DEVICE_IS_ORACLE") or jtk_lib.jtk_lc_device_ok(0) == 1, "needs a gfx950 device"
    return jtk_lib


def polish_call(names, radius, take_num, ignore_edge, **kw):
    fwd, rev = T.models()["asym"]
    b = P.batch_of(names)
    out = api.polish_chunks(device_params(fwd, rev, 100, 8), b, radius=radius, take_num=take_num, ignore_edge=ignore_edge, **kw)
    return b, out


@pytest.mark.parametrize("radius,names", [(8, P.MAIN), (20, SUBSET), (40, SUBSET)])
def test_polish_chunks_matches_the_reference(lib, radius, names):
    """every case in one batch per radius class: template ends, multi-base rows, the skip schedule, ops under an edit, edits at
    the 64-op step edges of rethread_kernel, reads of more than 1,023 ops, chunks that stop after 1, 2, 3 and 6+ rounds"""
    assert all(P.CASES[n]["take_num"] == 0 and P.CASES[n]["ignore_edge"] == 0 for n in names)
    b, out = polish_call(names, radius, 0, 0)
    assert out["rc"] == 0 and (out["result"]["status"] == 0).all()
    for c, name in enumerate(names):
        P.assert_same_outcome(P.reference(name, radius=radius), *P.outputs_of(b, out, c), where=(name, radius))


@pytest.mark.parametrize("name,take_num,ignore_edge,radius", [v + (r,) for v, r in zip(P.VARIANTS, [8, 20, 40, 20, 8])])
def test_take_num_and_ignore_edge(lib, name, take_num, ignore_edge, radius):
    """take_num limits the voters and not the reads that are re-threaded; ignore_edge limits the scan (2 * ignore_edge >= L: one
    round, the input returned)"""
    b, out = polish_call([name, "clean_draft"], radius, take_num, ignore_edge)
    assert out["rc"] == 0
    for c, nm in enumerate([name, "clean_draft"]):
        res = P.reference(nm, radius=radius, take_num=take_num, ignore_edge=ignore_edge)
        P.assert_same_outcome(res, *P.outputs_of(b, out, c), where=(nm, take_num, ignore_edge, radius))


def test_cluster_chunks_polishing_matches_the_reference(lib):
    """the clustering session's polish (column totals by sum_final_kernel): every case marked for it in one batch; band_frac 0.2
    gives radii 6-15 on the short chunks (phmm_pair_kernel, phmm_kernel) and 109 on the long one (phmm_wide_kernel)"""
    names = sorted(n for n, c in P.CASES.items() if c["cluster"])
    fwd, rev = T.models()["asym"]
    b = P.batch_of(names)
    p = jb.default_params(haploid_coverage=8.0, band_frac=0.2)
    fwd.fill(p.forward)
    rev.fill(p.reverse)
    out = api.cluster_chunks(p, b)
    assert out["rc"] == 0 and (out["result"]["status"] == 0).all()
    radii = set()
    for c, name in enumerate(names):
        radius = int(math.ceil(len(P.pile_of(name)["tmpl"]) * p.band_frac)) // 2
        radii.add(radius)
        res = P.reference(name, radius=radius, take_num=0, ignore_edge=3)
        P.assert_same_outcome(res, *P.outputs_of(b, out, c), where=(name, radius, "cluster"))
    assert min(radii) <= 14 and any(15 <= r <= 30 for r in radii) and max(radii) > 30, radii


def test_a_draft_too_short_for_its_capacity_fails_its_chunk_only(lib):
    """a consensus may grow to L + L / 8 + 64 bases.  The 40-base draft here lacks two of every three bases of its truth: the
    reference's polish passes 109 bases, so the device must fail THAT chunk with JTK_ERR_CHUNK_FAILED (a status, not a fault)
    and its neighbours in the batch must still match the reference.
    edit_cap = cap / 2 + 2 is not tested: edits of one round are at least 1 + inactive >= 6 positions apart, so a round selects
    at most ceil(L / 6) <= cap / 2 of them and the cap cannot bind."""
    rng = np.random.default_rng(900)
    draft = P.plain_tmpl(rng, 40)
    segs = []
    for k in range(40):
        extra = [P.other_base(rng, draft[k]), P.other_base(rng, draft[k])]
        segs.append(P.Seg(draft[k:k + 1], [draft[k]] + extra))
    pile = P.build(rng, segs, 6, err=0.0)
    fwd, rev = T.models()["asym"]
    cons, _, rounds, _ = R.polish(fwd, rev, pile["tmpl"], pile["reads"], pile["opss"], pile["strands"], 8, 6, 0)
    cap = 40 + 40 // 8 + 64
    assert len(cons) > cap, (len(cons), rounds)
    piles = [(950, 1, pile["tmpl"], pile["reads"], pile["opss"], pile["strands"], None)]
    names = ["skip_span1_-1", "clean_draft"]
    for k, name in enumerate(names):
        q = P.pile_of(name)
        piles.insert(2 * k, (951 + k, 1, q["tmpl"], q["reads"], q["opss"], q["strands"], None))
    b = jb.pack(piles)                                     # skip case, the short draft, the clean draft
    out = api.polish_chunks(device_params(fwd, rev, 100, 8), b, radius=8, take_num=0, ignore_edge=0, raise_on_chunk_failure=False)
    assert out["rc"] == -6 and out["result"]["status"].tolist() == [0, -6, 0]                  # JTK_ERR_CHUNK_FAILED
    for c, name in [(0, names[0]), (2, names[1])]:
        P.assert_same_outcome(P.reference(name, radius=8), *P.outputs_of(b, out, c), where=(name, "beside a failed chunk"))
