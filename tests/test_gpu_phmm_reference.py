"""The pair-HMM kernels against tests/phmm_reference.py directly, without the oracle in the loop: phmm_kernel + finalize
(jtk_lc_modification_table, radius <= 30), phmm_wide_kernel (radius 31-255, at the edges of its LDS frames and at full band),
phmm_pair_kernel (radius <= 14, reached through a session: its CAND rows) and the refit (jtk_lc_fit_model, one round).
The inputs are those of tests/test_phmm_reference.py: reads with 10-15 % errors and indel runs, mixed strands, forward and
reverse models that differ."""
import math
import os

import numpy as np
import pytest

import phmm_reference as R
import test_phmm_reference as T
import test_trace_rows as TR
from jtk_amd import api, batch as jb, ffi, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(jtk_lib):
    assert os.environ.get("JTK_DEVICE_IS_ORACLE") or jtk_lib.jtk_lc_device_ok(0) == 1, "needs a gfx950 device"
    return jtk_lib


def device_params(fwd, rev, tmpl_len, radius):
    """the stage's params with both strands' models and a band_frac that gives `radius` at tmpl_len (mod.rs:96,112)"""
    p = jb.default_params(haploid_coverage=10.0)
    fwd.fill(p.forward)
    rev.fill(p.reverse)
    p.band_frac = (2 * radius + 0.5) / tmpl_len
    assert int(np.ceil(tmpl_len * p.band_frac)) // 2 == radius
    return p


def check_pileup(tmpl, reads, opss, strands, radius, model="asym"):
    fwd, rev = T.models()[model]
    p = device_params(fwd, rev, len(tmpl), radius)
    tab, lk = api.modification_table(p, tmpl, reads, opss, strands)
    for r in range(len(reads)):
        ref_tab, ref_lk = R.modification_table(fwd if strands[r] else rev, tmpl, reads[r], opss[r], radius)
        T.assert_table_matches(ref_tab, ref_lk, tab[r].reshape(len(tmpl) + 1, R.NUM_ROW), lk[r], where=(radius, r))
    return tab, lk


def noisy_pileup(seed, L, n_reads=6):
    rng = np.random.default_rng(seed)
    tmpl = T.random_tmpl(rng, L)
    reads, opss = [], []
    for r in range(n_reads):
        rd, op = T.noisy_read(rng, tmpl, 0.10 + 0.01 * r, run_rate=0.02,
                              lead=[(R.OP_INS, 3)] if r == 2 else [], tail=[(R.OP_DEL, 3)] if r == 3 else [])
        reads.append(rd)
        opss.append(op)
    return tmpl, reads, opss, [1, 0, 1, 0, 0, 1][:n_reads]


@pytest.mark.parametrize("radius", [2, 3, 8, 29, 30])
def test_phmm_kernel_table_matches_the_reference(lib, radius):
    """phmm_kernel + finalize: lk, table - lk and the sentinel mask of every read, under its own strand's model"""
    L = 150 + 7 * radius if radius < 10 else 420
    check_pileup(*noisy_pileup(200 + radius, L), radius, model="asym")
    if radius == 3:
        check_pileup(*noisy_pileup(300, L), radius, model="zero")


@pytest.mark.parametrize("radius", [2, 8])
def test_phmm_kernel_at_block_boundaries(lib, radius):
    """T = L + n in {63, 64, 65, 127, 128, 129} (and {7, 8, 9} on a 4-base template): the 8-diagonal groups and the 64-diagonal
    scaling blocks end at the last diagonal"""
    rng = np.random.default_rng(40 + radius)
    shapes = [(60, [3, 4, 5, 67, 68, 69])] + ([(4, [3, 4, 5])] if radius == 2 else [])
    for L, ns in shapes:
        tmpl = T.random_tmpl(rng, L)
        reads, opss = zip(*[T.shaped_read(rng, tmpl, n, 0.15) for n in ns])
        check_pileup(tmpl, list(reads), list(opss), [k % 2 for k in range(len(ns))], radius)


@pytest.mark.parametrize("radius,L", [(31, 300), (127, 400), (128, 400), (255, 560)])
def test_phmm_wide_kernel_table_matches_the_reference(lib, radius, L):
    """phmm_wide_kernel at the edges of its LDS frames (256 band cells per ring row up to radius 127, 512 beyond)"""
    check_pileup(*noisy_pileup(500 + radius, L, n_reads=4), radius)


def test_phmm_wide_kernel_at_full_band_is_the_likelihood_of_the_edited_template(lib):
    """radius 255 >= L + n: every device table entry is the reference's unbanded likelihood of the explicitly edited template"""
    rng = np.random.default_rng(77)
    tmpl = T.homopolymer_tmpl(rng, 40)
    reads, opss = [], []
    for r in range(2):
        rd, op = T.noisy_read(rng, tmpl, 0.15, run_rate=0.05)
        reads.append(rd)
        opss.append(op)
    strands = [1, 0]
    tab, lk = check_pileup(tmpl, reads, opss, strands, 255)
    fwd, rev = T.models()["asym"]
    for r in range(2):
        m = fwd if strands[r] else rev
        t = tab[r].reshape(len(tmpl) + 1, R.NUM_ROW) + lk[r]
        for pos in range(len(tmpl) + 1):
            for row in range(R.NUM_ROW):
                t2 = R.edited(tmpl, pos, row)
                if t2 is None:
                    assert t[pos, row] <= -1e299
                else:
                    assert abs(t[pos, row] - R.likelihood_unbanded(m, t2, reads[r])) < 1e-8, (r, pos, row)


def test_phmm_pair_kernel_cand_rows_match_the_reference(lib):
    """HiFi pile-ups (radius 10: phmm_pair_kernel) through a session: the device's CAND rows are the numpy restatement of
    tests/test_trace_rows.py applied to the reference's tables of the session's own consensus and ops"""
    b, cfg = synth.make_batch("hifi_diploid", 2)
    p = jb.default_params(cfg["coverage"], cfg["band_frac"])
    p.reverse.mat_mat, p.reverse.mat_del = 0.96, 0.02          # the two strands' models differ
    fwd, rev = R.Model.of(p.forward), R.Model.of(p.reverse)
    seen = 0
    with api.Session(p, b) as s:
        s.run()
        out = s.fetch()
        for c in range(2):
            rows = s.trace(c)
            cands = [r.split("\t") for r in rows if r.startswith("CAND\t")]
            cons = out["cons"][int(out["cons_off"][c]):int(out["cons_off"][c + 1])]
            radius = int(math.ceil(len(cons) * p.band_frac)) // 2
            assert radius <= 14
            prof = []
            for g in b.chunk_reads(c):
                ops = out["ops_out"][int(out["ops_out_off"][g]):int(out["ops_out_off"][g + 1])]
                tab, lk = R.modification_table(fwd if b.strand[g] else rev, cons, b.read(g), ops, radius)
                prof.append(np.where(tab > -1e299, tab - lk, tab).ravel())
            prof = np.array(prof)
            homop = TR.homopolymer_lengths(cons)
            ks = range(1, int(b.chunks["copy_num"][c]) + 1)
            for cd in cands:
                lk, count = TR.cand_lk_count(prof, int(cd[1]), int(cd[2]), homop, p, ks)
                assert count == int(cd[4]) and "%.1f" % lk == cd[3], (c, cd, lk, count)
                seen += 1
    assert seen >= 2


def test_fit_model_one_round_matches_the_reference(lib):
    """jtk_lc_fit_model, rounds = 1, on pile-ups that are fixed points of the fit's polish: the refitted forward and reverse
    models are the reference's E-step (counts pooled per strand) + M-step"""
    b, po, radius = T.fit_pileups()
    p = jb.default_params(haploid_coverage=po.haploid_coverage, band_frac=po.band_frac)
    p.forward = ffi.Hmm.from_buffer_copy(bytes(po.forward))
    p.reverse = ffi.Hmm.from_buffer_copy(bytes(po.reverse))
    nf, nr, _ = T.reference_fit(b, po, radius)
    df, dr = api.fit_model(p, b, rounds=1)
    assert np.allclose(R.Model.of(df).flat(), nf.flat(), rtol=1e-9, atol=0)
    assert np.allclose(R.Model.of(dr).flat(), nr.flat(), rtol=1e-9, atol=0)
