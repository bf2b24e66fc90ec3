"""Sessions that share a lane (one stream, one merged chain launch: jtk_amd/csrc/session_lanes.h, launch_mcmc_merged) return,
bit for bit, what each returns when it runs alone.  JTK_LC_LANES forces the lane count per device (GPU_MAX_HW_QUEUES, which
decides it otherwise, cannot change once HIP has started).  The pile-ups are small (templates of 300 bp, 12 - 24 reads): what
is under test is whose pointers a chain workgroup of a merged launch runs on, which does not depend on the size.  The chunk
kinds cover both chain kernels and the early return: diploid pile-ups with variants (light kernel), one pile-up of copy number
3 (general kernel), one without a variant column (trivial)."""
import os
import threading

import numpy as np
import pytest

import helpers
from jtk_amd import api, batch as jb, synth

pytestmark = [pytest.mark.gpu, pytest.mark.changes_env]

FIELDS = ("label", "log_post", "cons_off", "ops_out_off")


@pytest.fixture(scope="module")
def lib(jtk_lib):
    assert jtk_lib.jtk_lc_device_ok(0) == 1, "needs a gfx950 device"
    return jtk_lib


def diploid(chunk_id, rph):
    return synth.make_pileup(chunk_id, dict(synth.CONFIGS["ont_diploid"], tmpl_len=300, reads_per_hap=rph), min_variants=1)


def three_copies(chunk_id):
    cfg = dict(synth.CONFIGS["ont_4copy"], tmpl_len=300, n_haps=3, copy_num=3, reads_per_hap=8, divergence=4e-2)
    return synth.make_pileup(chunk_id, cfg, min_variants=3)


def no_variant(chunk_id):
    # two identical haplotypes, HiFi error rates: no column passes the variant filter
    return synth.make_pileup(chunk_id, dict(synth.CONFIGS["hifi_diploid"], tmpl_len=300, reads_per_hap=6, divergence=0.0))


def pileups():
    """the nine pile-ups: [0] session 1, [1:3] session 2, [3:8] session 3, [8] one more for the one-shot call"""
    return [diploid(700, 7), diploid(701, 8), diploid(702, 12), diploid(703, 6), diploid(704, 10), three_copies(705),
            no_variant(706), diploid(707, 12), diploid(708, 9)]


PARAMS = jb.default_params(haploid_coverage=8.0, band_frac=synth.CONFIGS["ont_diploid"]["band_frac"])


def snapshot(out):
    n, m = int(out["cons_off"][-1]), int(out["ops_out_off"][-1])
    d = {k: out[k].copy() for k in FIELDS}
    d.update(result=out["result"].copy(), cons=out["cons"][:n].copy(), ops_out=out["ops_out"][:m].copy())
    return d


def assert_same(got, want, what):
    for k in FIELDS + ("cons", "ops_out"):
        assert np.array_equal(got[k], want[k]), (what, k)
    assert np.array_equal(helpers.bits(got["log_post"]), helpers.bits(want["log_post"])), (what, "log_post bits")
    assert got["result"].tobytes() == want["result"].tobytes(), (what, "result records")


def two_passes(session):
    outs = []
    for _ in range(2):
        session.run()
        outs.append(snapshot(session.fetch()))
    return outs


@pytest.fixture(scope="module")
def alone(lib):
    """every batch the tests use, run as a session of its own with JTK_LC_LANES unset: two passes each (computed once)"""
    assert "JTK_LC_LANES" not in os.environ
    ps = pileups()
    batches = dict(s1=jb.pack(ps[0:1]), s2=jb.pack(ps[1:3]), s3=jb.pack(ps[3:8]), all9=jb.pack(ps))
    batches.update({"one%d" % i: jb.pack([ps[i]]) for i in range(9)})
    ref = {}
    for name, b in batches.items():
        with api.Session(PARAMS, b) as s:
            first, second = two_passes(s)
        assert_same(second, first, (name, "second pass alone"))
        ref[name] = first
    r3 = ref["s3"]["result"]
    assert int(r3["n_variants"][3]) == 0 and int(r3["cluster_num"][3]) == 1, "the pile-up without a variant column has one"
    assert (np.delete(r3["n_variants"], 3) > 0).all() and (r3["status"] == 0).all()
    return batches, ref


def run_concurrently(batches, names):
    """one session per name, created here, then two passes each from a thread of its own (started together)"""
    sessions = [api.Session(PARAMS, batches[n]) for n in names]
    outs, errors = [None] * len(names), []
    gate = threading.Barrier(len(names))

    def work(i):
        try:
            gate.wait()
            outs[i] = two_passes(sessions[i])
        except BaseException as e:  # noqa: BLE001 -- handed to the main thread
            gate.abort()
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(names))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for s in sessions:
        s.close()
    if errors:
        raise errors[0]
    return outs


@pytest.mark.parametrize("lanes", ["1", "2"])
def test_three_sessions_sharing_lanes_equal_each_alone(lib, alone, monkeypatch, lanes):
    batches, ref = alone
    monkeypatch.setenv("JTK_LC_LANES", lanes)
    names = ["s1", "s2", "s3"]
    for name, (first, second) in zip(names, run_concurrently(batches, names)):
        assert_same(first, ref[name], (name, "lanes " + lanes, "first pass"))
        assert_same(second, first, (name, "lanes " + lanes, "second pass"))


def test_one_shot_call_on_shared_lanes(lib, alone, monkeypatch):
    batches, ref = alone
    b = batches["all9"]
    monkeypatch.setenv("JTK_LC_SLICES", "3")
    outs = {}
    for lanes in ("1", "3"):
        monkeypatch.setenv("JTK_LC_LANES", lanes)
        outs[lanes] = snapshot(api.cluster_chunks(PARAMS, b))
    assert_same(outs["3"], outs["1"], "one-shot, lanes 3 against 1")
    assert_same(outs["1"], ref["all9"], "one-shot on one lane against the resident session alone")


def test_nine_sessions_on_one_lane_cross_the_segment_bound(lib, alone, monkeypatch):
    batches, ref = alone
    monkeypatch.setenv("JTK_LC_LANES", "1")
    names = ["one%d" % i for i in range(9)]
    for name, (first, second) in zip(names, run_concurrently(batches, names)):
        assert_same(first, ref[name], (name, "first pass"))
        assert_same(second, first, (name, "second pass"))
