"""bench.py --dump-outputs on the host: the arrays a step hands its caller, written as float .npy files within 64 MiB, with the
consensus / re-threaded ops of slices stitched back into chunk / read order and sampled by a choice that depends on the inputs
only (the GPU run of the option is in tests/test_bench_gpu.py)."""
import os

import numpy as np

import helpers
from jtk_amd import api


def _fake_outputs(batch, first_chunk, first_read, n_chunks, n_reads):
    """what Session.fetch returns for a slice, filled with values that name their chunk / read"""
    sub = batch.subset(range(first_chunk, first_chunk + n_chunks))
    o = api._outputs(sub)
    o["label"][:] = np.arange(first_read, first_read + n_reads) % 3
    o["log_post"][:] = -np.arange(first_read, first_read + n_reads)[:, None] / 7.0
    o["result"]["score"] = np.arange(first_chunk, first_chunk + n_chunks) * 0.5
    o["result"]["cluster_num"] = 2
    pos = 0
    for c in range(n_chunks):
        n = 10 + (first_chunk + c)
        o["cons"][pos:pos + n] = first_chunk + c
        o["cons_off"][c + 1] = pos = pos + n
    pos = 0
    for r in range(n_reads):
        n = 5 + (first_read + r) % 4
        o["ops_out"][pos:pos + n] = (first_read + r) % 251
        o["ops_out_off"][r + 1] = pos = pos + n
    return o


def test_dump_outputs_writes_the_step_outputs_in_order(jtk_lib, tmp_path):
    import bench
    b, _, _ = helpers.small_batch(n_chunks=4, tmpl_len=200, reads_per_hap=3)
    rpc = b.n_reads // b.n_chunks
    pieces = [(_fake_outputs(b, 0, 0, 1, rpc), 0, 0), (_fake_outputs(b, 1, rpc, 3, 3 * rpc), 1, rpc)]
    merged = dict(label=np.concatenate([p[0]["label"] for p in pieces]), log_post=np.concatenate([p[0]["log_post"] for p in pieces]),
                  result=np.concatenate([p[0]["result"] for p in pieces]))
    total = bench.dump_outputs(str(tmp_path), b, merged, pieces)
    files = sorted(os.listdir(tmp_path))
    assert all(f.endswith(".npy") for f in files)
    got = {f[:-4]: np.load(tmp_path / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert total == sum(a.nbytes for a in got.values()) <= 64 << 20
    assert np.array_equal(got["label"], np.arange(b.n_reads) % 3)
    assert np.array_equal(got["log_post"], merged["log_post"])
    assert np.array_equal(got["result_score"], np.arange(4) * 0.5) and np.all(got["result_cluster_num"] == 2)
    # small outputs are kept whole: every chunk's consensus and every read's ops, in chunk / read order
    assert np.array_equal(got["cons_len"], 10 + np.arange(4)) and np.array_equal(got["cons_sample_chunks"], np.arange(4))
    assert np.array_equal(got["cons_sample"], np.repeat(np.arange(4), 10 + np.arange(4)))
    assert np.array_equal(got["ops_len"], 5 + np.arange(b.n_reads) % 4)
    assert np.array_equal(got["ops_sample"], np.repeat(np.arange(b.n_reads) % 251, 5 + np.arange(b.n_reads) % 4))


def test_ragged_sample_is_fixed_and_bounded():
    import bench
    est = np.full(1000, 100.0)
    a = bench.ragged_sample(1000, est, cap=10_000)
    assert np.array_equal(a, bench.ragged_sample(1000, est, cap=10_000))   # the same choice every run
    assert len(a) == 100 and np.all(np.diff(a) > 0) and a.max() < 1000
    assert np.array_equal(bench.ragged_sample(10, np.full(10, 5.0), cap=50), np.arange(10))
