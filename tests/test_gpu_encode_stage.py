"""dataset.encode on the device -- map_reads, map_trials, encode_nodes, settle_nodes, nodes_to_encoded_read, then
correct_chunk_deletion -- on the planted set at 5 %: the five chunks as selected_chunks, the twelve reads (two of them lower-cased
in part) and one read from an unrelated genome as raw_reads.  It is EQUAL, field for field, to the Python composition of
tests/map_reference.py, encode_reference.py, settle_reference.py and deletion_reference.py's correct_chunk_deletion
(tests/map_stage_reference.py; its answer for this data set is recorded in tests/golden/encode_stage_planted.json, and
test_map_abi.py recomputes a read of it).  Independently of that composition, every read names its planted chunks in read order
on the planted strands, gives back its raw read, and the data set passes sanity_check."""
import copy
import json
import os
import subprocess
import sys

import pytest

import map_stage_reference as MS
from jtk_amd import dataset as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def staged(jtk_lib):
    ds, planted = MS.planted_data_set()
    before = copy.deepcopy(ds)
    gained = D.encode(ds, MS.SIM_THR, MS.SD_OF_ERROR)
    return ds, before, planted, gained


def test_encode_equals_the_python_composition(staged):
    ds, before, _, gained = staged
    want = MS.recorded()
    assert gained == want["gained"]
    assert [r["id"] for r in ds["encoded_reads"]] == [r["id"] for r in want["encoded_reads"]]
    for got, exp in zip(ds["encoded_reads"], want["encoded_reads"]):
        assert set(got) == set(exp), got["id"]
        for key in exp:
            assert got[key] == exp[key], (got["id"], key)
    rest = dict(ds, encoded_reads=[])
    assert rest == before                                                  # nothing but encoded_reads is written


def test_the_planted_chunks_in_read_order_on_the_planted_strands(staged):
    ds, _, planted, _ = staged
    by_id = {r["id"]: r for r in ds["encoded_reads"]}
    raw = {r["id"]: r["seq"] for r in ds["raw_reads"]}
    chunk_len = len(planted["chunks"][0])
    for r, spans in enumerate(planted["truth"]):
        read = by_id[100 + r]
        nodes = [(n["chunk"] - 10, n["is_forward"], n["position_from_start"], len(n["seq"])) for n in read["nodes"]]
        whole = sorted((lo, c, bool(fw), hi) for c, (lo, hi, fw) in spans.items())
        lo_g, hi_g = planted["origin"][r]
        # a chunk that leaves the read by at most ALLOWED_END_GAP bases may be encoded too; every other node is a planted one
        near = {c for c, s in enumerate(planted["starts"]) if c not in spans and lo_g - 30 <= s and s + chunk_len <= hi_g + 30}
        inside = [n for n in nodes if n[0] not in near]
        assert [(n[0], n[1]) for n in inside] == [(c, fw) for _, c, fw, _ in whole], read["id"]
        for (c, fw, pos, length), (lo, _, _, hi) in zip(inside, whole):
            assert abs(pos - lo) <= 10 and abs(pos + length - hi) <= 10, (read["id"], c)
        assert [n[2] for n in nodes] == sorted(n[2] for n in nodes)
        assert D.recover_raw_read(read) == raw[read["id"]].upper()
        assert D.is_uppercase(read)
    assert sum(len(s) for s in planted["truth"]) >= 10
    D.validate(ds)
    D.sanity_check(ds)


def test_a_read_from_an_unrelated_genome_is_not_encoded(staged):
    ds, _, _, _ = staged
    unrelated = ds["raw_reads"][-1]["id"]
    assert unrelated == 112 and unrelated not in {r["id"] for r in ds["encoded_reads"]} and len(ds["encoded_reads"]) == 12


def test_the_stage_on_the_command_line(tmp_path, jtk_lib):
    ds = MS.small_data_set()
    want = copy.deepcopy(ds)
    MS.encode(want, 0.2, 0.02, k=11, w=5)
    assert [r["id"] for r in want["encoded_reads"]] == [100, 101, 102, 104]
    src, dst = tmp_path / "in.json", tmp_path / "out.json"
    src.write_text(json.dumps(ds))
    run = subprocess.run([sys.executable, "-m", "jtk_amd.dataset", "--stage", "encode", "--sim-thr", "0.2", "--sd-of-error", "0.02", "--map-k", "11",
                          "--map-w", "5", str(src), str(dst)], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stderr
    assert json.loads(dst.read_text()) == want
    assert "ENCODE\tEncoded\t4\t5" in run.stderr
