"""dataset.correct_chunk_deletion / purge_largeindel / correct_deletion and `--stage correct_deletion` against
tests/deletion_reference.py on one small planted data set: 12 reads (3 of them reverse) over 5 chunks of 200 bases, simulated
with one error profile at a fixed seed; the middle node is taken out of 3 reads, one of those reads also carries a second,
shifted node of chunk 1, 4 reads lack 60 bases of chunk 3, and chunk 1 has a second cluster of 5 nodes, whose consensus is
polished.  The fixture is first checked on the CPU with the reference
alone -- the removed nodes come back, the duplicate goes, the indel nodes are purged -- and then the device stage's DataSet has
to be EQUAL to the reference's, field for field.  No tolerance: every float that decides something is compared on both sides
with the same operations in the same order (tests/test_gpu_purge.py pins the fit's bits), and the posteriors of a new node are
ln(1 / cluster_num) from the host's libm on both sides."""
import copy
import functools
import json
import os
import subprocess
import sys

import pytest

import deletion_reference as DR
import purge_reference as PR
from deletion_fixture import DELETED, DUPLICATE, MISSING, N_READS, REVERSE, SMALL_INDEL, fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def reference():
    """the filling rounds, purge_largeindel by (chunk, cluster) and by chunk -- each on the filled data set, at the small
    indel_size at which it fires on this fixture -- and the whole stage, by the reference (computed once, never changed)"""
    filled = copy.deepcopy(fixture())
    new_ids = DR.correct_chunk_deletion(filled)
    small, small_ids = [], []
    for compress in (False, True):
        ds = copy.deepcopy(filled)
        small_ids.append(DR.purge_largeindel(ds, SMALL_INDEL, 0.5, compress))
        small.append(ds)
    stage, stage_ids, _ = DR.correct_deletion(fixture())
    return dict(filled=filled, new_ids=new_ids, small=small, small_ids=small_ids, stage=stage, stage_ids=stage_ids)


def chunks_of(read):
    return [n["chunk"] for n in read["nodes"]]


def test_the_fixture_shows_all_three_effects_by_the_reference_alone():
    before, ref = fixture(), reference()
    for r in MISSING:
        assert 12 not in chunks_of(before["encoded_reads"][r])
    assert chunks_of(before["encoded_reads"][DUPLICATE]).count(11) == 2
    order = [10, 11, 12, 13, 14]
    for r, read in enumerate(ref["filled"]["encoded_reads"]):
        assert chunks_of(read) == (order if r not in REVERSE else order[::-1]), r       # the removed nodes are back, the duplicate is gone
    assert 12 in ref["new_ids"] and set(ref["new_ids"]) <= {11, 12}      # (the read with two nodes of chunk 11 may be offered a third)
    for read in ref["filled"]["encoded_reads"]:
        assert PR.nodes_to_encoded_read(read["id"], read["nodes"], before["raw_reads"][read["id"]]["seq"])["edges"] == read["edges"]
    assert ref["small_ids"] == [[13], [13]]
    for after in (ds["encoded_reads"] for ds in ref["small"]):
        for r in DELETED:
            assert 13 not in chunks_of(after[r]) and len(after[r]["nodes"]) == 4            # the indel nodes are purged
        assert sum(13 in chunks_of(read) for read in after) >= N_READS - len(DELETED) - 2   # (a node without any indel goes with them)
    for ds in ref["small"] + [ref["stage"]]:
        for read in ds["encoded_reads"]:                                                # EncodedRead::remove keeps a read whole
            assert recover(read) == before["raw_reads"][read["id"]]["seq"]
    assert ref["stage_ids"] == ref["new_ids"]                                           # nothing reaches MAX_ALLOWED_GAP here


def recover(read):
    """EncodedRead::recover_raw_read"""
    out = read["leading_gap"]
    for node, edge in zip(read["nodes"], read["edges"]):
        out += DR.original_seq(node)
        if edge["offset"] < 0:
            out = out[:len(out) + edge["offset"]]
        out += edge["label"]
    return out + DR.original_seq(read["nodes"][-1]) + read["trailing_gap"]


def same_dataset(got, want):
    assert [r["id"] for r in got["encoded_reads"]] == [r["id"] for r in want["encoded_reads"]]
    for a, b in zip(got["encoded_reads"], want["encoded_reads"]):
        for key in ("original_length", "leading_gap", "trailing_gap", "edges"):
            assert a[key] == b[key], (a["id"], key)
        assert len(a["nodes"]) == len(b["nodes"]), a["id"]
        for x, y in zip(a["nodes"], b["nodes"]):
            assert x == y, (a["id"], x["chunk"])
    assert got["selected_chunks"] == want["selected_chunks"] and got["coverage"] == want["coverage"]
    assert got == want


@pytest.mark.gpu
def test_correct_chunk_deletion_and_purge_largeindel_equal_the_reference():
    from jtk_amd import dataset as D
    ref = reference()
    ds = copy.deepcopy(fixture())
    assert D.correct_chunk_deletion(ds) == ref["new_ids"]
    same_dataset(ds, ref["filled"])
    for step, compress in enumerate((False, True)):
        purged = copy.deepcopy(ds)
        assert D.purge_largeindel(purged, SMALL_INDEL, 0.5, compress) == ref["small_ids"][step]
        same_dataset(purged, ref["small"][step])
    with pytest.raises(NotImplementedError, match="estimate_multiplicity"):
        D.correct_deletion(copy.deepcopy(fixture()), re_clustering=True)


@pytest.mark.gpu
def test_the_stage_round_trips_a_file(tmp_path):
    src, dst = tmp_path / "in.json", tmp_path / "out.json"
    src.write_text(json.dumps(fixture()))
    run = subprocess.run([sys.executable, "-m", "jtk_amd.dataset", "--stage", "correct_deletion", str(src), str(dst)], cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stderr
    ref = reference()
    assert "CD\tChanged\t%s\n" % ",".join(str(x) for x in ref["stage_ids"]) in run.stderr
    same_dataset(json.loads(dst.read_text()), ref["stage"])
