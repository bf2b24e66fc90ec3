"""`ds.encode` with the mapper in minimap2's place, restated in plain Python on a JTK `DataSet` as parsed from JSON, composed from
the references of the primitives -- nothing of the library is used:

    tests/map_reference.py        the placements and the trial windows (own spec)
    tests/encode_reference.py     encode_node (guided passes: DESIGN section 4, not kiley)
    tests/settle_reference.py     the sorts and remove_slippy_alignment of encode_read_to_nodes_by_paf
    tests/purge_reference.py      nodes_to_encoded_read
    tests/deletion_reference.py   correct_chunk_deletion

Also the stand-ins of api.map_reads, api.encode_nodes and api.settle_nodes by these references, for tests of the driver that
run without a device, and the planted data set of the stage's tests."""
import json
import math
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))     # (run as a script: the package is one level up)

import deletion_reference as DR
import encode_reference as E
import map_cases as K
import map_reference as M
import purge_reference as PR
import settle_reference as S
from jtk_amd import dataset as D, ffi


def encode_by_map(ds, sim_thr, **map_params):
    chunks, reads = ds["selected_chunks"], ds["raw_reads"]
    chunk_seqs = [c["seq"].upper().encode("ascii") for c in chunks]
    read_seqs = [r["seq"].encode("ascii") for r in reads]
    placed = M.map_reads(chunk_seqs, read_seqs, **map_params)
    found = {}
    for i, start, end, forward, thr in M.map_trials(placed, [len(s) for s in read_seqs], [len(s) for s in chunk_seqs], sim_thr):
        r, c = placed[i]["query"], placed[i]["target"]
        res = E.encode_node(read_seqs[r], start, end, bool(forward), chunk_seqs[c], chunk_seqs[c], thr)
        if res["verdict"] != E.ACCEPTED:
            continue
        k = chunks[c]["cluster_num"]
        node = {"position_from_start": res["position_from_start"], "chunk": chunks[c]["id"], "cluster": 0, "seq": res["query"].decode("ascii"),
                "is_forward": bool(forward), "cigar": DR.cigar_of(res["ops"]), "posterior": [math.log(1.0 / max(k, 1))] * k}
        found.setdefault(r, []).append((node, res["score"], len(chunk_seqs[c])))
    ds["encoded_reads"] = []
    for r in sorted(found):
        nodes = []                                             # (node, score): the better of two that overlap by more than half the chunk
        for node, score, chunk_len in found[r]:
            span = (node["position_from_start"], node["position_from_start"] + len(node["seq"]))
            rival = [j for j, (o, _) in enumerate(nodes) if o["chunk"] == node["chunk"] and
                     2 * (min(span[1], o["position_from_start"] + len(o["seq"])) - max(span[0], o["position_from_start"])) > chunk_len]
            if not rival:
                nodes.append((node, score))
            elif nodes[rival[0]][1] < score:
                nodes[rival[0]] = (node, score)
        nodes = [n for n, _ in nodes]
        kept = S.settle_read([DR.settle_node(n) for n in nodes], S.BY_CHUNK)
        read = PR.nodes_to_encoded_read(reads[r]["id"], [nodes[i] for i in kept], reads[r]["seq"])
        ds["encoded_reads"].append({key: read[key] for key in ("id", "original_length", "leading_gap", "trailing_gap", "edges", "nodes")})


def encode(ds, sim_thr, sd_of_error, **map_params):
    encode_by_map(ds, sim_thr, **map_params)
    return DR.correct_chunk_deletion(ds, sim_thr=sim_thr, stddev_of_error=sd_of_error)


# ---- stand-ins of the three device calls of dataset.encode_by_map

def map_reads(targets, queries, device=0, **params):
    found = M.map_reads(list(targets), list(queries), **params)
    return np.array([tuple(p[f] for f in ffi.MAP_PLACEMENT_DT.names) for p in found], dtype=ffi.MAP_PLACEMENT_DT)


def encode_nodes(trials, read_bases, cons_bases, chunk_bases, device=0, raise_on_trial_failure=True):
    result, ops, ops_off = np.zeros(len(trials), dtype=ffi.ENCODE_RESULT_DT), [], [0]
    for t, tr in enumerate(trials):
        res = E.encode_node(bytes(read_bases[int(tr["read_off"]):]), int(tr["start"]), int(tr["end"]), bool(tr["is_forward"]),
                            bytes(cons_bases[int(tr["cons_off"]):int(tr["cons_off"]) + int(tr["cons_len"])]),
                            bytes(chunk_bases[int(tr["chunk_off"]):int(tr["chunk_off"]) + int(tr["chunk_len"])]), float(tr["sim_thr"]))
        for key in ("status", "verdict", "trim_head", "trim_tail", "position_from_start", "score"):
            result[t][key] = res[key]
        ops += list(res["ops"])
        ops_off.append(len(ops))
    return dict(result=result, ops=np.array(ops, dtype=np.uint8), ops_off=np.array(ops_off, dtype=np.uint64), rc=0)


def settle_nodes(node_off, nodes, ops, ops_off, mode=1, device=0):
    reads = []
    for r in range(len(node_off) - 1):
        reads.append([dict(chunk=int(n["chunk"]), pos=int(n["position_from_start"]), fwd=bool(n["is_forward"]), qlen=int(n["query_len"]),
                           cigar=DR.runs(D.ops_to_cigar(ops[int(ops_off[e]):int(ops_off[e + 1])])))
                      for e, n in enumerate(nodes) if int(node_off[r]) <= e < int(node_off[r + 1])])
    out = S.settle(reads, mode)
    return dict(order=[np.array(o) for o in out["order"]], rc=out["rc"])


# ---- data

def data_set(chunks, reads, read_type="ONT"):
    hmm = {n: 0.0 for n in ("mat_mat", "mat_ins", "mat_del", "ins_mat", "ins_ins", "ins_del", "del_mat", "del_ins", "del_del")}
    hmm.update(mat_emit=[0.0] * 16, ins_emit=[0.0] * 20)
    return {"input_file": "reads.fa", "masked_kmers": {"k": 12, "thr": 0}, "coverage": "NotAvailable",
            "raw_reads": [{"name": "r%d" % i, "desc": "", "id": 100 + i, "seq": r.decode("ascii")} for i, r in enumerate(reads)], "hic_pairs": [],
            "selected_chunks": [{"id": 10 + i, "seq": c.decode("ascii"), "cluster_num": 1, "copy_num": 1, "score": 0.0} for i, c in enumerate(chunks)],
            "encoded_reads": [], "hic_edges": [], "read_type": read_type, "model_param": {"forward": hmm, "reverse": dict(hmm)},
            "error_rate": {n: 0.0 for n in ("del", "del_sd", "ins", "ins_sd", "mismatch", "mism_sd", "total", "total_sd")}, "processed_stages": []}


def planted_data_set():
    """the planted set at 5 %: the five chunks, the twelve reads -- two of them lower-cased in part, as a masked read is -- and one
    more read from an unrelated genome.  -> (the data set, the planted set)"""
    p = K.planted_at(0.05)
    reads = list(p["reads"]) + [p["unrelated"]]
    reads[2] = reads[2][:700] + reads[2][700:3100].lower() + reads[2][3100:]
    reads[7] = reads[7][:40].lower() + reads[7][40:]
    return data_set(p["chunks"], reads), p


def small_data_set():
    """three chunks of 150 bases and five reads: forward, reverse, one that holds chunk 1 twice, one unrelated, one lower case"""
    rng = random.Random(77)
    genome = K.rand_seq(rng, 900)
    chunks = [genome[100:250], genome[350:500], genome[600:750]]
    noisy = lambda s: K.mutate(s, 0.04, rng)[0]   # noqa: E731
    reads = [noisy(genome[40:800]), K.rc(noisy(genome[60:560])), noisy(genome[300:520]) + K.rand_seq(rng, 30) + noisy(genome[340:520]),
             K.rand_seq(rng, 700), noisy(genome[80:780]).lower()]
    return data_set(chunks, reads)


# The guided passes of encode_node take this plain Python about a minute on the planted set (23 windows of 2,400 bases against
# 2,000, three banded passes each), so its answer is recorded: tests/golden/encode_stage_planted.json holds `encode` of
# planted_data_set() with these arguments, written by `python tests/map_stage_reference.py`.  test_map_abi.py recomputes one
# read of it on every run.
SIM_THR, SD_OF_ERROR = 0.15, 0.02
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encode_stage_planted.json")


def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":
    ds, _ = planted_data_set()
    gained = encode(ds, SIM_THR, SD_OF_ERROR)
    with open(GOLDEN, "w") as f:
        json.dump({"sim_thr": SIM_THR, "sd_of_error": SD_OF_ERROR, "gained": gained, "encoded_reads": ds["encoded_reads"]}, f, indent=0)
        f.write("\n")
