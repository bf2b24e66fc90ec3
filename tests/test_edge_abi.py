"""jtk_lc_encode_edges through every layer that needs no GPU: the header declares it and its structs, the ctypes binding agrees on
their sizes and field order, the library exports it, the build list, the Rust source and the documents carry it, and every
invalid argument is refused before a device is looked for."""
import os
import re

import numpy as np
import pytest

from jtk_amd import api, ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, DEBUG = "jtk_lc_encode_edges", "jtk_lc_debug_edges_timing"
STRUCTS = (("jtk_edge_trial", "EDGE_TRIAL_DT", 56, "JtkEdgeTrial"), ("jtk_edge_result", "EDGE_RESULT_DT", 32, "JtkEdgeResult"),
           ("jtk_edge_node", "EDGE_NODE_DT", 32, "JtkEdgeNode"))


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_declared_listed_and_exported(jtk_lib):
    header = re.sub(r"/\*.*?\*/", "", read("include", "jtk_lc.h"), flags=re.S)
    debug = re.sub(r"/\*.*?\*/", "", read("include", "jtk_lc_debug.h"), flags=re.S)
    assert re.search(r"\b%s\s*\(" % NAME, header) and NAME in ffi.EXPORTED_SYMBOLS and hasattr(jtk_lib, NAME)
    assert re.search(r"\b%s\s*\(" % DEBUG, debug) and DEBUG in ffi.DEBUG_SYMBOLS and hasattr(jtk_lib, DEBUG)
    decl = re.search(r"JTK_LC_API int %s\((.*?)\);" % NAME, header, flags=re.S).group(1)
    f = getattr(ffi.lib(), NAME)
    assert len(decl.split(",")) == len(f.argtypes) == 12
    assert "JTK_EDGE_ACCEPTED = 0, JTK_EDGE_REJECTED = 2, JTK_EDGE_NOT_REACHED = 3" in header
    assert (ffi.EDGE_ACCEPTED, ffi.EDGE_REJECTED, ffi.EDGE_NOT_REACHED) == (0, 2, 3)
    assert "encode_edges.hip" in read("jtk_amd", "build.py") and "jtk_lc_*" in read("jtk_amd", "csrc", "exports.map")
    assert jtk_lib.jtk_lc_version() == 2


def c_fields(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s_t;" % (name, name), header, flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            out += [n.strip() for n in decl.split(None, 1)[1].split(",")]
    return out


def test_struct_layouts():
    header = re.sub(r"/\*.*?\*/", "", read("include", "jtk_lc.h"), flags=re.S)
    rust = read("rust", "gpu_ffi.rs")
    for c_name, dt_name, size, r_name in STRUCTS:
        dt = getattr(ffi, dt_name)
        assert list(dt.names) == c_fields(header, c_name), c_name
        assert dt.itemsize == size, c_name
        body = re.search(r"pub struct %s \{(.*?)\}" % r_name, rust, flags=re.S).group(1)
        assert re.findall(r"pub ([a-z_0-9]+)\s*:", body) == list(dt.names), r_name
    ext = re.search(r"pub fn %s\((.*?)\)\s*->" % NAME, rust, flags=re.S).group(1)
    assert len([a for a in ext.split(",") if a.strip()]) == 12
    shim = read("rust", "gpu_shim.rs")
    assert "encode_edges_gpu" in shim and "fn edge_trials" in shim and "dense_encoding.rs:627-697" in shim and "dense_encoding.rs:202-293" in shim


def test_documents_carry_the_call():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md", "SURVEY.md"):
        assert NAME in read(doc), doc
    design = read("DESIGN.md")
    assert "edge_cut_kernel" in design and "not tuned" in design and "fill_gap" in design and "enumerate_polyploid_edges" in design


# ---- invalid arguments

READ = b"ggACGTTGCAAGGCTAtt"             # the window [2, 16) is ACGTTGCAAGGCTA
CONTIG = b"ACGTTGCAAGGCTA"


def call(L, trial=None, breaks=(5, 9, 14), read_seq=READ, contig=CONTIG, node_off=None, ops_cap=None, n=1, null=()):
    """one trial: (read_off, start, end, is_forward, radius, contig_off, contig_len, n_chunks, break_first, sim_thr)"""
    arr = np.zeros(1, dtype=ffi.EDGE_TRIAL_DT)
    arr[0] = trial if trial is not None else (0, 2, 16, 1, 10, 0, len(contig), len(breaks), 0, 0.25)
    rb, cb = (np.frombuffer(bytes(v) + b"\0", np.uint8).copy() for v in (read_seq, contig))
    bp = np.array(list(breaks) + [0], dtype=np.uint32)
    off = np.array([0, int(arr[0]["n_chunks"])] if node_off is None else node_off, dtype=np.uint64)
    cap = int(arr[0]["contig_len"]) + max(int(arr[0]["end"]) - int(arr[0]["start"]), 0) if ops_cap is None else ops_cap
    result = np.zeros(2, dtype=ffi.EDGE_RESULT_DT)
    nodes = np.zeros(int(off[-1]) + 1, dtype=ffi.EDGE_NODE_DT)
    ops, ops_off = np.zeros(cap + 1, np.uint8), np.zeros(int(off[-1]) + 2, np.uint64)
    args = dict(trials=arr.ctypes.data, read_bases=ffi.u8p(rb), contig_bases=ffi.u8p(cb), break_points=ffi.u32p(bp), node_off=ffi.u64p(off),
                result=result.ctypes.data, nodes=nodes.ctypes.data, ops_out=ffi.u8p(ops), ops_out_off=ffi.u64p(ops_off))
    for name in null:
        args[name] = None
    return L.jtk_lc_encode_edges(n, args["trials"], args["read_bases"], args["contig_bases"], args["break_points"], args["node_off"], args["result"],
                                 args["nodes"], args["ops_out"], args["ops_out_off"], cap, 0)


BAD = {
    "start == end": dict(trial=(0, 5, 5, 1, 10, 0, 14, 3, 0, 0.25)),
    "start > end": dict(trial=(0, 9, 5, 1, 10, 0, 14, 3, 0, 0.25)),
    "n_chunks == 0": dict(trial=(0, 2, 16, 1, 10, 0, 14, 0, 0, 0.25), node_off=[0, 0]),
    "an empty contig": dict(trial=(0, 2, 16, 1, 10, 0, 0, 1, 0, 0.25), breaks=(0,)),
    "break points that repeat": dict(breaks=(5, 5, 14)),
    "break points that descend": dict(breaks=(9, 5, 14)),
    "a first break point of 0": dict(breaks=(0, 9, 14)),
    "break points that end short of contig_len": dict(breaks=(5, 9, 13)),
    "break points that end behind contig_len": dict(breaks=(5, 9, 15)),
    "a non-ACGT base in the window": dict(read_seq=b"ggACGTNGCAAGGCTAtt"),
    "a non-ACGT base in the contig": dict(contig=b"ACGTTGCNAGGCTA"),
    "a lower-case base in the contig": dict(contig=b"ACGTTGCaAGGCTA"),
    "ops_cap one byte too small": dict(ops_cap=14 + 14 - 1),
    "node_off that is no prefix sum": dict(node_off=[0, 2]),
    "node_off that does not start at 0": dict(node_off=[1, 4]),
    "null trials": dict(null=("trials",)),
    "null ops_out_off": dict(null=("ops_out_off",)),
    "null nodes": dict(null=("nodes",)),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_invalid_arguments_are_refused_before_the_device_is_looked_for(jtk_lib, what):
    assert call(jtk_lib, **BAD[what]) == -1, what
    assert ffi.lib().jtk_lc_last_error()


def test_a_valid_call_runs_or_fails_loudly(jtk_lib):
    """0 on a machine with a gfx950 device, JTK_ERR_NO_DEVICE without one: there is no fallback.  Bases outside the window may
    be anything, the window may be lower-case"""
    assert call(jtk_lib) in (0, -2)
    assert call(jtk_lib, read_seq=b"NNacgttgcaaggctaNN") in (0, -2)
    assert call(jtk_lib, n=0) in (0, -2)                                 # an empty batch looks for the device too
    if jtk_lib.jtk_lc_device_ok(0) != 1:
        arr, rb, cb, bp = api.pack_edge_trials([dict(read=READ, start=2, end=16, is_forward=True, chunks=[CONTIG[:5], CONTIG[5:]], radius=10, sim_thr=0.25)])
        with pytest.raises(ffi.JtkError) as err:
            api.encode_edges(arr, rb, cb, bp)
        assert err.value.status == -2


def test_pack_edge_trials():
    items = [dict(read=b"ACGTACGT", start=1, end=7, is_forward=True, chunks=[b"ACG", b"TA"], radius=9, sim_thr=0.25),
             dict(read=b"TTGGCCAATT", start=0, end=10, is_forward=False, chunks=[b"GGCC", b"A", b"ATT"], radius=11, sim_thr=0.5)]
    arr, rb, cb, bp = api.pack_edge_trials(items)
    assert arr.dtype == ffi.EDGE_TRIAL_DT and bp.tolist() == [3, 5, 4, 5, 8]
    assert arr[0].tolist() == (0, 1, 7, 1, 9, 0, 5, 2, 0, 0.25) and arr[1].tolist() == (8, 0, 10, 0, 11, 5, 8, 3, 2, 0.5)
    assert bytes(rb[:18]) == b"ACGTACGTTTGGCCAATT" and bytes(cb[:13]) == b"ACGTAGGCCAATT"
