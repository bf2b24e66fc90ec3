"""jtk_lc_align_guided and jtk_lc_encode_nodes through every layer that needs no GPU: the header declares them, the ctypes
binding lists them and agrees on the struct sizes, the library exports them, the Rust source declares them, and bad arguments
are refused before a device is looked for."""
import ctypes as C
import os
import re

import numpy as np

from jtk_amd import api, ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("jtk_lc_align_guided", "jtk_lc_encode_nodes")
NEW_DEBUG = ("jtk_lc_debug_guided_scratch_cap", "jtk_lc_debug_guided_timing", "jtk_lc_debug_encode_timing")


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_declared_listed_and_exported(jtk_lib):
    header = re.sub(r"/\*.*?\*/", "", read("include", "jtk_lc.h"), flags=re.S)
    debug = re.sub(r"/\*.*?\*/", "", read("include", "jtk_lc_debug.h"), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in ffi.EXPORTED_SYMBOLS and hasattr(jtk_lib, name), name
    for name in NEW_DEBUG:
        assert re.search(r"\b%s\s*\(" % name, debug), name
        assert name in ffi.DEBUG_SYMBOLS and hasattr(jtk_lib, name), name
    assert "#define JTK_GUIDED_MAX_WIDTH %d" % ffi.GUIDED_MAX_WIDTH in header and ffi.GUIDED_MAX_WIDTH >= 2048
    assert jtk_lib.jtk_lc_version() == 2
    assert "guided.hip" in read("jtk_amd", "build.py") and "encode_nodes.hip" in read("jtk_amd", "build.py")


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
    for c_name, dt, size, r_name in (("jtk_guided_pair", ffi.GUIDED_PAIR_DT, 40, "JtkGuidedPair"), ("jtk_encode_trial", ffi.ENCODE_TRIAL_DT, 56, "JtkEncodeTrial"),
                                     ("jtk_encode_result", ffi.ENCODE_RESULT_DT, 64, "JtkEncodeResult")):
        assert list(dt.names) == c_fields(header, c_name), c_name
        assert dt.itemsize == size, c_name
        body = re.search(r"pub struct %s \{(.*?)\}" % r_name, rust, flags=re.S).group(1)
        assert re.findall(r"pub ([a-z_0-9]+)\s*:", body) == list(dt.names), r_name
    for name in NEW:
        assert "pub fn %s(" % name in rust, name
    assert "encode_nodes_gpu" in read("rust", "gpu_shim.rs") and "fill_trials" in read("rust", "gpu_shim.rs")


def guided_call(L, mode=0, scores=(2, -6, -5, -1), x=b"ACGT", y=b"ACGT", guide=(0, 0, 0, 0), pairs=None):
    xb, yb, gb = (np.frombuffer(bytes(v) + b"\0", np.uint8).copy() for v in (x, y, bytes(guide)))
    if pairs is None:
        pairs = np.array([(0, 0, 0, len(x), len(y), len(guide), 2)], dtype=ffi.GUIDED_PAIR_DT)
    n = len(pairs)
    ops, off = np.zeros(64, np.uint8), np.zeros(n + 1, np.uint64)
    score, status, start, end = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    PI32 = C.POINTER(C.c_int32)
    return L.jtk_lc_align_guided(n, pairs.ctypes.data, ffi.u8p(xb), ffi.u8p(yb), ffi.u8p(gb), mode, *scores, ffi.u8p(ops), ffi.u64p(off), 64,
                                 score.ctypes.data_as(PI32), ffi.u32p(start), ffi.u32p(end), status.ctypes.data_as(PI32), 0)


def test_bad_arguments_are_refused_before_the_device_is_looked_for(jtk_lib):
    L = jtk_lib
    good = guided_call(L)
    assert good in (0, -2)                                   # JTK_ERR_NO_DEVICE on a machine without one: there is no fallback
    assert guided_call(L, mode=2) == -1                      # prefix is no mode of this call
    for scores in ((2, -6, -1, -5), (2, -6, -5, 1), (2, 1, -5, -1), (-1, -6, -5, -1), (2000, -6, -5, -1), (2, -6, -5000, -1)):
        assert guided_call(L, scores=scores) == -1, scores
    assert guided_call(L, x=b"ACNT") == -1 and guided_call(L, y=b"acgt") == -1 and guided_call(L, guide=(0, 4, 0, 0)) == -1
    assert L.jtk_lc_align_guided(1, None, None, None, None, 0, 2, -6, -5, -1, None, None, 0, None, None, None, None, 0) == -1
    trial = np.zeros(1, dtype=ffi.ENCODE_TRIAL_DT)
    trial[0] = (0, 3, 3, 1, 4, 0, 0, 4, 0, 0.25)             # start == end: the reference asserts start < end
    buf = np.frombuffer(b"ACGTACGT\0", np.uint8).copy()
    res, off = np.zeros(1, dtype=ffi.ENCODE_RESULT_DT), np.zeros(2, np.uint64)
    args = (ffi.u8p(buf), ffi.u8p(buf), ffi.u8p(buf), res.ctypes.data, ffi.u8p(np.zeros(16, np.uint8)), ffi.u64p(off), 16, 0)
    assert L.jtk_lc_encode_nodes(1, trial.ctypes.data, *args) == -1
    trial[0] = (0, 0, 4, 1, 0, 0, 0, 4, 0, 0.25)             # an empty consensus
    assert L.jtk_lc_encode_nodes(1, trial.ctypes.data, *args) == -1
    trial[0] = (0, 0, 4, 1, 4, 0, 0, 4, 0, 0.25)
    assert L.jtk_lc_encode_nodes(1, trial.ctypes.data, *args) in (0, -2)
    assert L.jtk_lc_encode_nodes(1, None, *args) == -1


def test_documents_state_the_unpinned_parity():
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        text = read(doc)
        assert "jtk_lc_align_guided" in text and "jtk_lc_encode_nodes" in text, doc
        assert re.search(r"parity with kiley[^.]*not pinned", text, flags=re.S | re.I), doc
