"""jtk_lc_polish_guided through every layer that needs no GPU: the header declares it, the ctypes binding lists it, the library
exports it, the Rust source declares it, bad arguments are refused before a device is looked for, and the documents say that
parity with kiley's polish is not pinned."""
import os
import re

import numpy as np

from jtk_amd import ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("jtk_lc_polish_guided",)
NEW_DEBUG = ("jtk_lc_debug_guided_table", "jtk_lc_debug_gpolish_timing")


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_declared_listed_and_exported(jtk_lib):
    header = re.sub(r"/\*.*?\*/", "", read("include", "jtk_lc.h"), flags=re.S)
    debug = re.sub(r"/\*.*?\*/", "", read("include", "jtk_lc_debug.h"), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in ffi.EXPORTED_SYMBOLS and hasattr(jtk_lib, name), name
        assert "pub fn %s(" % name in read("rust", "gpu_ffi.rs"), name
    for name in NEW_DEBUG:
        assert re.search(r"\b%s\s*\(" % name, debug), name
        assert name in ffi.DEBUG_SYMBOLS and hasattr(jtk_lib, name), name
    assert jtk_lib.jtk_lc_version() == 2
    assert "gpolish.hip" in read("jtk_amd", "build.py")
    shim = read("rust", "gpu_shim.rs")
    assert "take_consensus_gpu" in shim and "jtk_lc_polish_guided" in shim and "deletion_fill.rs:260-285" in shim


def polish_call(L, tmpl=b"ACGTACGT", read_=b"ACGACGT", ops=(0, 0, 0, 3, 0, 0, 0, 0), radius=3, nulls=()):
    tb, rb, ob = (np.frombuffer(bytes(v) + b"\0", np.uint8).copy() for v in (tmpl, read_, bytes(ops)))
    chunks = np.array([(0, 1, 1, 0, len(tmpl), 0)], dtype=ffi.CHUNK_DT)
    read_off, ops_off = np.array([0, len(read_)], np.uint64), np.array([0, len(ops)], np.uint64)
    rad = np.array([radius, 0], np.uint32)
    cons, cons_off = np.zeros(256, np.uint8), np.zeros(2, np.uint64)
    out, out_off, dist = np.zeros(256, np.uint8), np.zeros(2, np.uint64), np.zeros(2, np.uint32)
    result = np.zeros(2, dtype=ffi.RESULT_DT)
    args = dict(chunks=chunks.ctypes.data, tmpl=ffi.u8p(tb), reads=ffi.u8p(rb), read_off=ffi.u64p(read_off), ops=ffi.u8p(ob), ops_off=ffi.u64p(ops_off),
                radius=ffi.u32p(rad), cons=ffi.u8p(cons), cons_off=ffi.u64p(cons_off), out=ffi.u8p(out), out_off=ffi.u64p(out_off), dist=ffi.u32p(dist),
                result=result.ctypes.data)
    for k in nulls:
        args[k] = None
    return L.jtk_lc_polish_guided(1, args["chunks"], args["tmpl"], args["reads"], args["read_off"], args["ops"], args["ops_off"], args["radius"], 0, 0, 0,
                                  args["cons"], args["cons_off"], 256, args["out"], args["out_off"], 256, args["dist"], args["result"], 0)


def test_bad_arguments_are_refused_before_the_device_is_looked_for(jtk_lib):
    L = jtk_lib
    assert polish_call(L) in (0, -2)                         # JTK_ERR_NO_DEVICE on a machine without one: there is no fallback
    assert polish_call(L, radius=0) == -1
    assert polish_call(L, tmpl=b"ACGTNCGT") == -1 and polish_call(L, read_=b"ACGNCGT") == -1 and polish_call(L, read_=b"acgacgt") == -1
    assert polish_call(L, ops=(0, 0, 0, 4, 0, 0, 0, 0)) == -1
    for name in ("chunks", "tmpl", "reads", "read_off", "ops", "ops_off", "radius", "cons", "cons_off", "out", "out_off", "dist", "result"):
        assert polish_call(L, nulls=(name,)) == -1, name
    # chunks that do not list their reads back to back, as for jtk_lc_polish_chunks
    chunks = np.array([(0, 1, 1, 0, 4, 1)], dtype=ffi.CHUNK_DT)
    z8, z64, z32 = np.zeros(16, np.uint8), np.zeros(4, np.uint64), np.ones(4, np.uint32)
    res = np.zeros(2, dtype=ffi.RESULT_DT)
    assert L.jtk_lc_polish_guided(1, chunks.ctypes.data, ffi.u8p(z8), ffi.u8p(z8), ffi.u64p(z64), ffi.u8p(z8), ffi.u64p(z64), ffi.u32p(z32), 0, 0, 0,
                                  ffi.u8p(z8), ffi.u64p(z64), 16, ffi.u8p(z8), ffi.u64p(z64), 16, ffi.u32p(z32), res.ctypes.data, 0) == -1
    # the debug entry takes a radius of 0 but no bad base
    tb, rb, ob = (np.frombuffer(v + b"\0", np.uint8).copy() for v in (b"ACGT", b"ACNT", bytes((0, 0, 0, 0))))
    off = np.array([0, 4], np.uint64)
    table = np.zeros(5 * 14, np.uint32)
    assert L.jtk_lc_debug_guided_table(ffi.u8p(tb), 4, 1, ffi.u8p(rb), ffi.u64p(off), ffi.u8p(ob), ffi.u64p(off), 0, ffi.u32p(z32), ffi.u32p(table), 70, 0) == -1


def test_documents_state_the_unpinned_parity():
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md", "SURVEY.md"):
        text = read(doc)
        assert "jtk_lc_polish_guided" in text, doc
        near = [m.start() for m in re.finditer("jtk_lc_polish_guided", text)]
        assert any(re.search(r"parity with kiley[^.]*not pinned", text[max(0, at - 1500):at + 1500], flags=re.S | re.I) for at in near), doc
    assert "Guided polishing" in read("DESIGN.md")
    assert "`take_consensus_sequence` is `jtk_lc_polish_chunks`" not in read("README.md")
