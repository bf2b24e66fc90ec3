"""jtk_lc_mask_repeats, jtk_lc_repetitive_kmers and jtk_lc_repetitiveness through every layer that needs no GPU: the header declares
them and jtk_mask_report_t, the ctypes binding agrees on its size, offsets and field order (asked of the C compiler), the library
exports them, the build list and the Rust sources carry them, every invalid argument is refused before a device is looked for,
and the stage built on them touches raw_reads[*].seq and masked_kmers.k only."""
import copy
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import mask_reference as R
from jtk_amd import api, dataset as D, ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"jtk_lc_mask_repeats": 11, "jtk_lc_repetitive_kmers": 8, "jtk_lc_repetitiveness": 9}
DEBUG = "jtk_lc_debug_mask_timing"


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_declared_listed_and_exported(jtk_lib):
    header = re.sub(r"/\*.*?\*/", "", read("include", "jtk_lc.h"), flags=re.S)
    debug = re.sub(r"/\*.*?\*/", "", read("include", "jtk_lc_debug.h"), flags=re.S)
    rust = read("rust", "gpu_ffi.rs")
    for name, n_args in NAMES.items():
        assert re.search(r"\b%s\s*\(" % name, header) and name in ffi.EXPORTED_SYMBOLS and hasattr(jtk_lib, name), name
        decl = re.search(r"JTK_LC_API int %s\((.*?)\);" % name, header, flags=re.S).group(1)
        assert len(decl.split(",")) == len(getattr(ffi.lib(), name).argtypes) == n_args, name
        ext = re.search(r"pub fn %s\((.*?)\)\s*->" % name, rust, flags=re.S).group(1)
        assert len([a for a in ext.split(",") if a.strip()]) == n_args, name
    assert re.search(r"\b%s\s*\(" % DEBUG, debug) and DEBUG in ffi.DEBUG_SYMBOLS and hasattr(jtk_lib, DEBUG)
    assert "mask.hip" in read("jtk_amd", "build.py")
    assert jtk_lib.jtk_lc_version() == 2
    shim = read("rust", "gpu_shim.rs")
    assert "fn mask_repeat_gpu" in shim and "repeat_masking.rs:135-158" in shim and "jtk_lc_mask_repeats(" in shim
    assert "fn repetitiveness_gpu" in shim and "repeat_masking.rs:90-105" in shim and "jtk_lc_repetitiveness(" in shim


def test_the_report_layout_by_the_c_compiler(tmp_path):
    dt = ffi.MASK_REPORT_DT
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "jtk_lc.h"', 'int main(void) {',
             'printf("{\\"sizeof\\": %zu", sizeof(jtk_mask_report_t));']
    for f in dt.names:
        lines.append('printf(", \\"%s\\": %%zu", offsetof(jtk_mask_report_t, %s));' % (f, f))
    lines += ['printf("}\\n");', 'return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic-errors", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = json.loads(subprocess.check_output([str(exe)]))
    assert got.pop("sizeof") == dt.itemsize == 56
    assert got == {f: dt.fields[f][1] for f in dt.names}
    header = re.sub(r"/\*.*?\*/", "", read("include", "jtk_lc.h"), flags=re.S)
    body = re.search(r"typedef struct jtk_mask_report \{(.*?)\} jtk_mask_report_t;", header, flags=re.S).group(1)
    fields = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert fields == list(dt.names)
    body = re.search(r"pub struct JtkMaskReport \{(.*?)\}", read("rust", "gpu_ffi.rs"), flags=re.S).group(1)
    assert re.findall(r"pub ([a-z_0-9]+)\s*:", body) == list(dt.names)


GOOD = dict(bases=b"ACGTACGTNNACGT", off=[0, 8, 14])


def mask_call(bases=GOOD["bases"], off=GOOD["off"], k=3, freq=0.5, min_count=1, cap=4, device=99, null=()):
    bases, off = np.frombuffer(bases, dtype=np.uint8).copy(), np.asarray(off, dtype=np.uint64)
    out, kmers, report = np.zeros(len(bases) + 1, np.uint8), np.zeros(cap + 1, np.uint64), np.zeros(1, ffi.MASK_REPORT_DT)
    args = dict(bases=ffi.u8p(bases), off=ffi.u64p(off), out=ffi.u8p(out), kmers=ffi.u64p(kmers), report=report.ctypes.data)
    for name in null:
        args[name] = None
    return ffi.lib().jtk_lc_mask_repeats(len(off) - 1, args["bases"], args["off"], k, freq, min_count, args["out"], args["kmers"], cap, args["report"], device)


def kmers_call(bases=GOOD["bases"], off=GOOD["off"], k=3, cap=4, device=99, null=()):
    bases, off = np.frombuffer(bases, dtype=np.uint8).copy(), np.asarray(off, dtype=np.uint64)
    kmers, n = np.zeros(cap + 1, np.uint64), np.zeros(1, np.uint64)
    args = dict(bases=ffi.u8p(bases), off=ffi.u64p(off), kmers=ffi.u64p(kmers), n=ffi.u64p(n))
    for name in null:
        args[name] = None
    return ffi.lib().jtk_lc_repetitive_kmers(len(off) - 1, args["bases"], args["off"], k, args["kmers"], cap, args["n"], device)


def rep_call(bases=GOOD["bases"], off=GOOD["off"], k=3, kmers=(9, 36), device=99, null=()):
    bases, off = np.frombuffer(bases, dtype=np.uint8).copy(), np.asarray(off, dtype=np.uint64)
    kmers = np.asarray(kmers, dtype=np.uint64)
    num, den = np.zeros(len(off), np.uint32), np.zeros(len(off), np.uint32)
    args = dict(bases=ffi.u8p(bases), off=ffi.u64p(off), kmers=ffi.u64p(kmers), num=ffi.u32p(num), den=ffi.u32p(den))
    for name in null:
        args[name] = None
    return ffi.lib().jtk_lc_repetitiveness(len(off) - 1, args["bases"], args["off"], k, args["kmers"], len(kmers), args["num"], args["den"], device)


def test_invalid_arguments_are_refused_before_a_device_is_looked_for(jtk_lib):
    for call in (mask_call, kmers_call, rep_call):
        assert call() == -2, call.__name__                               # valid: the only thing missing is device 99
        assert jtk_lib.jtk_lc_last_error().decode() != ""
        assert call(k=0) == -1 and call(k=32) == -3 and call(k=33) == -3 and call(k=31) == -2 and call(k=1) == -2
        assert call(off=[1, 8, 14]) == -1 and call(off=[0, 9, 8]) == -1   # does not start at 0; decreases
        assert call(null=("bases",)) == -1 and call(null=("off",)) == -1
        assert call(bases=b"", off=[0, 0, 0], null=("bases",)) == -2      # no bases: no pointer to them is needed
    for freq in (float("nan"), -0.001, 1.001, float("inf")):
        assert mask_call(freq=freq) == -1, freq
    assert mask_call(freq=0.0) == -2 and mask_call(freq=1.0) == -2
    assert mask_call(null=("out",)) == -1 and mask_call(null=("report",)) == -1 and mask_call(null=("kmers",)) == -1
    assert mask_call(null=("kmers",), cap=0) == -2                        # the mask is not asked for
    assert kmers_call(null=("n",)) == -1 and kmers_call(null=("kmers",)) == -1 and kmers_call(null=("kmers",), cap=0) == -2
    assert rep_call(null=("num",)) == -1 and rep_call(null=("den",)) == -1 and rep_call(null=("kmers",)) == -1
    assert rep_call(null=("kmers",), kmers=()) == -2
    # five sequences need three bits above the 62 of a 31-mer
    assert rep_call(bases=b"", off=[0] * 6, k=31) == -3 and rep_call(bases=b"", off=[0] * 5, k=31) == -2 and rep_call(bases=b"", off=[0] * 6, k=30) == -2


def a_data_set():
    reads = [b"acgacgacgtttnaacgtac", b"NNNN", b""]
    return {"input_file": "x.fa", "masked_kmers": {"k": 0, "thr": 41}, "coverage": {"Estimated": 3.5},
            "raw_reads": [{"name": "r%d" % i, "desc": "d", "id": i, "seq": r.decode()} for i, r in enumerate(reads)], "hic_pairs": [],
            "selected_chunks": [{"id": 1, "seq": "acgt", "cluster_num": 1, "copy_num": 1, "score": 0.0}], "encoded_reads": [], "hic_edges": [],
            "read_type": "ONT", "model_param": {"forward": {}, "reverse": {}}, "error_rate": {}, "processed_stages": [{"stage_name": "s", "arg": []}]}


def by_the_reference(reads, k, freq, min_count, device=0):
    out, report, mask, rc = R.mask_repeat(reads, k, freq, min_count)
    return out, dict(report, rc=rc), np.array(mask, dtype=np.uint64)


def test_the_stage_writes_the_reads_and_k_and_nothing_else(monkeypatch):
    monkeypatch.setattr(api, "mask_repeats", by_the_reference)
    ds = a_data_set()
    before = copy.deepcopy(ds)
    rows = []
    report = D.mask_repeat(ds, k=3, freq=0.3, min_count=1, record=rows)
    assert [r["seq"] for r in ds["raw_reads"]] == ["acgacgacgtTTNAacgtAC", "NNNN", ""] and ds["masked_kmers"] == {"k": 3, "thr": 41}
    assert report["n_lower"] == 14 and rows == ["MASKREPEAT\tMaskLen\t3\t1", "MASKREPEAT\tTotalMask\t14\t24", "MASKREPEAT\tMaskedKmers\t1\t3"]
    for r, b in zip(ds["raw_reads"], before["raw_reads"]):
        r["seq"] = b["seq"]
    ds["masked_kmers"]["k"] = 0
    assert ds == before
    with pytest.raises(ffi.JtkError) as err:                             # freq = 0: the reference panics
        D.mask_repeat(ds, k=3, freq=0.0, min_count=1)
    assert err.value.status == -6 and ds == before
    import inspect
    defaults = {n: p.default for n, p in inspect.signature(D.mask_repeat).parameters.items()}
    assert (defaults["k"], defaults["freq"], defaults["min_count"]) == (12, 0.001, 10)    # example.toml
