"""jtk_lc_map_reads, jtk_lc_sketch and jtk_lc_debug_map_timing through every layer that needs no GPU: the headers declare them and
the two structs, the ctypes dtypes agree with the C compiler on size and offsets, the library exports them, the build list and
the Rust sources carry them, every invalid argument and every limit is refused before a device is looked for, api.map_trials is
the arithmetic of tests/map_reference.py, and dataset.encode_by_map -- with its three device calls replaced by the Python
references -- writes encoded_reads and nothing else, with every read's nodes in the order encode_read_to_nodes_by_paf leaves."""
import copy
import ctypes as C
import json
import os
import random
import re
import subprocess

import numpy as np
import pytest

import map_cases as K
import map_reference as R
import map_stage_reference as MS
from jtk_amd import api, dataset as D, ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"jtk_lc_map_reads": 11, "jtk_lc_sketch": 12}
DEBUG = "jtk_lc_debug_map_timing"


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
    assert re.search(r"\b%s\s*\(" % DEBUG, debug) and DEBUG in ffi.DEBUG_SYMBOLS and hasattr(jtk_lib, DEBUG) and DEBUG in rust
    assert "map.hip" in read("jtk_amd", "build.py")
    shim = read("rust", "gpu_shim.rs")
    assert "fn map_reads_gpu" in shim and "encode/mod.rs:41-64" in shim and "minimap2.rs" in shim and "jtk_lc_map_reads(" in shim
    assert "tstart < 25" in shim                                          # the PAF filter it replaces


@pytest.mark.parametrize("c_name,rust_name,dt", [("jtk_map_params", "JtkMapParams", ffi.MAP_PARAMS_DT),
                                                 ("jtk_map_placement", "JtkMapPlacement", ffi.MAP_PLACEMENT_DT)])
def test_the_struct_layouts_by_the_c_compiler(tmp_path, c_name, rust_name, dt):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "jtk_lc.h"', 'int main(void) {',
             'printf("{\\"sizeof\\": %%zu", sizeof(%s_t));' % c_name]
    for f in dt.names:
        lines.append('printf(", \\"%s\\": %%zu", offsetof(%s_t, %s));' % (f, c_name, f))
    lines += ['printf("}\\n");', 'return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic-errors", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = json.loads(subprocess.check_output([str(exe)]))
    assert got.pop("sizeof") == dt.itemsize == 4 * len(dt.names)
    assert got == {f: dt.fields[f][1] for f in dt.names}
    header = re.sub(r"/\*.*?\*/", "", read("include", "jtk_lc.h"), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s_t;" % (c_name, c_name), header, flags=re.S).group(1)
    fields = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert fields == list(dt.names)
    body = re.search(r"pub struct %s \{(.*?)\}" % rust_name, read("rust", "gpu_ffi.rs"), flags=re.S).group(1)
    assert re.findall(r"pub ([a-z_0-9]+)\s*:", body) == list(dt.names)
    assert dt.fields["diag_lo"][0] == np.dtype("<i4") if "diag_lo" in dt.names else True
    assert tuple(dt.names) == (R.FIELDS if "query" in dt.names else ("k", "w", "max_occ", "max_gap", "min_seeds", "skip_self"))


GOOD = dict(bases=b"ACGTACGTNNACGT", off=[0, 8, 14])


def flat(bases, off):
    return np.frombuffer(bases, dtype=np.uint8).copy(), np.asarray(off, dtype=np.uint64)


def map_call(tb=GOOD["bases"], toff=GOOD["off"], qb=GOOD["bases"], qoff=GOOD["off"], k=3, w=2, min_seeds=1, cap=4, device=99, null=()):
    (tb, toff), (qb, qoff) = flat(tb, toff), flat(qb, qoff)
    params = np.array([(k, w, 10, 100, min_seeds, 0)], dtype=ffi.MAP_PARAMS_DT)
    out, n = np.zeros(cap + 1, dtype=ffi.MAP_PLACEMENT_DT), np.zeros(1, np.uint64)
    args = dict(tb=ffi.u8p(tb), toff=ffi.u64p(toff), qb=ffi.u8p(qb), qoff=ffi.u64p(qoff), params=params.ctypes.data, out=out.ctypes.data, n=ffi.u64p(n))
    for name in null:
        args[name] = None
    return ffi.lib().jtk_lc_map_reads(len(toff) - 1, args["tb"], args["toff"], len(qoff) - 1, args["qb"], args["qoff"], args["params"], args["out"], cap,
                                      args["n"], device)


def sketch_call(bases=GOOD["bases"], off=GOOD["off"], k=3, w=2, cap=4, device=99, null=()):
    bases, off = flat(bases, off)
    h, s, p, st, n = np.zeros(cap + 1, np.uint64), np.zeros(cap + 1, np.uint32), np.zeros(cap + 1, np.uint32), np.zeros(cap + 1, np.uint8), np.zeros(1, np.uint64)
    args = dict(bases=ffi.u8p(bases), off=ffi.u64p(off), hash=ffi.u64p(h), seq=ffi.u32p(s), pos=ffi.u32p(p), strand=ffi.u8p(st), n=ffi.u64p(n))
    for name in null:
        args[name] = None
    return ffi.lib().jtk_lc_sketch(len(off) - 1, args["bases"], args["off"], k, w, args["hash"], args["seq"], args["pos"], args["strand"], cap, args["n"],
                                   device)


def test_invalid_arguments_and_limits_are_refused_before_a_device_is_looked_for(jtk_lib):
    for call in (map_call, sketch_call):
        assert call() == -2, call.__name__                               # valid: the only thing missing is device 99
        assert jtk_lib.jtk_lc_last_error().decode() != ""
        assert call(k=0) == -1 and call(w=0) == -1
        assert call(k=32) == -3 and call(k=31) == -2 and call(w=65) == -3 and call(w=64) == -2
        assert call(k=0, w=65) == -1                                      # an invalid argument is named before a limit
    assert map_call(min_seeds=0) == -1
    assert map_call(toff=[1, 8, 14]) == -1 and map_call(toff=[0, 9, 8]) == -1 and map_call(qoff=[1, 8, 14]) == -1 and map_call(qoff=[0, 9, 8]) == -1
    assert sketch_call(off=[1, 8, 14]) == -1 and sketch_call(off=[0, 9, 8]) == -1
    for name in ("tb", "toff", "qb", "qoff", "params", "out", "n"):
        assert map_call(null=(name,)) == -1, name
    for name in ("bases", "off", "hash", "seq", "pos", "strand", "n"):
        assert sketch_call(null=(name,)) == -1, name
    assert map_call(null=("out",), cap=0) == -2 and sketch_call(null=("hash", "seq", "pos", "strand"), cap=0) == -2     # only the need is asked for
    assert map_call(tb=b"", toff=[0, 0], null=("tb",)) == -2 and sketch_call(bases=b"", off=[0, 0, 0], null=("bases",)) == -2
    # the limits of DESIGN section 4: a target of 65,535 bases, a query of 4,000,000, 2^25 targets
    long_target = b"A" * (ffi.MAP_MAX_TARGET_LEN + 1)
    assert map_call(tb=long_target, toff=[0, len(long_target)]) == -3 and map_call(tb=long_target[:-1], toff=[0, len(long_target) - 1]) == -2
    long_query = b"A" * (ffi.MAP_MAX_QUERY_LEN + 1)
    assert map_call(qb=long_query, qoff=[0, len(long_query)]) == -3 and map_call(qb=long_query[:-1], qoff=[0, len(long_query) - 1]) == -2
    assert sketch_call(bases=long_query, off=[0, len(long_query)]) == -2  # the sketch alone takes longer sequences
    many = np.zeros(ffi.MAP_MAX_TARGETS + 2, dtype=np.uint64)
    assert map_call(tb=b"", toff=many, null=("tb",)) == -3 and map_call(tb=b"", toff=many[:-1], null=("tb",)) == -2
    assert (ffi.MAP_MAX_K, ffi.MAP_MAX_W, ffi.MAP_MAX_TARGET_LEN, ffi.MAP_MAX_QUERY_LEN, ffi.MAP_MAX_TARGETS) == (
        R.MAX_K, R.MAX_W, R.MAX_TARGET_LEN, R.MAX_QUERY_LEN, R.MAX_TARGETS)


def test_map_trials_is_the_reference_arithmetic():
    rng = random.Random(3)
    qlens, tlens = [5000, 300, 2100], [2000, 150]
    placements = []
    for _ in range(300):
        q, t = rng.randrange(3), rng.randrange(2)
        ts = rng.randrange(0, tlens[t] - 20)
        te = rng.randrange(ts + 15, tlens[t] + 1)
        qs = rng.randrange(0, qlens[q] - 20)
        qe = min(qs + (te - ts) + rng.randrange(-5, 6), qlens[q])
        fw = rng.randrange(2)
        placements.append(dict(query=q, target=t, is_forward=fw, n_seeds=5, qstart=qs if fw else qlens[q] - qe, qend=qe if fw else qlens[q] - qs,
                               oq_start=qs, oq_end=qe, tstart=ts, tend=te, diag_lo=qs - ts, diag_hi=qs - ts))
    want = R.map_trials(placements, qlens, tlens, 0.25)
    packed = np.array([tuple(p[f] for f in ffi.MAP_PLACEMENT_DT.names) for p in placements], dtype=ffi.MAP_PLACEMENT_DT)
    assert api.map_trials(packed, qlens, tlens, 0.25) == want and 0 < len(want) < len(placements)
    assert (api.ALLOWED_END_GAP, api.OFFSET_FACTOR) == (R.ALLOWED_END_GAP, R.OFFSET_FACTOR) == (25, 0.1)
    # a placement that spans the whole chunk at the read's very start, forward and reverse: the window is clipped and mirrored
    whole = dict(query=0, target=0, n_seeds=9, oq_start=0, oq_end=2000, tstart=0, tend=2000, diag_lo=0, diag_hi=0)
    assert R.map_trials([dict(whole, is_forward=1, qstart=0, qend=2000)], qlens, tlens, 0.1) == [(0, 0, 2200, 1, 0.1)]
    assert R.map_trials([dict(whole, is_forward=0, qstart=3000, qend=5000)], qlens, tlens, 0.1) == [(0, 2800, 5000, 0, 0.1)]
    # 26 bases of the chunk would lie in front of the read: dropped; 25: kept
    assert R.map_trials([dict(whole, is_forward=1, tstart=26, oq_end=1974, qstart=0, qend=1974)], qlens, tlens, 0.1) == []
    assert len(R.map_trials([dict(whole, is_forward=1, tstart=25, oq_end=1975, qstart=0, qend=1975)], qlens, tlens, 0.1)) == 1


def test_the_stage_writes_encoded_reads_and_nothing_else(monkeypatch):
    monkeypatch.setattr(api, "map_reads", MS.map_reads)
    monkeypatch.setattr(api, "encode_nodes", MS.encode_nodes)
    monkeypatch.setattr(api, "settle_nodes", MS.settle_nodes)
    ds = MS.small_data_set()
    ds["encoded_reads"] = [{"id": 1, "stale": True}]
    before = copy.deepcopy(ds)
    params = dict(k=11, w=5, min_seeds=3)
    D.encode_by_map(ds, 0.2, **params)
    got = ds.pop("encoded_reads")
    before.pop("encoded_reads")
    assert ds == before
    want = copy.deepcopy(before)
    MS.encode_by_map(want, 0.2, **params)
    assert got == want["encoded_reads"]
    ids = [r["id"] for r in got]
    assert ids == [100, 101, 102, 104]                                     # raw-read order; the unrelated read is dropped
    assert [[n["chunk"] for n in r["nodes"]] for r in got] == [[10, 11, 12], [11, 10], [11, 11], [10, 11, 12]]
    assert [[n["is_forward"] for n in r["nodes"]] for r in got] == [[True] * 3, [False] * 2, [True] * 2, [True] * 3]
    for r in got:                                                          # as encode_read_to_nodes_by_paf leaves them: by position
        starts = [n["position_from_start"] for n in r["nodes"]]
        assert starts == sorted(starts) and all(n["cluster"] == 0 and n["posterior"] == [0.0] for n in r["nodes"])
        assert D.is_uppercase(r)
    ds["encoded_reads"] = got
    D.validate(ds)
    D.sanity_check(ds)


def test_one_read_of_the_recorded_stage_result():
    """tests/golden/encode_stage_planted.json is what tests/map_stage_reference.py computes: recomputed here for the read with the
    fewest bases among those with a single node (a few seconds of plain Python; the whole set takes a minute)"""
    rec = MS.recorded()
    assert (rec["sim_thr"], rec["sd_of_error"]) == (MS.SIM_THR, MS.SD_OF_ERROR)
    ds, p = MS.planted_data_set()
    assert [r["id"] for r in rec["encoded_reads"]] == [r["id"] for r in ds["raw_reads"][:-1]]      # all but the unrelated read
    pick = min((r for r in rec["encoded_reads"] if len(r["nodes"]) == 1), key=lambda r: r["original_length"])
    ds["raw_reads"] = [r for r in ds["raw_reads"] if r["id"] == pick["id"]]
    MS.encode(ds, MS.SIM_THR, MS.SD_OF_ERROR)
    assert ds["encoded_reads"] == [pick]
