"""squish_erroneous_clusters without a device: the Python reference (tests/squish_reference.py) on the problems of
tests/squish_cases.py, its generator and its adjusted Rand index against independent statements, and the host-only entry point
jtk_lc_squish_classify, the declarations and the dataset.py stages against the reference."""
import ctypes as C
import copy
import itertools
import json
import os
import random

import numpy as np
import pytest

import clustering_reference as CR
import squish_cases as K
import squish_reference as R
from jtk_amd import api, dataset as D, ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


def reference(name, math="project"):
    """squish_reference.squish on a case, computed once per (case, exp) and shared by every test (GPU module included)"""
    if (name, math) not in _cache:
        exp = CR.ProjectMath().exp if math == "project" else CR.LibmMath.exp
        stats = {}
        res = R.squish(K.CASES[name]["ds"], K.CASES[name].get("cfg"), exp=exp, stats=stats)
        res["stats"] = stats
        _cache[(name, math)] = res
    return _cache[(name, math)]


def config_of(name):
    return ffi.SquishConfig(**dict(R.DEFAULT_CONFIG, **K.CASES[name].get("cfg", {})))


# ---- the generator

def test_xoshiro256plusplus_known_answers():
    g = R.Xoshiro256PlusPlus([1, 2, 3, 4])
    assert [g.next_u64() for _ in range(2)] == [41943041, 58720359]     # derived by hand from the recurrence
    # the next outputs follow from the state update alone: evaluate it once more, written out separately
    s = [1, 2, 3, 4]
    outs = []
    for _ in range(6):
        outs.append((R._rotl((s[0] + s[3]) & R.M64, 23) + s[0]) & R.M64)
        t = (s[1] << 17) & R.M64
        s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3]; s[2] ^= t   # noqa: E702
        s[3] = R._rotl(s[3], 45)
    g = R.Xoshiro256PlusPlus([1, 2, 3, 4])
    assert [g.next_u64() for _ in range(6)] == outs and outs[2:4] == [3588806011781223, 3591011842654386]
    # seed_from_u64 is SplitMix64 (known answers for x = 1234567: SURVEY.md 8c)
    assert R.Xoshiro256PlusPlus.seed_from_u64(1234567).s[:3] == [6457827717110365317, 3203168211198807973, 9817491932198370423]


def test_gen_range_and_gen_bool_follow_rand_085():
    class Fixed:
        def __init__(self, vals):
            self.vals = list(vals)

        def next_u64(self):
            return self.vals.pop(0)
    # n = 3: zone = (3 << 62) - 1; a draw whose low product word is above the zone is rejected
    r = R.Rand085(Fixed([R.M64, 1 << 63, 5]))
    assert (R.M64 * 3) & R.M64 > ((3 << 62) - 1) and r.gen_range(3) == 1 and r.draws == 2
    r = R.Rand085(Fixed([(1 << 63) - 1, 1 << 63]))
    assert r.gen_bool(1.0) is True and r.draws == 0 and r.no_draw == 1          # p == 1: no draw
    assert r.gen_bool(0.5) is True and r.gen_bool(0.5) is False and r.draws == 2   # u < 2^63
    assert R.Rand085(Fixed([0])).gen_bool(0.0) is False


# ---- the adjusted Rand index

def _ari_by_pairs(label, pred):
    """the pair-counting definition, with the integer quirks of misc.rs:34-45: floor of the mean, i64 casts, one f64 division"""
    n = len(label)
    same_l = same_p = same_both = 0
    for i, j in itertools.combinations(range(n), 2):
        same_l += label[i] == label[j]
        same_p += pred[i] == pred[j]
        same_both += label[i] == label[j] and pred[i] == pred[j]
    total = n * (n - 1) // 2
    numer, denom = total * same_both - same_l * same_p, total * (same_l + same_p) // 2 - same_l * same_p
    if denom == 0:
        return float("nan") if numer == 0 else float("inf") * (1 if numer > 0 else -1)
    return numer / denom


def test_adjusted_rand_index_against_pair_counting():
    rng = random.Random(3)
    seen_nan = 0
    for _ in range(600):
        n = rng.randrange(1, 14)
        ka, kb = rng.randrange(1, 5), rng.randrange(1, 5)
        a, b = [rng.randrange(ka) for _ in range(n)], [rng.randrange(kb) for _ in range(n)]
        got, want = R.adjusted_rand_index(a, b), _ari_by_pairs(a, b)
        assert (got != got and want != want) or got == want, (a, b)
        seen_nan += got != got
    for a, b in (([0, 1], [0, 0]), ([0], [0])):     # 0 / 0
        assert R.adjusted_rand_index(a, b) != R.adjusted_rand_index(a, b)
    assert seen_nan > 0
    # the floor in num_of_pairs * (lab_match + pred_match) / 2 shows when that product is odd: 3 * (1 + 0) / 2 = 1, ARI 0 / 1
    assert R.adjusted_rand_index([0, 0, 1], [0, 1, 2]) == 0.0 == _ari_by_pairs([0, 0, 1], [0, 1, 2])
    assert R.adjusted_rand_index([0, 1, 1, 1, 1, 1], [2, 0, 1, 1, 1, 1]) == 0.5


# ---- the cases

@pytest.mark.parametrize("name", K.NAMES)
def test_cases_go_where_they_were_built_to_go(name):
    case, res = K.CASES[name], reference(name)
    assert res["status"] == case.get("status", 0)
    if res["status"] != 0:
        assert res["classes"] is None
        return
    if "pairs" in case:
        assert [p[:2] for p in res["pairs"]] == case["pairs"]
    for pair, n in case.get("n_obs", {}).items():
        assert {p[:2]: p[3] for p in res["pairs"]}[pair] == n
    for pair, a in case.get("ari", {}).items():
        assert {p[:2]: p[2] for p in res["pairs"]}[pair] == a
    if "classes" in case:
        assert {c["id"]: k for c, k in zip(case["ds"]["chunks"], res["classes"])} == case["classes"]
    assert [p[:2] for p in res["pairs"]] == sorted(p[:2] for p in res["pairs"])


def test_cases_cover_the_branches_they_name():
    ari = {name: {p[:2]: p[2] for p in reference(name)["pairs"]} for name in K.NAMES if reference(name)["status"] == 0}
    assert ari["both_constant"][(13, 14)] == 1.0 and ari["one_constant"][(15, 16)] == 0.0
    assert ari["perfect_match"][(17, 18)] == 1.0 and ari["anti_correlated"][(19, 20)] == -0.1
    assert ari["chunk_twice_in_read"] == {(5, 5): 1.0, (5, 6): 1.0}            # the minimum cluster, not the first node's
    assert reference("chunk_twice_in_read")["counts"] == {(5, 5): 11, (5, 6): 22}
    assert reference("count_threshold")["counts"] == {(3, 4): 11}
    assert ari["unbiased_nodes_not_in_table"][(9, 10)] == 1.0
    st = reference("graph_fractional_scores")["stats"]
    assert st["no_draw"] > 0 and st["rejected"] > 0 and st["draws"] > 10000     # both branches of gen_bool
    assert len(ari["one_read_of_300_nodes"]) == 190 and len(ari["beyond_every_grid"]) == 1225
    grid = K.CASES["beyond_every_grid"]["ds"]
    assert len(grid["reads"]) > 1024 and sum(len(r["nodes"]) * (len(r["nodes"]) + 1) // 2 for r in grid["reads"]) > 1024 * 64
    sus = [name for name in ari if R.SUSPICIOUS in reference(name)["classes"]]
    assert "suspicious_smaller_isolated_larger" in sus and len(sus) >= 3


@pytest.mark.parametrize("name", K.NAMES)
def test_libm_and_project_math_agree(name):
    """a case on which they differed would sit on an ulp edge of exp: its inputs would have to move"""
    a, b = reference(name, "libm"), reference(name, "project")
    for key in ("status", "pairs", "classes", "cluster_num", "cluster", "touched"):
        assert a[key] == b[key], key


# ---- jtk_lc_squish_classify (host only)

@pytest.mark.parametrize("name", K.NAMES)
def test_classify_entry_point_follows_the_given_order(jtk_lib, name):
    res = reference(name)
    if res["status"] != 0 or not res["pairs"]:
        return   # no pair list to classify
    cfg = dict(R.DEFAULT_CONFIG, **K.CASES[name].get("cfg", {}))
    shuffled = list(res["pairs"])
    random.Random(1).shuffle(shuffled)
    for pairs in (res["pairs"], shuffled, [(b, a, x, n) for a, b, x, n in shuffled]):
        ids, stiff = api.squish_classify([p[0] for p in pairs], [p[1] for p in pairs], [p[2] for p in pairs], [p[3] for p in pairs],
                                         config=config_of(name))
        want_ids, want = R.classify(pairs, cfg, CR.ProjectMath().exp)
        assert ids.tolist() == want_ids and stiff.tolist() == [int(x) for x in want]


def test_classify_entry_point_edges(jtk_lib):
    ids, stiff = api.squish_classify([], [], [], [])
    assert len(ids) == 0 and len(stiff) == 0
    # NaN and out-of-range indices are clamped like .max(0).min(1); (u, u) is a node with two self-edges
    pairs = [(4, 4, float("nan"), 12), (4, 9, 7.5, 11), (2, 9, -3.0, 30)]
    want_ids, want = R.classify([(a, b, 0.0 if x != x else x, n) for a, b, x, n in pairs], R.DEFAULT_CONFIG, CR.ProjectMath().exp)
    ids, stiff = api.squish_classify(*zip(*pairs))
    assert ids.tolist() == want_ids == [4, 9, 2] and stiff.tolist() == [int(x) for x in want]
    L = ffi.lib()
    n_ids = C.c_size_t(0)
    u = np.array([1, 2], dtype=np.uint64)
    one = np.ones(2, dtype=np.uint64)
    cfg = ffi.SquishConfig()
    rc = L.jtk_lc_squish_classify(2, ffi.u64p(u), ffi.u64p(u + 5), ffi.f64p(np.ones(2)), ffi.u64p(one), C.byref(cfg), ffi.u64p(one.copy()),
                                  ffi.u8p(np.zeros(2, np.uint8)), 2, C.byref(n_ids))
    assert rc == -1 and n_ids.value == 4          # id_cap too small: the count comes back
    assert L.jtk_lc_squish_classify(0, None, None, None, None, None, None, None, 0, C.byref(n_ids)) == -1


# ---- declarations

def test_symbols_are_declared_exported_and_bound():
    for name, n_args in (("jtk_lc_squish_clusters", 17), ("jtk_lc_squish_classify", 10)):
        assert name in ffi.EXPORTED_SYMBOLS
        f = getattr(ffi.lib(), name)
        assert f.restype is C.c_int and len(f.argtypes) == n_args
    header = open(os.path.join(ROOT, "include", "jtk_lc.h")).read()
    for needle in ("jtk_lc_squish_clusters(", "jtk_lc_squish_classify(", "JTK_REL_STIFF = 0, JTK_REL_ISOLATED = 1, JTK_REL_SUSPICIOUS = 2",
                   "typedef struct jtk_squish_config", "ascending by (u1, u2)"):
        assert needle in header, needle
    rust = open(os.path.join(ROOT, "rust", "gpu_ffi.rs")).read()
    assert "pub fn jtk_lc_squish_clusters(" in rust and "pub fn jtk_lc_squish_classify(" in rust and "pub struct JtkSquishConfig" in rust
    assert C.sizeof(ffi.SquishConfig) == 32 and ffi.lib().jtk_lc_version() == 2
    cfg = ffi.SquishConfig()
    assert (cfg.ari_thr, cfg.match_score, cfg.mismatch_score, cfg.count_thr) == (0.5, 4.0, -1.0, 10)
    assert (ffi.REL_STIFF, ffi.REL_ISOLATED, ffi.REL_SUSPICIOUS) == (R.STIFF, R.ISOLATED, R.SUSPICIOUS)


def test_entry_point_rejects_bad_arguments_and_has_no_cpu_path(jtk_lib):
    prob = __import__("correction_reference").flatten(K.CASES["perfect_match"]["ds"])
    L = ffi.lib()
    if L.jtk_lc_device_ok(0) != 1:         # no device: an error, never a host computation
        with pytest.raises(ffi.JtkError) as e:
            api.squish_clusters(prob["node_off"], prob["nodes"], prob["posteriors"], prob["chunks"].copy())
        assert e.value.status == -2
    assert L.jtk_lc_squish_clusters(0, None, None, None, 0, None, None, None, None, None, None, None, None, None, 0, None, 0) == -1


# ---- the dataset.py stages, the device call stubbed by the reference

def dataset_json(ds):
    """a DataSet JSON (every field of the wire format) around a case: every node is ACGT (its own reverse complement), edges that recover the raw read"""
    reads, raw = [], []
    for read in ds["reads"]:
        nodes = [dict(position_from_start=4 * i, chunk=n["chunk"], cluster=n["cluster"], seq="ACGT", is_forward=bool(n["is_forward"]), cigar="4M",
                      posterior=list(n["posterior"])) for i, n in enumerate(read["nodes"])]
        edges = [{"from": a["chunk"], "to": b["chunk"], "offset": 0, "label": ""} for a, b in zip(nodes, nodes[1:])]
        reads.append(dict(id=read["id"], original_length=4 * len(nodes), leading_gap="", trailing_gap="", edges=edges, nodes=nodes))
        raw.append(dict(name="r%d" % read["id"], desc="", id=read["id"], seq="ACGT" * len(nodes)))
    hmm = {k: float(getattr(ffi.default_hmm(), k)) for k in D.SCHEMA["HMMParam"][:9]}
    hmm.update(mat_emit=list(ffi.default_hmm().mat_emit), ins_emit=list(ffi.default_hmm().ins_emit))
    return dict(input_file="x.fa", masked_kmers=dict(k=12, thr=10), coverage={"Protected": float(ds.get("coverage", 10.0))}, raw_reads=raw,
                hic_pairs=[], selected_chunks=[dict(id=c["id"], seq="ACGT", cluster_num=c["cluster_num"], copy_num=c["copy_num"],
                                                    score=c["score"]) for c in ds["chunks"]],
                encoded_reads=reads, hic_edges=[], read_type="CCS", model_param=dict(forward=hmm, reverse=copy.deepcopy(hmm)),
                error_rate={k: 0.01 for k in D.SCHEMA["ErrorRate"]}, processed_stages=[dict(stage_name="local_clustering", arg=[])])


def stub_squish(monkeypatch, calls):
    def fake(node_off, nodes, posteriors, chunks, config=None, device=0):
        import correction_reference as CRF
        ds = CRF.unflatten(dict(read_id=np.arange(len(node_off) - 1), node_off=node_off, nodes=nodes, posteriors=posteriors,
                                chunks=chunks), 10.0)
        cfg = config or ffi.SquishConfig()
        res = R.squish(ds, dict(ari_thr=cfg.ari_thr, match_score=cfg.match_score, mismatch_score=cfg.mismatch_score,
                                count_thr=cfg.count_thr), exp=CR.ProjectMath().exp)
        assert res["status"] == 0
        chunks["cluster_num"] = res["cluster_num"]
        calls.append("squish")
        return dict(classes=np.array(res["classes"], np.uint8), cluster=np.array(res["cluster"], np.uint64),
                    touched=np.array(res["touched"], np.uint8))
    monkeypatch.setattr(api, "squish_clusters", fake)


def test_dataset_stages(monkeypatch, tmp_path):
    name = "suspicious_smaller_isolated_larger"
    ds = K.CASES[name]["ds"]
    want = R.written_back(ds, reference(name))
    calls = []
    stub_squish(monkeypatch, calls)
    monkeypatch.setattr(api, "trim_cache", lambda device=0: None)
    src, dst = tmp_path / "in.json", tmp_path / "out.json"
    before = dataset_json(ds)
    src.write_text(json.dumps(before))
    assert D.main(["--stage", "squish_erroneous_clusters", str(src), str(dst)]) == 0
    after = json.loads(dst.read_text())
    assert [c["cluster_num"] for c in after["selected_chunks"]] == [c["cluster_num"] for c in want["chunks"]]
    changed = 0
    for ra, rb, rw in zip(after["encoded_reads"], before["encoded_reads"], want["reads"]):
        for na, nb, nw in zip(ra["nodes"], rb["nodes"], rw["nodes"]):
            assert (na["cluster"], na["posterior"]) == (nw["cluster"], nw["posterior"])
            changed += (na["cluster"], na["posterior"]) != (nb["cluster"], nb["posterior"])
            assert {k: v for k, v in na.items() if k not in ("cluster", "posterior")} == {k: v for k, v in nb.items() if k not in ("cluster", "posterior")}
    assert changed > 0 and [n["posterior"] for r in after["encoded_reads"] for n in r["nodes"] if n["chunk"] == 29][0] == [0.0]
    for key in before:
        if key not in ("selected_chunks", "encoded_reads"):
            assert after[key] == before[key]
    # --stage corrected: squish, then correct_clustering on its output (cli/src/pipeline.rs:174-175)
    seen = []

    def fake_correct(ds_, device=0, min_gain=None):
        seen.append(copy.deepcopy(ds_))
        calls.append("correct")
    monkeypatch.setattr(D, "correct_clustering", fake_correct)
    assert D.main(["--stage", "corrected", str(src), str(dst)]) == 0
    assert calls == ["squish", "squish", "correct"] and seen[0] == after
    # --stage correct_clustering stays as it is: no squish
    assert D.main(["--stage", "correct_clustering", str(src), str(dst)]) == 0 and calls[3:] == ["correct"] and seen[1] == before
