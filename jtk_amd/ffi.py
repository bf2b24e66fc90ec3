"""ctypes binding of libjtk_lc.so (the C-ABI of include/jtk_lc.h) and of libjtk_synth.so (include/jtk_synth.h: the
synthetic pile-up generator of bench.py and the tests, deliberately a separate library).

There is no Python or CPU fallback: if the shared library is missing this module raises, and a compute
call on a machine without a gfx950 device returns JTK_ERR_NO_DEVICE which is raised as JtkError.
"""
import ctypes as C
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG_DIR)
# JTK_LC_LIB: an experiment build of the library (scripts/*probe*.sh); the product never sets it
LIB_PATH = os.environ.get("JTK_LC_LIB") or os.path.join(PKG_DIR, "_build", "libjtk_lc.so")
SYNTH_LIB_PATH = os.path.join(PKG_DIR, "_build", "libjtk_synth.so")

NUM_ROW = 14
OP_MATCH, OP_MISMATCH, OP_INS, OP_DEL = 0, 1, 2, 3   # enum jtk_op (jtk_lc.h) == kiley::Op
GAINS_MAX_HOMOP = 8
K_COUNT = 4
KERNEL_NAMES = ("phmm", "polish", "filter", "mcmc")


class JtkError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"jtk_lc status {status}: {msg}")
        self.status = status


class Hmm(C.Structure):
    """jtk_hmm_t == definitions::HMMParam (definitions/src/lib.rs:101-126)."""
    _fields_ = [(n, C.c_double) for n in ("mat_mat", "mat_ins", "mat_del", "ins_mat", "ins_ins", "ins_del",
                                           "del_mat", "del_ins", "del_del")] + [
        ("mat_emit", C.c_double * 16), ("ins_emit", C.c_double * 20)]


class GainProfile(C.Structure):
    _fields_ = [("gain", C.c_double), ("prob", C.c_double)]


class Gains(C.Structure):
    _fields_ = [("max_homopolymer_len", C.c_uint32), ("reserved", C.c_uint32),
                ("subst", GainProfile * GAINS_MAX_HOMOP), ("deletions", GainProfile * GAINS_MAX_HOMOP),
                ("insertions", GainProfile * GAINS_MAX_HOMOP)]


class Params(C.Structure):
    _fields_ = [("forward", Hmm), ("reverse", Hmm), ("gains", Gains), ("haploid_coverage", C.c_double),
                ("band_frac", C.c_double)]


class SynthCfg(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("tmpl_len", C.c_uint32), ("n_haps", C.c_uint32),
                ("reads_per_hap", C.c_uint32), ("min_variants", C.c_uint32), ("divergence", C.c_double),
                ("err_sub", C.c_double), ("err_ins", C.c_double), ("err_del", C.c_double),
                ("tmpl_err", C.c_double)]


class Timing(C.Structure):
    _fields_ = [("total_ms", C.c_double), ("h2d_ms", C.c_double), ("d2h_ms", C.c_double),
                ("kernel_ms", C.c_double * K_COUNT), ("kernel_launches", C.c_uint32 * K_COUNT),
                ("chain_lds_bytes", C.c_uint32 * 2)]


DEBUG_LANE_RECORDS = 8   # JTK_LC_DEBUG_LANE_RECORDS


class LaneLaunch(C.Structure):
    """jtk_lc_debug_lane_launch_t: one call of a lane's chain launch"""
    _fields_ = [("members", C.c_uint32), ("segments", C.c_uint32 * 2), ("chunks", C.c_uint32 * 2),
                ("seg_chunks", (C.c_uint32 * 8) * 2)]


class LaneState(C.Structure):
    """jtk_lc_debug_lane_state_t"""
    _fields_ = [("in_pass", C.c_uint32), ("holds", C.c_uint32), ("pending", C.c_uint32), ("n_records", C.c_uint32),
                ("launch_calls", C.c_uint64), ("records", LaneLaunch * DEBUG_LANE_RECORDS)]


DEBUG_ROUND_RECORDS = 64          # JTK_LC_DEBUG_ROUND_RECORDS
DEBUG_ROUND_OPEN = 0xffffffff     # JTK_LC_DEBUG_ROUND_OPEN


class RoundLaunch(C.Structure):
    """jtk_lc_debug_round_launch_t: one call of a lane's round launch"""
    _fields_ = [("members", C.c_uint32), ("merged", C.c_uint32), ("round", C.c_uint32 * 8), ("chunks", C.c_uint32 * 8),
                ("phmm_items", C.c_uint32 * 8)]


class RoundState(C.Structure):
    """jtk_lc_debug_round_state_t"""
    _fields_ = [("in_rounds", C.c_uint32), ("holds", C.c_uint32), ("parked", C.c_uint32), ("n_records", C.c_uint32),
                ("launch_calls", C.c_uint64), ("records", RoundLaunch * DEBUG_ROUND_RECORDS)]


DEBUG_PASS_RECORDS = 4   # JTK_LC_DEBUG_PASS_RECORDS
LEFT_BY_WORD, LEFT_BY_EVENT = 1, 2   # JTK_LC_DEBUG_LEFT_BY_*


class PassRecord(C.Structure):
    """jtk_lc_debug_pass_t: how one pass of a session ended"""
    _fields_ = [("pass_", C.c_uint64), ("how", C.c_uint32), ("event_pending", C.c_uint32), ("members", C.c_uint32),
                ("still_waiting", C.c_uint32), ("round_stream", C.c_uint32), ("next_round_stream", C.c_uint32),
                ("stamp_left", C.c_uint64), ("stamp_returned", C.c_uint64), ("stamp_fetched", C.c_uint64),
                ("stamp_round0", C.c_uint64)]


class SquishConfig(C.Structure):
    """jtk_squish_config_t; the defaults are SquishConfig::default() (squish_erroneous_clusters.rs:29-38)."""
    _fields_ = [("ari_thr", C.c_double), ("match_score", C.c_double), ("mismatch_score", C.c_double), ("count_thr", C.c_uint64)]

    def __init__(self, ari_thr=0.5, match_score=4.0, mismatch_score=-1.0, count_thr=10):
        super().__init__(ari_thr, match_score, mismatch_score, count_thr)


REL_STIFF, REL_ISOLATED, REL_SUSPICIOUS = 0, 1, 2   # enum jtk_rel_class

CHUNK_DT = np.dtype([("chunk_id", "<u8"), ("copy_num", "<u4"), ("n_reads", "<u4"), ("tmpl_off", "<u8"),
                     ("tmpl_len", "<u8"), ("read_first", "<u8")])
RESULT_DT = np.dtype([("score", "<f8"), ("cluster_num", "<u4"), ("status", "<i4"), ("polish_rounds", "<u4"),
                      ("n_variants", "<u4")])
FEATURE_CHUNK_DT = np.dtype([("chunk_id", "<u8"), ("copy_num", "<u4"), ("n_reads", "<u4"), ("dim", "<u4"),
                             ("reserved", "<u4"), ("var_off", "<u8"), ("vt_off", "<u8"), ("read_first", "<u8"),
                             ("local_coverage", "<f8")])

CC_NODE_DT = np.dtype([("chunk", "<u8"), ("cluster", "<u8"), ("is_forward", "<u4"), ("post_len", "<u4"), ("post_off", "<u8")])
CC_CHUNK_DT = np.dtype([("id", "<u8"), ("cluster_num", "<u4"), ("copy_num", "<u4"), ("score", "<f8")])
# jtk_fill_node_t / jtk_fill_cand_t (jtk_lc_fill_candidates)
FILL_NODE_DT = np.dtype([("chunk", "<u8"), ("cluster", "<u8"), ("is_forward", "<u4"), ("query_len", "<u4"), ("position", "<u8")])
FILL_CAND_DT = np.dtype([("read", "<u4"), ("slot", "<u4"), ("side", "<u4"), ("is_forward", "<u4"), ("chunk", "<u8"), ("cluster", "<u8"),
                         ("count", "<u4"), ("reserved", "<u4"), ("position", "<i8")])
FILL_MATCH, FILL_INS, FILL_DEL = 0, 1, 2   # op codes of jtk_lc_debug_fill_pairs
# jtk_guided_pair_t (jtk_lc_align_guided); jtk_encode_trial_t / jtk_encode_result_t (jtk_lc_encode_nodes)
GUIDED_PAIR_DT = np.dtype([("x_off", "<u8"), ("y_off", "<u8"), ("guide_off", "<u8"), ("x_len", "<u4"), ("y_len", "<u4"), ("guide_len", "<u4"),
                           ("radius", "<u4")])
ENCODE_TRIAL_DT = np.dtype([("read_off", "<u8"), ("start", "<u4"), ("end", "<u4"), ("is_forward", "<u4"), ("cons_len", "<u4"), ("cons_off", "<u8"),
                            ("chunk_off", "<u8"), ("chunk_len", "<u4"), ("reserved", "<u4"), ("sim_thr", "<f8")])
ENCODE_RESULT_DT = np.dtype([("status", "<i4"), ("verdict", "<u4"), ("trim_head", "<u4"), ("trim_tail", "<u4"), ("position_from_start", "<u8"),
                             ("query_len", "<u4"), ("band", "<u4"), ("score", "<i4"), ("mat_num", "<u4"), ("ops_len", "<u4"), ("head_match", "<u4"),
                             ("head_len", "<u4"), ("tail_match", "<u4"), ("tail_len", "<u4"), ("reserved", "<u4")])
# jtk_edge_trial_t / jtk_edge_result_t / jtk_edge_node_t (jtk_lc_encode_edges)
EDGE_TRIAL_DT = np.dtype([("read_off", "<u8"), ("start", "<u4"), ("end", "<u4"), ("is_forward", "<u4"), ("radius", "<u4"), ("contig_off", "<u8"),
                          ("contig_len", "<u4"), ("n_chunks", "<u4"), ("break_first", "<u8"), ("sim_thr", "<f8")])
EDGE_RESULT_DT = np.dtype([("status", "<i4"), ("score", "<i4"), ("seq_start", "<u4"), ("seq_end", "<u4"), ("ctg_start", "<u4"), ("ctg_end", "<u4"),
                           ("first_chunk", "<u4"), ("head_ins", "<u4")])
EDGE_NODE_DT = np.dtype([("verdict", "<u4"), ("mat_num", "<u4"), ("ops_len", "<u4"), ("query_off", "<u4"), ("query_len", "<u4"), ("reserved", "<u4"),
                         ("position_from_start", "<u8")])
EDGE_ACCEPTED, EDGE_REJECTED, EDGE_NOT_REACHED = 0, 2, 3   # enum jtk_edge_verdict
GUIDED_MAX_WIDTH = 4096    # JTK_GUIDED_MAX_WIDTH
ENCODE_ACCEPTED, ENCODE_LOWER_BOUND, ENCODE_REJECTED = 0, 1, 2   # enum jtk_encode_verdict
# jtk_settle_node_t / jtk_node_stats_t (jtk_lc_settle_nodes); the C struct pads del_size to offset 16
SETTLE_NODE_DT = np.dtype([("chunk", "<u8"), ("position_from_start", "<u8"), ("is_forward", "<u4"), ("query_len", "<u4")])
NODE_STATS_DT = np.dtype({"names": ["score", "total", "indel", "del_size"], "formats": ["<i4", "<u4", "<u4", "<i8"],
                          "offsets": [0, 4, 8, 16], "itemsize": 24})
SETTLE_STATS_ONLY, SETTLE_BY_CHUNK_POS, SETTLE_BY_CHUNK = 0, 1, 2   # enum jtk_settle_mode
SETTLE_DROPPED = 0xffffffff   # order[] behind a read's survivors
# jtk_mask_report_t (jtk_lc_mask_repeats)
MASK_REPORT_DT = np.dtype([("n_bases", "<u8"), ("n_kmers", "<u8"), ("n_distinct", "<u8"), ("n_singleton", "<u8"), ("n_masked_kmers", "<u8"),
                           ("n_lower", "<u8"), ("thr", "<u4"), ("takes_all", "<u4")])
MASK_MAX_K = 31
# jtk_map_params_t / jtk_map_placement_t (jtk_lc_map_reads)
MAP_PARAMS_DT = np.dtype([(n, "<u4") for n in ("k", "w", "max_occ", "max_gap", "min_seeds", "skip_self")])
MAP_PLACEMENT_DT = np.dtype([(n, "<u4") for n in ("query", "target", "is_forward", "n_seeds", "qstart", "qend", "oq_start", "oq_end", "tstart", "tend")]
                            + [("diag_lo", "<i4"), ("diag_hi", "<i4")])
MAP_MAX_K, MAP_MAX_W, MAP_MAX_TARGET_LEN, MAP_MAX_QUERY_LEN, MAP_MAX_TARGETS = 31, 64, 65535, 4000000, 1 << 25

# every symbol declared in include/jtk_lc.h (tests check the library exports them)
EXPORTED_SYMBOLS = (
    "jtk_lc_cluster_chunks", "jtk_lc_cluster_chunks_multi", "jtk_lc_cluster_polished", "jtk_lc_polish_chunks", "jtk_lc_align_reads", "jtk_lc_align_reads_mode", "jtk_lc_modification_table",
    "jtk_lc_cluster_features", "jtk_lc_estimate_gains", "jtk_lc_estimate_minimum_gain", "jtk_lc_fit_model", "jtk_lc_correct_clustering", "jtk_lc_squish_clusters", "jtk_lc_squish_classify", "jtk_lc_node_errors", "jtk_lc_error_quantile", "jtk_lc_estimate_error_rate", "jtk_lc_purge_diverged", "jtk_lc_settle_nodes", "jtk_lc_mask_repeats", "jtk_lc_repetitive_kmers", "jtk_lc_repetitiveness", "jtk_lc_map_reads", "jtk_lc_sketch", "jtk_lc_fill_candidates", "jtk_lc_align_guided", "jtk_lc_polish_guided", "jtk_lc_encode_nodes", "jtk_lc_encode_edges", "jtk_lc_trim_cache", "jtk_lc_pileup_sort_key", "jtk_lc_normalize_pileup", "jtk_lc_strerror",
    "jtk_lc_last_error", "jtk_lc_version", "jtk_lc_device_ok", "jtk_lc_last_timing",
    "jtk_lc_session_create", "jtk_lc_session_run", "jtk_lc_session_fetch", "jtk_lc_session_destroy", "jtk_lc_session_trace",
)
# every symbol declared in include/jtk_lc_debug.h: diagnostic entry points, not part of the drop-in boundary
DEBUG_SYMBOLS = (
    "jtk_lc_debug_cc_keep_sims", "jtk_lc_debug_cc_first_sims", "jtk_lc_debug_cc_sims_count", "jtk_lc_debug_cc_sims",
    "jtk_lc_debug_chain_profile", "jtk_lc_debug_purge_timing", "jtk_lc_debug_fill_pairs", "jtk_lc_debug_fill_timing",
    "jtk_lc_debug_gains_keep", "jtk_lc_debug_gains_batches", "jtk_lc_debug_gains_batch_sizes", "jtk_lc_debug_gains_batch",
    "jtk_lc_debug_guided_scratch_cap", "jtk_lc_debug_guided_timing", "jtk_lc_debug_encode_timing",
    "jtk_lc_debug_guided_table", "jtk_lc_debug_gpolish_timing", "jtk_lc_debug_edges_timing",
    "jtk_lc_debug_session_lane", "jtk_lc_debug_lane_hold", "jtk_lc_debug_lane_state", "jtk_lc_debug_filter",
    "jtk_lc_debug_round_hold", "jtk_lc_debug_round_state", "jtk_lc_debug_session_passes", "jtk_lc_debug_settle_timing", "jtk_lc_debug_mask_timing", "jtk_lc_debug_map_timing",
)
DEBUG_FILTER_TABLE, DEBUG_FILTER_ROWS_FUSED, DEBUG_FILTER_ROWS_TABLE = 0, 1, 2   # modes of jtk_lc_debug_filter
DEBUG_FILTER_TRACE_WORDS = 66   # JTK_LC_DEBUG_FILTER_TRACE_WORDS
MAX_DIM = 21                    # JTK_MAX_DIM: the columns a chunk picks at most
DEBUG_GAINS_OPS_STRIDE = 512   # JTK_LC_DEBUG_GAINS_OPS_STRIDE
SYNTH_SYMBOLS = ("jtk_synth_pileup",)


def u8p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def f64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def u64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def u32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


_lib = None


def lib():
    """Load libjtk_lc.so; raise (never fall back) if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). jtk_amd has no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp, sz, u64, u32, i32 = C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint32, C.c_int
    PU8, PU64, PU32, PD = (C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
                           C.POINTER(C.c_double))
    PP = C.POINTER(Params)

    def sig(name, res, *args):
        f = getattr(L, name)
        f.restype = res
        f.argtypes = list(args)

    sig("jtk_lc_cluster_chunks", i32, PP, sz, vp, PU8, PU8, PU64, PU8, PU64, PU8, PU32, PD, u32, vp, PU8,
        PU64, u64, PU8, PU64, u64, i32)
    sig("jtk_lc_cluster_chunks_multi", i32, PP, sz, vp, PU8, PU8, PU64, PU8, PU64, PU8, PU32, PD, u32, vp, PU8,
        PU64, u64, PU8, PU64, u64, C.POINTER(C.c_int), sz)
    sig("jtk_lc_cluster_polished", i32, PP, sz, vp, PU8, PU8, PU64, PU8, PU64, PU8, PU32, PD, u32, vp, i32)
    sig("jtk_lc_polish_chunks", i32, PP, sz, vp, PU8, PU8, PU64, PU8, PU64, PU8, u32, u32, u32, PU8, PU64, u64, PU8, PU64,
        u64, vp, i32)
    sig("jtk_lc_align_reads", i32, sz, vp, PU8, PU8, PU64, u32, PU8, PU64, u64, PU32, C.POINTER(C.c_int32), i32)
    sig("jtk_lc_align_reads_mode", i32, sz, vp, PU8, PU8, PU64, i32, i32, u32, PU8, PU64, u64, PU32, PU32, PU32,
        C.POINTER(C.c_int32), i32)
    sig("jtk_lc_modification_table", i32, PP, PU8, u64, u32, PU8, PU64, PU8, PU64, PU8, PD, PD, i32)
    sig("jtk_lc_estimate_gains", i32, C.POINTER(Hmm), C.POINTER(Hmm), u64, u32, u32, u32, C.POINTER(Gains), i32)
    sig("jtk_lc_estimate_minimum_gain", i32, C.POINTER(Hmm), C.POINTER(Hmm), u64, u32, u32, u32, u32, PD, i32)
    sig("jtk_lc_fit_model", i32, PP, sz, vp, PU8, PU8, PU64, PU8, PU64, PU8, u32, C.POINTER(Hmm), C.POINTER(Hmm), i32)
    sig("jtk_lc_correct_clustering", i32, sz, PU64, PU64, vp, PD, sz, vp, sz, PU64, C.c_double, C.c_double, PU64, PU8, i32)
    PSQ, PSZ = C.POINTER(SquishConfig), C.POINTER(sz)
    sig("jtk_lc_squish_clusters", i32, sz, PU64, vp, PD, sz, vp, PSQ, PU8, PU64, PU8, PU64, PU64, PD, PU64, sz, PSZ, i32)
    sig("jtk_lc_squish_classify", i32, sz, PU64, PU64, PD, PU64, PSQ, PU64, PU8, sz, PSZ)
    PI32 = C.POINTER(C.c_int32)
    sig("jtk_lc_node_errors", i32, sz, PU64, vp, sz, vp, PU8, PU64, PU8, PU64, PU8, PU64, PU32, PU32, PI32, i32)
    sig("jtk_lc_error_quantile", i32, sz, PU32, PU32, C.c_double, PD, i32)
    sig("jtk_lc_estimate_error_rate", i32, sz, PU64, vp, PU32, PU32, sz, vp, C.c_double, PD, PD, PU64, sz, PD, PU32, i32)
    sig("jtk_lc_purge_diverged", i32, sz, PU64, vp, sz, sz, vp, PU8, PU64, PU8, PU64, PU8, PU64, C.c_double, PU8, PU64, sz, PU8, PU64,
        PU8, PU8, PU64, sz, PSZ, PD, PD, PD, i32)
    sig("jtk_lc_settle_nodes", i32, sz, PU64, vp, PU8, PU64, i32, vp, PU32, PU32, PU8, PI32, i32)
    sig("jtk_lc_debug_settle_timing", None, PD)
    if hasattr(L, "jtk_lc_mask_repeats"):   # (a JTK_LC_LIB build of an earlier revision has none: scripts/build_rev.py)
        sig("jtk_lc_mask_repeats", i32, sz, PU8, PU64, u32, C.c_double, u32, PU8, PU64, u64, vp, i32)
        sig("jtk_lc_repetitive_kmers", i32, sz, PU8, PU64, u32, PU64, u64, PU64, i32)
        sig("jtk_lc_repetitiveness", i32, sz, PU8, PU64, u32, PU64, u64, PU32, PU32, i32)
        sig("jtk_lc_debug_mask_timing", None, PD)
    if hasattr(L, "jtk_lc_map_reads"):      # (likewise)
        sig("jtk_lc_map_reads", i32, sz, PU8, PU64, sz, PU8, PU64, vp, vp, u64, PU64, i32)
        sig("jtk_lc_sketch", i32, sz, PU8, PU64, u32, u32, PU64, PU32, PU32, PU8, u64, PU64, i32)
        sig("jtk_lc_debug_map_timing", None, PD)
    sig("jtk_lc_fill_candidates", i32, sz, PU64, vp, PU8, PU32, PU32, PU64, vp, sz, PSZ, i32)
    sig("jtk_lc_debug_fill_pairs", i32, sz, PU64, vp, sz, PU32, PU32, PI32, PI32, PU8, PU64, PU32, sz, PSZ, i32)
    sig("jtk_lc_debug_fill_timing", None, PD)
    sig("jtk_lc_align_guided", i32, sz, vp, PU8, PU8, PU8, i32, i32, i32, i32, i32, PU8, PU64, u64, PI32, PU32, PU32, PI32, i32)
    sig("jtk_lc_encode_nodes", i32, sz, vp, PU8, PU8, PU8, vp, PU8, PU64, u64, i32)
    sig("jtk_lc_encode_edges", i32, sz, vp, PU8, PU8, PU32, PU64, vp, vp, PU8, PU64, u64, i32)
    sig("jtk_lc_debug_edges_timing", None, PD)
    sig("jtk_lc_debug_guided_scratch_cap", None, u64)
    sig("jtk_lc_debug_guided_timing", None, PD)
    sig("jtk_lc_debug_encode_timing", None, PD)
    sig("jtk_lc_polish_guided", i32, sz, vp, PU8, PU8, PU64, PU8, PU64, PU32, u32, u32, u32, PU8, PU64, u64, PU8, PU64, u64, PU32, vp, i32)
    sig("jtk_lc_debug_guided_table", i32, PU8, u32, u32, PU8, PU64, PU8, PU64, u32, PU32, PU32, u64, i32)
    sig("jtk_lc_debug_gpolish_timing", None, PD)
    sig("jtk_lc_trim_cache", i32, i32)
    sig("jtk_lc_cluster_features", i32, PP, sz, vp, PD, PU32, PU32, PD, u32, vp, i32)
    sig("jtk_lc_pileup_sort_key", i32, PU8, u64, PU8, u64, PU8, u64, PU64)
    sig("jtk_lc_normalize_pileup", i32, u32, u32, PU32, PD, u32)
    sig("jtk_lc_strerror", C.c_char_p, i32)
    sig("jtk_lc_last_error", C.c_char_p)
    sig("jtk_lc_version", i32)
    sig("jtk_lc_device_ok", i32, i32)
    sig("jtk_lc_last_timing", i32, C.POINTER(Timing))
    sig("jtk_lc_session_create", i32, PP, sz, vp, PU8, PU8, PU64, PU8, PU64, PU8, u32, i32,
        C.POINTER(vp))
    sig("jtk_lc_session_run", i32, vp, i32)
    sig("jtk_lc_session_fetch", i32, vp, PU32, PD, vp, PU8, PU64, u64, PU8, PU64, u64)
    sig("jtk_lc_session_destroy", i32, vp)
    sig("jtk_lc_session_trace", i32, vp, sz, C.c_char_p, sz, C.POINTER(sz))
    sig("jtk_lc_debug_gains_keep", None, i32)
    sig("jtk_lc_debug_gains_batches", sz)
    sig("jtk_lc_debug_gains_batch_sizes", i32, sz, PU64)
    sig("jtk_lc_debug_gains_batch", i32, sz, PU8, PU64, PU8, PU64, PU8, PU32, PD)
    sig("jtk_lc_debug_session_lane", i32, vp)
    sig("jtk_lc_debug_lane_hold", i32, i32, i32, i32)
    sig("jtk_lc_debug_lane_state", i32, i32, i32, C.POINTER(LaneState))
    if hasattr(L, "jtk_lc_debug_round_hold"):   # (a JTK_LC_LIB build of an earlier revision has none: scripts/build_rev.py)
        sig("jtk_lc_debug_round_hold", i32, i32, i32, i32)
        sig("jtk_lc_debug_round_state", i32, i32, i32, C.POINTER(RoundState))
    if hasattr(L, "jtk_lc_debug_session_passes"):
        sig("jtk_lc_debug_session_passes", i32, vp, C.POINTER(PassRecord), sz)
    sig("jtk_lc_debug_filter", i32, PP, sz, vp, PU8, PU8, i32, PD, PI32, PD, PD, PU32, PU32, PU32, PD, PU32, i32)
    _lib = L
    return L


_synth = None


def synth_lib():
    """libjtk_synth.so: synthetic inputs for bench.py and the tests (not part of the product library)."""
    global _synth
    if _synth is None:
        if not os.path.exists(SYNTH_LIB_PATH):
            raise ImportError(f"{SYNTH_LIB_PATH} is missing: run __graft_entry__.build()")
        L = C.CDLL(SYNTH_LIB_PATH)
        PU8, PU64, PU32 = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
        L.jtk_synth_pileup.restype = C.c_int
        L.jtk_synth_pileup.argtypes = [C.POINTER(SynthCfg), PU8, C.c_uint64, PU64, PU8, C.c_uint64, PU64, PU8,
                                       C.c_uint64, PU64, PU8, PU32]
        _synth = L
    return _synth


def check(status):
    if status != 0:
        L = lib()
        msg = L.jtk_lc_strerror(status).decode()
        extra = L.jtk_lc_last_error().decode()
        raise JtkError(status, msg + (": " + extra if extra else ""))


def default_hmm():
    """HMMParam::default() (definitions/src/lib.rs:128-147)."""
    h = Hmm()
    for n in ("mat_mat", "ins_mat", "del_mat"):
        setattr(h, n, 0.97)
    for n in ("mat_ins", "mat_del", "ins_ins", "ins_del", "del_ins", "del_del"):
        setattr(h, n, 0.01)
    for r in range(4):
        for q in range(4):
            h.mat_emit[4 * r + q] = 0.97 if r == q else 0.01
    for i in range(20):
        h.ins_emit[i] = 0.25
    return h
