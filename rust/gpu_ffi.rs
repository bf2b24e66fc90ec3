// haplotyper/src/local_clustering/gpu_ffi.rs -- field-for-field #[repr(C)] mirrors of include/jtk_lc.h + the extern block
// NOT compiled in this repository: the build image has no Rust toolchain (cargo, rustc: command not found) and the
// reference's git dependencies are un-vendored.  Source a jtk maintainer adds to ban-m/jtk; INTEGRATION.md explains it and
// tests/test_rust_shim_source.py keeps it in step with include/jtk_lc.h.  The same call sequence is exercised end to end
// by the C++ host mirror (jtk_amd/csrc/host/local_clustering.hpp) and the Python harness (jtk_amd/api.py).
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)] #[derive(Clone, Copy)]
pub struct JtkHmm {                       // == definitions::HMMParam (definitions/src/lib.rs:101-126)
    pub mat_mat: f64, pub mat_ins: f64, pub mat_del: f64,
    pub ins_mat: f64, pub ins_ins: f64, pub ins_del: f64,
    pub del_mat: f64, pub del_ins: f64, pub del_del: f64,
    pub mat_emit: [f64; 16], pub ins_emit: [f64; 20],
}
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct JtkGainProfile { pub gain: f64, pub prob: f64 }     // likelihood_gains.rs:41-47
#[repr(C)] #[derive(Clone, Copy)]
pub struct JtkGains {                                           // likelihood_gains.rs:55-61
    pub max_homopolymer_len: u32, pub reserved: u32,
    pub subst: [JtkGainProfile; 8], pub deletions: [JtkGainProfile; 8], pub insertions: [JtkGainProfile; 8],
}
#[repr(C)] #[derive(Clone, Copy)]
pub struct JtkLcParams {
    pub forward: JtkHmm, pub reverse: JtkHmm, pub gains: JtkGains,
    pub haploid_coverage: f64, pub band_frac: f64,
}
#[repr(C)] #[derive(Clone, Copy)]
pub struct JtkLcChunk {
    pub chunk_id: u64, pub copy_num: u32, pub n_reads: u32,
    pub tmpl_off: u64, pub tmpl_len: u64, pub read_first: u64,
}
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct JtkLcResult {
    pub score: f64, pub cluster_num: u32, pub status: i32, pub polish_rounds: u32, pub n_variants: u32,
}

// the flattened DataSet view of jtk_lc_correct_clustering (phmm_likelihood_correction.rs:32-97)
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct JtkCcNode {
    pub chunk: u64, pub cluster: u64, pub is_forward: u32, pub post_len: u32, pub post_off: u64,
}
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct JtkCcChunk {
    pub id: u64, pub cluster_num: u32, pub copy_num: u32, pub score: f64,
}
// SquishConfig (squish_erroneous_clusters.rs:6-11; default 0.5, 4, -1, 10)
#[repr(C)] #[derive(Clone, Copy)]
pub struct JtkSquishConfig {
    pub ari_thr: f64, pub match_score: f64, pub mismatch_score: f64, pub count_thr: u64,
}
// what ReadSkelton::from_rich_nodes reads of a Node (encode/deletion_fill.rs:1003-1030), and one candidate of
// check_insertion_head (side 0) / check_insertion_tail (side 1) (:940-981)
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct JtkFillNode {
    pub chunk: u64, pub cluster: u64, pub is_forward: u32, pub query_len: u32, pub position: u64,
}
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct JtkFillCand {
    pub read: u32, pub slot: u32, pub side: u32, pub is_forward: u32, pub chunk: u64, pub cluster: u64,
    pub count: u32, pub reserved: u32, pub position: i64,
}
// what the settle step reads of a Node (encode/deletion_fill.rs:349-361, encode/mod.rs:248-313), and the numbers it and
// purge_large_deletion_nodes (purge_diverged.rs:75-80) take from a node's cigar
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct JtkSettleNode {
    pub chunk: u64, pub position_from_start: u64, pub is_forward: u32, pub query_len: u32,
}
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct JtkNodeStats {
    pub score: i32, pub total: u32, pub indel: u32, pub del_size: i64,
}
// the numbers of mask_repeat's MASKREPEAT debug rows (repeat_masking.rs:144-157, :262), thr and the TakesAll branch of create_mask
#[repr(C)] #[derive(Clone, Copy, Default, Debug)]
pub struct JtkMaskReport {
    pub n_bases: u64, pub n_kmers: u64, pub n_distinct: u64, pub n_singleton: u64, pub n_masked_kmers: u64, pub n_lower: u64,
    pub thr: u32, pub takes_all: u32,
}
// the mapper's parameters (minimap2's -k, -w, -f as a count, the chaining gap, -n, -X) and one seed cluster of a read on a chunk
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct JtkMapParams {
    pub k: u32, pub w: u32, pub max_occ: u32, pub max_gap: u32, pub min_seeds: u32, pub skip_self: u32,
}
#[repr(C)] #[derive(Clone, Copy, Default, Debug)]
pub struct JtkMapPlacement {
    pub query: u32, pub target: u32, pub is_forward: u32, pub n_seeds: u32,
    pub qstart: u32, pub qend: u32,
    pub oq_start: u32, pub oq_end: u32,
    pub tstart: u32, pub tend: u32,
    pub diag_lo: i32, pub diag_hi: i32,
}
pub const JTK_SETTLE_STATS_ONLY: c_int = 0;
pub const JTK_SETTLE_BY_CHUNK_POS: c_int = 1;
pub const JTK_SETTLE_BY_CHUNK: c_int = 2;
// one pair of jtk_lc_align_guided: offsets into two base buffers and one op buffer, so that pairs can share a sequence
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct JtkGuidedPair {
    pub x_off: u64, pub y_off: u64, pub guide_off: u64, pub x_len: u32, pub y_len: u32, pub guide_len: u32, pub radius: u32,
}
// one call of encode_node (encode/deletion_fill.rs:451-489) and what it returns
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct JtkEncodeTrial {
    pub read_off: u64, pub start: u32, pub end: u32, pub is_forward: u32, pub cons_len: u32, pub cons_off: u64,
    pub chunk_off: u64, pub chunk_len: u32, pub reserved: u32, pub sim_thr: f64,
}
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct JtkEncodeResult {
    pub status: i32, pub verdict: u32, pub trim_head: u32, pub trim_tail: u32, pub position_from_start: u64,
    pub query_len: u32, pub band: u32, pub score: i32, pub mat_num: u32, pub ops_len: u32, pub head_match: u32,
    pub head_len: u32, pub tail_match: u32, pub tail_len: u32, pub reserved: u32,
}
// one call of encode_edge (dense_encoding.rs:627-697), what tune_position found for it, and one record per chunk of its contig
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct JtkEdgeTrial {
    pub read_off: u64, pub start: u32, pub end: u32, pub is_forward: u32, pub radius: u32, pub contig_off: u64,
    pub contig_len: u32, pub n_chunks: u32, pub break_first: u64, pub sim_thr: f64,
}
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct JtkEdgeResult {
    pub status: i32, pub score: i32, pub seq_start: u32, pub seq_end: u32, pub ctg_start: u32, pub ctg_end: u32,
    pub first_chunk: u32, pub head_ins: u32,
}
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct JtkEdgeNode {
    pub verdict: u32, pub mat_num: u32, pub ops_len: u32, pub query_off: u32, pub query_len: u32, pub reserved: u32,
    pub position_from_start: u64,
}

extern "C" {
    pub fn jtk_lc_cluster_chunks(
        params: *const JtkLcParams, n_chunks: usize, chunks: *const JtkLcChunk,
        tmpl_bases: *const u8, read_bases: *const u8, read_off: *const u64,
        ops: *const u8, ops_off: *const u64, strand: *const u8,
        label: *mut u32, log_post: *mut f64, post_stride: u32, result: *mut JtkLcResult,
        cons_out: *mut u8, cons_off: *mut u64, cons_cap: u64,
        ops_out: *mut u8, ops_out_off: *mut u64, ops_cap: u64, device: c_int) -> c_int;
    // the same over several GPUs of one node (contiguous, read-balanced shares; no collective)
    pub fn jtk_lc_cluster_chunks_multi(
        params: *const JtkLcParams, n_chunks: usize, chunks: *const JtkLcChunk,
        tmpl_bases: *const u8, read_bases: *const u8, read_off: *const u64,
        ops: *const u8, ops_off: *const u64, strand: *const u8,
        label: *mut u32, log_post: *mut f64, post_stride: u32, result: *mut JtkLcResult,
        cons_out: *mut u8, cons_off: *mut u64, cons_cap: u64,
        ops_out: *mut u8, ops_out_off: *mut u64, ops_cap: u64, devices: *const c_int, n_devices: usize) -> c_int;
    pub fn jtk_lc_estimate_gains(forward: *const JtkHmm, reverse: *const JtkHmm, seed: u64, seq_len: u32, band: u32,
                                 homop_len: u32, out: *mut JtkGains, device: c_int) -> c_int;   // likelihood_gains.rs:162-192
    pub fn jtk_lc_estimate_minimum_gain(forward: *const JtkHmm, reverse: *const JtkHmm, seed: u64, sample_num: u32,
                                        seq_num: u32, len: u32, band: u32, out: *mut f64, device: c_int) -> c_int;  // likelihood_gains.rs:6-39
    // model_tune.rs:119-152 on the training pile-ups the host selected (model_tune.rs:99-118)
    pub fn jtk_lc_fit_model(
        params: *const JtkLcParams, n_chunks: usize, chunks: *const JtkLcChunk,
        tmpl_bases: *const u8, read_bases: *const u8, read_off: *const u64,
        ops: *const u8, ops_off: *const u64, strand: *const u8, rounds: u32,
        forward_out: *mut JtkHmm, reverse_out: *mut JtkHmm, device: c_int) -> c_int;
    // kiley polish_until_converge_antidiagonal on a batch of windows (consensus/mod.rs:476-483)
    pub fn jtk_lc_polish_chunks(
        params: *const JtkLcParams, n_chunks: usize, chunks: *const JtkLcChunk,
        tmpl_bases: *const u8, read_bases: *const u8, read_off: *const u64,
        ops: *const u8, ops_off: *const u64, strand: *const u8, radius: u32, take_num: u32, ignore_edge: u32,
        cons_out: *mut u8, cons_off: *mut u64, cons_cap: u64,
        ops_out: *mut u8, ops_out_off: *mut u64, ops_cap: u64, result: *mut JtkLcResult, device: c_int) -> c_int;
    // edlib Global / Alignment of every read to its chunk's template (consensus/mod.rs:424-435, polish_chunks.rs:114-120)
    pub fn jtk_lc_align_reads(
        n_chunks: usize, chunks: *const JtkLcChunk, tmpl_bases: *const u8, read_bases: *const u8, read_off: *const u64,
        max_dist: u32, ops_out: *mut u8, ops_out_off: *mut u64, ops_cap: u64,
        dist_out: *mut u32, read_status: *mut i32, device: c_int) -> c_int;
    // edlib Infix / Prefix / Alignment (mode 1 / 2; 0 = the call above), free_seq 0 = the template is edlib's target, 1 = the read:
    // encode/mod.rs:227-246, encode/deletion_fill.rs:544-554, dense_encoding.rs:728-757, determine_chunks.rs:520-538,
    // consensus/mod.rs:563-614; the ops consume [start_out[r], end_out[r]) of the free sequence
    pub fn jtk_lc_align_reads_mode(
        n_chunks: usize, chunks: *const JtkLcChunk, tmpl_bases: *const u8, read_bases: *const u8, read_off: *const u64,
        mode: c_int, free_seq: c_int, max_dist: u32, ops_out: *mut u8, ops_out_off: *mut u64, ops_cap: u64,
        dist_out: *mut u32, start_out: *mut u32, end_out: *mut u32, read_status: *mut i32, device: c_int) -> c_int;
    // AlignmentCorrection::correct_clustering_selected (phmm_likelihood_correction.rs:32-97)
    pub fn jtk_lc_correct_clustering(
        n_reads: usize, read_id: *const u64, node_off: *const u64, nodes: *const JtkCcNode, posteriors: *const f64,
        n_chunks: usize, chunks: *mut JtkCcChunk, n_selected: usize, selection: *const u64,
        haploid_coverage: f64, min_gain: f64, cluster_out: *mut u64, touched: *mut u8, device: c_int) -> c_int;
    // SquishErroneousClusters::squish_erroneous_clusters (squish_erroneous_clusters.rs:44-60), which pipeline.rs:174-175 and
    // dense_encoding.rs:62-64 run in front of correct_clustering; class_out: 0 Stiff, 1 Isolated, 2 Suspicious.  The four pair
    // arrays are optional (null skips them): the surviving chunk pairs ascending by (u1, u2)
    pub fn jtk_lc_squish_clusters(
        n_reads: usize, node_off: *const u64, nodes: *const JtkCcNode, posteriors: *const f64,
        n_chunks: usize, chunks: *mut JtkCcChunk, cfg: *const JtkSquishConfig, class_out: *mut u8,
        cluster_out: *mut u64, touched: *mut u8, pair_u1: *mut u64, pair_u2: *mut u64, pair_ari: *mut f64,
        pair_count: *mut u64, pair_cap: usize, n_pairs: *mut usize, device: c_int) -> c_int;
    // classify (:254-365) alone, on the host, on a pair list in the order given
    pub fn jtk_lc_squish_classify(
        n_pairs: usize, u1: *const u64, u2: *const u64, ari: *const f64, count: *const u64,
        cfg: *const JtkSquishConfig, ids: *mut u64, stiff: *mut u8, id_cap: usize, n_ids: *mut usize) -> c_int;
    // the step after the stage, `ds.purge` (purge_diverged.rs:42-48), and the two functions it rests on.  The flattened DataSet of
    // jtk_lc_correct_clustering plus what Node::recover reads: node sequences, per-base ops (0 Match, 1 Mismatch, 2 Ins, 3 Del)
    // and the chunk sequences in chunks[] order.
    // Node::recover's columns per node (definitions/src/lib.rs:773-813): err_num / err_len is the node's error rate
    pub fn jtk_lc_node_errors(
        n_reads: usize, node_off: *const u64, nodes: *const JtkCcNode, n_chunks: usize, chunks: *const JtkCcChunk,
        seq_bases: *const u8, seq_off: *const u64, ops: *const u8, ops_off: *const u64, tmpl_bases: *const u8, tmpl_off: *const u64,
        err_num: *mut u32, err_len: *mut u32, status: *mut i32, device: c_int) -> c_int;
    // calc_sim_thr (determine_chunks.rs:806-823; also deletion_fill.rs:141, jtk.rs:251, determine_chunks.rs:113,157,164)
    pub fn jtk_lc_error_quantile(n_nodes: usize, err_num: *const u32, err_len: *const u32, quantile: f64, out: *mut f64,
                                 device: c_int) -> c_int;
    // estimate_error_rate (estimate_error_rate.rs:37-133); chunk_err is flat in chunks[] order, chunk_err_off its n_chunks + 1 offsets
    pub fn jtk_lc_estimate_error_rate(
        n_reads: usize, node_off: *const u64, nodes: *const JtkCcNode, err_num: *const u32, err_len: *const u32,
        n_chunks: usize, chunks: *const JtkCcChunk, fallback: f64, read_err: *mut f64, chunk_err: *mut f64,
        chunk_err_off: *mut u64, chunk_err_cap: usize, median_of_sqrt_err: *mut f64, n_iter: *mut u32, device: c_int) -> c_int;
    // purge_diverged_nodes (purge_diverged.rs:238-322) up to the rebuild of the reads; read_err / chunk_err / median are optional
    pub fn jtk_lc_purge_diverged(
        n_reads: usize, node_off: *const u64, nodes: *const JtkCcNode, n_post: usize, n_chunks: usize, chunks: *mut JtkCcChunk,
        seq_bases: *const u8, seq_off: *const u64, ops: *const u8, ops_off: *const u64, tmpl_bases: *const u8, tmpl_off: *const u64,
        thr: f64, diverged: *mut u8, chunk_err_off: *mut u64, slot_cap: usize, keep: *mut u8, cluster_out: *mut u64,
        touched: *mut u8, post_keep: *mut u8, purged: *mut u64, purged_cap: usize, n_purged: *mut usize,
        read_err: *mut f64, chunk_err: *mut f64, median_of_sqrt_err: *mut f64, device: c_int) -> c_int;
    // the node statistics (remove_slippy_alignment::score, the identity of remove_overlapping_encoding, del_size of
    // purge_diverged.rs:75-80) and, unless mode is JTK_SETTLE_STATS_ONLY, the list surgery of encode/deletion_fill.rs:349-361 per read;
    // order[node_off[r] ..][.. n_kept[r]] = the surviving nodes' indices inside read r in their final order
    pub fn jtk_lc_settle_nodes(
        n_reads: usize, node_off: *const u64, nodes: *const JtkSettleNode, ops: *const u8, ops_off: *const u64, mode: c_int,
        stats: *mut JtkNodeStats, n_kept: *mut u32, order: *mut u32, keep: *mut u8, read_status: *mut i32,
        device: c_int) -> c_int;
    // mask_repeat (repeat_masking.rs:135-158): the reads upper-cased, then lower-cased where a masked k-mer covers a base; masked
    // may be `bases`; mask_kmers may be null with mask_cap 0.  -6 where create_mask's counts[percentile] panics
    pub fn jtk_lc_mask_repeats(
        n_reads: usize, bases: *const u8, read_off: *const u64, k: u32, freq: f64, min_count: u32, masked: *mut u8,
        mask_kmers: *mut u64, mask_cap: u64, report: *mut JtkMaskReport, device: c_int) -> c_int;
    // get_repetitive_kmer (repeat_masking.rs:109-134): the k-mers of the all-lower-case windows, ascending; -1 with *n_kmers = the
    // need where cap is too small
    pub fn jtk_lc_repetitive_kmers(
        n_reads: usize, bases: *const u8, read_off: *const u64, k: u32, kmers: *mut u64, cap: u64, n_kmers: *mut u64,
        device: c_int) -> c_int;
    // RepeatAnnot::repetitiveness (repeat_masking.rs:90-105) of every sequence as rep_num / rep_den; kmers ascending and unique
    pub fn jtk_lc_repetitiveness(
        n_seqs: usize, bases: *const u8, seq_off: *const u64, k: u32, kmers: *const u64, n_kmers: u64, rep_num: *mut u32,
        rep_den: *mut u32, device: c_int) -> c_int;
    // what encode_by_mm2 asks of minimap2 (encode/mod.rs:41-64, :315-355; minimap2.rs): where a chunk lies in a read, by this
    // library's own minimizer seeding and chaining (parity with minimap2's seeds and chains is not pinned).
    // Placements in the order (query, target, strand, diag_lo); -1 with *n_placements = the need where cap is too small.
    // (jtk_lc_debug_map_timing of jtk_lc_debug.h, the phases' times, is diagnostic and is not bound here.)
    pub fn jtk_lc_map_reads(
        n_targets: usize, target_bases: *const u8, target_off: *const u64, n_queries: usize, query_bases: *const u8,
        query_off: *const u64, params: *const JtkMapParams, out: *mut JtkMapPlacement, cap: u64, n_placements: *mut u64,
        device: c_int) -> c_int;
    // the minimizers alone, ascending by (seq, pos), as parallel arrays; -1 with *n = the need where cap is too small
    pub fn jtk_lc_sketch(
        n_seqs: usize, bases: *const u8, seq_off: *const u64, k: u32, w: u32, hash: *mut u64, seq: *mut u32, pos: *mut u32,
        strand: *mut u8, cap: u64, n: *mut u64, device: c_int) -> c_int;
    // get_pileup, ins_thr and check_insertion_head / _tail of correct_deletion_error (encode/deletion_fill.rs:301-337, 642-698,
    // 883-981) for every read with target[r] == 1 (null: every read); cands sorted by (read, slot, side, chunk, cluster, is_forward)
    pub fn jtk_lc_fill_candidates(
        n_reads: usize, node_off: *const u64, nodes: *const JtkFillNode, target: *const u8, coverage: *mut u32,
        ins_thr: *mut u32, cand_off: *mut u64, cands: *mut JtkFillCand, cand_cap: usize, n_cands: *mut usize,
        device: c_int) -> c_int;
    // kiley::bialignment::guided::{global_guided, infix_guided} on this library's own specification (parity
    // with kiley is not pinned): mode 0 global, 1 infix (both ends of x free); Del consumes an x base, Ins a y base
    pub fn jtk_lc_align_guided(
        n_pairs: usize, pairs: *const JtkGuidedPair, x_bases: *const u8, y_bases: *const u8, guide_ops: *const u8, mode: c_int,
        mat: c_int, mismatch: c_int, gap_open: c_int, gap_ext: c_int, ops_out: *mut u8, ops_out_off: *mut u64, ops_cap: u64,
        score_out: *mut i32, start_out: *mut u32, end_out: *mut u32, status: *mut i32, device: c_int) -> c_int;
    // kiley::bialignment::guided::polish_until_converge(_with) on this library's own specification ("Guided
    // polishing"; parity with kiley's polish is not pinned): encode/deletion_fill.rs:260-285, polish_chunks.rs:64-65,
    // consensus/mod.rs:442,470-472, determine_chunks.rs:439, dense_encoding.rs:575-577.  radius: one per chunk; take_num 0 = every
    // read votes; max_rounds 0 = 20; dist_out: one per read
    pub fn jtk_lc_polish_guided(
        n_chunks: usize, chunks: *const JtkLcChunk, tmpl_bases: *const u8, read_bases: *const u8, read_off: *const u64,
        ops: *const u8, ops_off: *const u64, radius: *const u32, take_num: u32, ignore_edge: u32, max_rounds: u32,
        cons_out: *mut u8, cons_off: *mut u64, cons_cap: u64, ops_out: *mut u8, ops_out_off: *mut u64, ops_cap: u64,
        dist_out: *mut u32, result: *mut JtkLcResult, device: c_int) -> c_int;
    // encode_node with fine_mapping and fit_query_by_edlib (encode/deletion_fill.rs:451-566) for a batch of trials; verdict 0
    // accepted, 1 the lower-bound filter (:461-465), 2 identity or edge (:504-505)
    pub fn jtk_lc_encode_nodes(
        n_trials: usize, trials: *const JtkEncodeTrial, read_bases: *const u8, cons_bases: *const u8, chunk_bases: *const u8,
        result: *mut JtkEncodeResult, ops_out: *mut u8, ops_out_off: *mut u64, ops_cap: u64, device: c_int) -> c_int;
    // encode_edge with tune_position (dense_encoding.rs:627-759) for a batch of trials: one node record per chunk of the trial's
    // contig, in chunk order; verdict 0 accepted, 2 rejected (:671), 3 not reached
    pub fn jtk_lc_encode_edges(
        n_trials: usize, trials: *const JtkEdgeTrial, read_bases: *const u8, contig_bases: *const u8, break_points: *const u32,
        node_off: *const u64, result: *mut JtkEdgeResult, nodes: *mut JtkEdgeNode, ops_out: *mut u8, ops_out_off: *mut u64,
        ops_cap: u64, device: c_int) -> c_int;
    // the resident-batch form (jtk_lc.h: session_create + run + fetch == jtk_lc_cluster_chunks) and, on it, the reference's
    // trace! rows of one chunk (TOTAL / CAND / PICK / DUMP / RANGE / LK / COUNTS; pseudo_mcmc.rs:122-127,236,250-262,467-472,539)
    pub fn jtk_lc_session_create(
        params: *const JtkLcParams, n_chunks: usize, chunks: *const JtkLcChunk,
        tmpl_bases: *const u8, read_bases: *const u8, read_off: *const u64,
        ops: *const u8, ops_off: *const u64, strand: *const u8, post_stride: u32, device: c_int,
        out: *mut *mut c_void) -> c_int;
    pub fn jtk_lc_session_run(s: *mut c_void, skip_polish: c_int) -> c_int;
    pub fn jtk_lc_session_trace(s: *mut c_void, chunk: usize, text: *mut c_char, cap: usize, len: *mut usize) -> c_int;
    pub fn jtk_lc_session_destroy(s: *mut c_void) -> c_int;
    pub fn jtk_lc_trim_cache(device: c_int) -> c_int;          // hand pooled device workspaces back to the driver
    pub fn jtk_lc_strerror(status: c_int) -> *const c_char;
    pub fn jtk_lc_last_error() -> *const c_char;
}
