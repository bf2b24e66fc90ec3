// guided_internal.h -- the guided aligner of guided.hip as encode_nodes.hip drives it: pair descriptors, sequences and guides
// already on the device, results left there.
#pragma once
#include <vector>

#include "prim_host.h"

// One batch of pairs on the device.  The host knows an upper bound of every pair's lengths (exact ones where it made the
// descriptors itself); the work area is budgeted from those, so descriptors a kernel wrote need no trip to the host.
struct GuidedBatch {
    size_t n = 0;
    const jtk_guided_pair_t *d_pairs = nullptr;
    const uint8_t *d_x = nullptr, *d_y = nullptr, *d_guide = nullptr;
    int infix = 0;
    int32_t match = 0, mismatch = 0, gap_open = 0, gap_ext = 0;
    const uint32_t *h_xlen = nullptr, *h_ylen = nullptr, *h_radius = nullptr;  // bounds, per pair
    // results, per pair; d_status comes in: a pair whose status is not 0 is left alone
    int32_t *d_score = nullptr, *d_status = nullptr;
    uint32_t *d_start = nullptr, *d_end = nullptr, *d_nops = nullptr;
    // pair p's ops END at d_slots + h_slot_end[p] (d_slot_end is the same list on the device); its slot holds h_xlen[p] + h_ylen[p] bytes
    uint8_t *d_slots = nullptr;
    const uint64_t *d_slot_end = nullptr;
};

// A pair's share of the work area of its slice.
struct GuidedWork {
    uint64_t tab_off;  // into the row tables, in uint32: 2 (n + 2) entries -- first column of every row, then its offset (n + 2 of them)
    uint64_t tb_off;   // into the traceback bytes
    uint64_t tb_cap;   // cells the slice holds for this pair
};

// The work area: row tables, traceback bytes, and the rows of the waves that keep theirs in global memory.  Batches that run
// behind each other on one stream share one; it is grown (guided_reserve) before anything that uses it is enqueued.
struct GuidedArea {
    DevArr<uint32_t> tab;
    DevArr<uint8_t> tb;
    DevArr<int32_t> rows;
    uint64_t tab_have = 0, tb_have = 0;
    bool rows_have = false;
};

// One batch's plan and what its kernels need besides the area.  It owns the host table its upload reads and the device blocks
// its kernels use, so it must live until the caller has synchronised the stream.
struct GuidedRun {
    std::vector<GuidedWork> work;       // per pair; the asynchronous upload reads it
    std::vector<uint32_t> slice_first;  // first pair of every slice, then n
    uint64_t tab_need = 0, tb_need = 0; // of the largest slice: uint32 entries, bytes
    bool any_large = false;
    DevArr<GuidedWork> d_work;
    DevArr<uint32_t> maxw;
    DevArr<unsigned long long> cells;
    DevEvents ev;                       // around the batch's kernels
    uint32_t slices = 0;
};
// host only: the shares of the work area and the slices the budget asks for
int guided_plan(const GuidedBatch &b, GuidedRun &run);
// grows the area to what the plan needs; frees and allocates, so it comes before the first enqueue on the area
int guided_reserve(GuidedArea &area, const GuidedRun &run);
// enqueues the planned batch on `st`, slice behind slice; returns without waiting
int guided_enqueue(const GuidedBatch &b, GuidedRun &run, GuidedArea &area, hipStream_t st);
// after the stream is synchronised: kernel ms and the cells filled
int guided_elapsed(const GuidedRun &run, double *ms, double *cells);
// packs the ops of the slots behind each other: out[dst_off[p] ..) = the n_ops[p] bytes that end at slot_end[p]
int guided_pack(size_t n, const uint8_t *d_slots, const uint64_t *d_slot_end, const uint32_t *d_nops, const uint64_t *d_dst_off,
                uint8_t *d_out, hipStream_t st);
uint64_t guided_scratch_cap();  // the work-area budget in bytes (jtk_lc_debug_guided_scratch_cap or the default)
