// host_common.h -- the host plumbing every translation unit with entry points shares: the per-thread error string and timing
// record, the one HIP error macro, the gfx950 device check, a plain RAII device buffer and the read-order walk of a flat batch.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "jtk_lc.h"

// What jtk_lc_last_error() / jtk_lc_last_timing() report, per host thread (defined in session.hip).  The worker threads of the
// sliced and the multi-GPU one-shot calls fill their own and hand them to the calling thread.
extern thread_local std::string g_last_error;
extern thread_local jtk_lc_timing_t g_timing;

int jtk_fail(int status, const std::string &msg);  // sets the thread's error string, returns `status`

#define JTK_HIP_TRY(expr)                                                                      \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return jtk_fail(_e == hipErrorOutOfMemory ? JTK_ERR_ALLOC : JTK_ERR_NO_DEVICE,     \
                            std::string(#expr) + ": " + hipGetErrorString(_e));                \
    } while (0)

// Makes `device` current if it is a visible gfx950; JTK_ERR_NO_DEVICE and a message otherwise (there is no CPU fallback).
int jtk_require_device(int device);

// A block straight from hipMalloc, freed with its owner.  The entry points beside the session (gains, correction, alignment)
// hold a handful each per call; the session's own workspaces come from its block pool (session_internal.h: DevPtr).
struct DevBuf {
    void *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t bytes) {  // a previous block goes first
        if (p) (void)hipFree(p);
        p = nullptr;
        return hipMalloc(&p, bytes);
    }
    template <typename T>
    int upload(const std::vector<T> &v, hipStream_t st) {
        if (alloc(std::max<size_t>(v.size(), 1) * sizeof(T)) != hipSuccess) return JTK_ERR_ALLOC;
        if (!v.empty() && hipMemcpyAsync(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st) != hipSuccess)
            return JTK_ERR_NO_DEVICE;
        return 0;
    }
};

// The chunks of a flat batch list their reads back to back, in order (jtk_lc_chunk_t and jtk_lc_feature_chunk_t alike).
template <typename Chunk>
int check_contiguous(const Chunk *chunks, size_t n_chunks, uint64_t *n_reads) {
    uint64_t n = 0;
    for (size_t c = 0; c < n_chunks; c++) {
        if (chunks[c].read_first != n) return jtk_fail(JTK_ERR_INVALID_ARG, "chunks must list their reads contiguously in order");
        n += chunks[c].n_reads;
    }
    *n_reads = n;
    return 0;
}

// session_refit.hip: log P(read | template) of every read of a batch with a fixed band radius (the gains calibration's scorer)
extern "C" int jtk_internal_likelihoods(const jtk_lc_params_t *params, size_t n_chunks, const jtk_lc_chunk_t *chunks,
                                        const uint8_t *tmpl_bases, const uint8_t *read_bases, const uint64_t *read_off,
                                        const uint8_t *ops, const uint64_t *ops_off, const uint8_t *strand,
                                        uint32_t radius, int device, double *lk_out);
