// encode_window.h -- the window of a raw read as encode_node (deletion_fill.rs:467-472) and tune_position
// (dense_encoding.rs:722-727) take it: reverse-complemented when the trial is reverse, upper-cased.  encode_nodes.hip and
// encode_edges.hip include it; the kernel stays local to each of them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

struct EnWindow {
    uint64_t off;   // into the raw slices and into the windows alike
    uint32_t len, is_forward;
};

// one workgroup per window; flags |= 1 where a base is not ACGT after upper-casing
__global__ void __launch_bounds__(256) encode_window_kernel(uint32_t n, const EnWindow *wins, const uint8_t *raw, uint8_t *out, uint32_t *flags) {
    const uint32_t t = blockIdx.x;
    if (t >= n) return;
    const EnWindow w = wins[t];
    bool bad = false;
    for (uint32_t q = threadIdx.x; q < w.len; q += blockDim.x) {
        uint8_t c = raw[w.off + (w.is_forward ? q : w.len - 1 - q)];
        if (c >= 'a' && c <= 'z') c -= 32;
        if (!w.is_forward) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c;
        bad |= c != 'A' && c != 'C' && c != 'G' && c != 'T';
        out[w.off + q] = c;
    }
    if (bad) atomicOr(flags, 1u);
}

}  // namespace
