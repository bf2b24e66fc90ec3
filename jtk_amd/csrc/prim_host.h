// prim_host.h -- the host toolkit of the stand-alone primitives (squish, purge, settle, fill, mask, map, guided, encode_nodes,
// gpolish, correction): a typed device array over DevBuf, a stream with its timing events, the block rocprim's calls borrow, the
// grid size of a grid-stride launch, the check every offsets array gets, the refusal of a work area the device has no room
// for, and the sequences of a k-mer primitive on the device.  Every member that calls HIP hands the hipError_t (or
// DevBuf::upload's status) back, so call sites keep their JTK_HIP_TRY and their own messages.
#pragma once
#include <string>

#include "host_common.h"
#include "kmer_plan.h"

// blocks of `per` elements for n of them: at least one, at most `cap` (the kernels stride over the rest)
inline uint32_t jtk_blocks(uint64_t n, uint32_t per, uint32_t cap) {
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((n + per - 1) / per, 1), cap);
}

// `count` elements of T on the device.  An empty array still owns a block (of one element), so get() is never null after
// alloc or upload and a kernel that is handed the pointer of an empty input has something to point at.
template <typename T>
struct DevArr {
    DevBuf buf;
    T *get() const { return static_cast<T *>(buf.p); }
    const T *cget() const { return static_cast<const T *>(buf.p); }
    hipError_t alloc(size_t count) { return buf.alloc(std::max<size_t>(count, 1) * sizeof(T)); }
    // The copies are asynchronous: the host side must live until the caller has synchronised `st`.
    int upload(const std::vector<T> &v, hipStream_t st) { return buf.upload(v, st); }
    int upload(const T *src, size_t count, hipStream_t st) {
        if (alloc(count) != hipSuccess) return JTK_ERR_ALLOC;
        if (count && hipMemcpyAsync(buf.p, src, count * sizeof(T), hipMemcpyHostToDevice, st) != hipSuccess) return JTK_ERR_NO_DEVICE;
        return 0;
    }
    hipError_t download(T *dst, size_t count, hipStream_t st, size_t first = 0) const {
        return hipMemcpyAsync(dst, cget() + first, count * sizeof(T), hipMemcpyDeviceToHost, st);
    }
    hipError_t zero(size_t count, hipStream_t st) { return hipMemsetAsync(buf.p, 0, count * sizeof(T), st); }
};

// Up to four events that go with their owner; create() makes the first n of them (those it has already made stay).
struct DevEvents {
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    DevEvents() = default;
    DevEvents(const DevEvents &) = delete;
    DevEvents &operator=(const DevEvents &) = delete;
    ~DevEvents() { destroy(); }
    void destroy() {
        for (hipEvent_t &x : e) {
            if (x) (void)hipEventDestroy(x);
            x = nullptr;
        }
    }
    hipError_t create(int n) {
        for (int i = 0; i < n; i++)
            if (!e[i])
                if (hipError_t err = hipEventCreate(&e[i])) return err;
        return hipSuccess;
    }
    hipEvent_t operator[](int i) const { return e[i]; }
    hipError_t elapsed(int i, int j, float *ms) const { return hipEventElapsedTime(ms, e[i], e[j]); }
};

// A stream that dies with its scope, and the events recorded on it.
struct DevStream {
    hipStream_t st = nullptr;
    DevEvents ev;
    DevStream() = default;
    DevStream(const DevStream &) = delete;
    DevStream &operator=(const DevStream &) = delete;
    ~DevStream() {  // the events first, then the stream
        ev.destroy();
        if (st) (void)hipStreamDestroy(st);
    }
    hipError_t create(int n_events = 0) {
        if (hipError_t err = hipStreamCreate(&st)) return err;
        return ev.create(n_events);
    }
    hipError_t elapsed(int i, int j, float *ms) const { return ev.elapsed(i, j, ms); }
};

// The temporary block of rocprim's two-call protocol: `call(nullptr, bytes)` asks for the size, `call(block, bytes)` runs.
// The block only grows and serves every call of its owner.  Growing frees the old block with hipFree, which waits for the
// device: that is what makes it safe while an earlier rocprim call that uses the old block is still queued.
struct RocTemp {
    DevBuf buf;
    size_t bytes = 0;
    template <typename Call>
    hipError_t run(Call &&call) {
        size_t need = 0;
        if (hipError_t err = call(nullptr, need)) return err;
        if (need > bytes) {
            bytes = 0;
            if (hipError_t err = buf.alloc(need)) return err;
            bytes = need;
        }
        return call(buf.p, need);
    }
};

// offsets of `n` slices: they start at 0 and never decrease (JTK_ERR_INVALID_ARG), and no slice is longer than max_slice
// (JTK_ERR_UNSUPPORTED), tested slice by slice in that order.  `off` is not null.
inline int jtk_check_offsets(size_t n, const uint64_t *off, const char *what, uint64_t max_slice = ~0ull) {
    if (off[0] != 0) return jtk_fail(JTK_ERR_INVALID_ARG, std::string(what) + "[0] is not 0");
    for (size_t i = 0; i < n; i++) {
        if (off[i + 1] < off[i]) return jtk_fail(JTK_ERR_INVALID_ARG, std::string(what) + " decreases");
        if (off[i + 1] - off[i] > max_slice)
            return jtk_fail(JTK_ERR_UNSUPPORTED, std::string(what) + ": a slice of more than " + std::to_string(max_slice) + " entries");
    }
    return 0;
}

// refuses `what` (a work area, a buffer) above 80 % of the device's free memory, before anything of it is allocated
inline int jtk_fits(uint64_t bytes, const char *what) {
    size_t free_b = 0, total_b = 0;
    JTK_HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if ((double)bytes > 0.8 * (double)free_b)
        return jtk_fail(JTK_ERR_ALLOC, std::string(what) + " of this call is " + std::to_string(bytes) + " bytes, above 80 % of the device's " +
                                           std::to_string(free_b) + " free bytes");
    return 0;
}

// The sequences of a k-mer primitive on the device: bases, offsets and the tiles of a KmerPlan; kmer_off only where the
// kernels write a k-mer at its position's own slot (with_kmer_off).
struct DevSeqs {
    DevArr<uint8_t> bases;
    DevArr<uint64_t> off, kmer_off;
    DevArr<uint32_t> tile_seq, tile_start;
    uint32_t n_tiles = 0;
    static uint64_t bytes(size_t n, const uint64_t *h_off, const KmerPlan &P, bool with_kmer_off) {
        return h_off[n] + (with_kmer_off ? 16 : 8) * (uint64_t)(n + 1) + 8 * (uint64_t)P.tile_seq.size();
    }
    // (asynchronous: the host side, P included, must live until the caller has synchronised `st`)
    int upload(size_t n, const uint8_t *h_bases, const uint64_t *h_off, const KmerPlan &P, bool with_kmer_off, hipStream_t st) {
        int rc;
        if ((rc = bases.upload(h_bases, h_off[n], st)) || (rc = off.upload(h_off, n + 1, st)) || (with_kmer_off && (rc = kmer_off.upload(P.kmer_off, st))) ||
            (rc = tile_seq.upload(P.tile_seq, st)) || (rc = tile_start.upload(P.tile_start, st)))
            return jtk_fail(rc, "device upload failed");
        n_tiles = (uint32_t)P.tile_seq.size();
        return 0;
    }
};
