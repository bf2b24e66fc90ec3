// prim_host.h -- the host toolkit of the stand-alone primitives (squish, purge, fill, guided, encode_nodes, gpolish,
// correction): a typed device array over DevBuf, a stream with its timing events, the block rocprim's calls borrow, and the
// grid size of a grid-stride launch.  Every member that calls HIP hands the hipError_t (or DevBuf::upload's status) back, so
// call sites keep their JTK_HIP_TRY and their own messages.
#pragma once
#include "host_common.h"

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
