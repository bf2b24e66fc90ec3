// mask.hip -- jtk_lc_mask_repeats, jtk_lc_repetitive_kmers, jtk_lc_repetitiveness: canonical k-mer counting over the raw reads and
// what the reference does with the counts.
//
//   mask_repeat (repeat_masking.rs:135-158)        upper-case every read, create_mask, mask_repeats on every read
//   KMers / to_idx (:39-85, :196-208)              forward strand: base i at bits 2i (A C G T = 0 1 2 3); reverse strand: the last
//                                                  base's complement at bits 0..1 (A C G T = 3 2 1 0); EVERY OTHER BYTE IS 0 IN BOTH
//                                                  TABLES, so the reverse strand is not the bitwise complement of the forward one
//   create_mask (:255-285)                         counts, singletons dropped, the percentile over the counts above `min`
//   mask_repeats (:287-325)                        a base is lower case iff a masked k-mer starts in [j - k + 1, j]
//   get_repetitive_kmer (:109-134)                 to_idx of every window whose bytes are all ASCII lower case
//   repetitiveness (:90-105)                       per sequence, the occurrences of the set's k-mers that occur more than once
// On the device a read is cut into tiles of MK_TILE bases, one workgroup per tile.  The workgroup stages the tile's bytes (and a
// halo) in LDS and packs them into three bit streams: the forward codes, the complement codes IN REVERSED ORDER, and an
// "is lower case" bit.  A byte that is no base has code 0 in both code streams -- the second stream is the validity the 2-bit
// forward code lacks -- and with the second stream reversed the reverse-strand k-mer of a position is a bit field of it, as the
// forward k-mer is of the first: each lane forms both from three LDS words by shifts.  One emit kernel serves the three entry
// points (every position; windows that are all lower case; k-mers that are in a sorted set, with the sequence's index above
// the k-mer).  Counting is one radix sort over the 2k bits of the keys, run lengths, and selections (rocprim); the only value the
// host waits for is M, the number of k-mers counted more than once, because the percentile is an f64 expression of it.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "jtk_lc_debug.h"
#include "kmer_tile.h"
#include "prim_host.h"
#include "wave_util.h"

namespace {

constexpr uint32_t MK_THREADS = 256;
constexpr uint32_t MK_WAVES = MK_THREADS / 64;
constexpr uint32_t MK_TILE = 2048;                       // bases of a read per workgroup
constexpr uint32_t MK_PRE = 64;                          // positions in front of a tile whose hits reach into it: one ballot word (k - 1 <= 30)
constexpr uint32_t MK_STAGE = MK_PRE + MK_TILE + 32;     // bytes staged at most (the halo behind a tile is k - 1 <= 30 bases)
constexpr uint32_t MK_W2 = MK_STAGE / 16;                // words of a 2-bit stream
constexpr uint32_t MK_W1 = MK_STAGE / 32;                // words of the 1-bit stream
constexpr uint32_t MK_MAX_K = 31;
enum { MK_EVERY = 0, MK_LOWER = 1, MK_MEMBER = 2 };      // which positions the emit kernel writes
static_assert(MK_STAGE % 32 == 0, "the streams are whole words");

thread_local double g_mask_timing[4];  // ms: emit, sort, count and select, apply

struct Tile {
    uint8_t raw[MK_STAGE];
    uint32_t fwd[MK_W2 + 2], rev[MK_W2 + 2], low[MK_W1 + 1];  // each stream and its zero words (kmer_tile.h)
};

// Bases a .. a + MK_STAGE of the read (0 behind its end) into the tile's streams, by the whole workgroup.  Local index i is the
// read's base a + i; it sits at position i of fwd and low and at position MK_STAGE - 1 - i of rev.
__device__ __forceinline__ void mk_stage(Tile &T, const uint8_t *read, uint32_t len, uint32_t a) {
    jtk_stage_bytes<MK_STAGE, MK_THREADS>(T.raw, read, len, a);
    __syncthreads();
    jtk_pack2<MK_W2, MK_THREADS>({T.fwd, T.rev}, [&](uint32_t i) { return jtk_base_code(T.raw[i]); },
                                 [&](uint32_t i) { return jtk_base_complement(T.raw[MK_STAGE - 1 - i]); });
    jtk_pack1<MK_W1, MK_THREADS>(T.low, [&](uint32_t i) { return T.raw[i] >= 'a' && T.raw[i] <= 'z' ? 1u : 0u; });
    __syncthreads();
}

// the canonical k-mer of the window at local index q
__device__ __forceinline__ uint64_t mk_kmer(const Tile &T, uint32_t q, uint32_t k) {
    const uint64_t f = jtk_field2(T.fwd, q, k), r = jtk_field2(T.rev, MK_STAGE - q - k, k);
    return f < r ? f : r;
}

__device__ __forceinline__ bool mk_all_lower(const Tile &T, uint32_t q, uint32_t k) { return jtk_field1(T.low, q, k) == (1u << k) - 1; }

template <typename Key>
__device__ __forceinline__ bool mk_member(const Key *list, uint64_t n, Key x) {
    const uint64_t at = jtk_lower_bound(list, n, x);
    return at < n && list[at] == x;
}

// One workgroup per tile.  MK_EVERY: the k-mer of position p of read r goes to out[kmer_off[r] + p].  MK_LOWER / MK_MEMBER:
// the positions that pass are appended at *cursor, one atomic per wave and step (the order is the sort's to make); a member's
// record carries the read's index above the k-mer.
template <typename Key>
__global__ void __launch_bounds__(MK_THREADS) emit_kernel(const uint8_t *bases, const uint64_t *read_off, const uint64_t *kmer_off,
                                                          const uint32_t *tile_read, const uint32_t *tile_start, uint32_t k, int mode,
                                                          const uint64_t *set, uint64_t n_set, Key *out, unsigned long long *cursor) {
    __shared__ Tile T;
    const uint32_t r = tile_read[blockIdx.x], s = tile_start[blockIdx.x], lane = threadIdx.x & 63u;
    const uint64_t ro = read_off[r];
    const uint32_t len = (uint32_t)(read_off[r + 1] - ro);
    if (len < k || s > len - k) return;  // no k-mer starts in this tile
    const uint32_t n_pos = len - k + 1 - s < MK_TILE ? len - k + 1 - s : MK_TILE;
    mk_stage(T, bases + ro, len, s);
    for (uint32_t q0 = 0; q0 < n_pos; q0 += MK_THREADS) {
        const uint32_t q = q0 + threadIdx.x;
        const bool active = q < n_pos;
        const uint64_t kmer = active ? mk_kmer(T, q, k) : 0;
        if (mode == MK_EVERY) {
            if (active) out[kmer_off[r] + s + q] = (Key)kmer;
            continue;
        }
        const bool pass = active && (mode == MK_LOWER ? mk_all_lower(T, q, k) : mk_member(set, n_set, kmer));
        const uint64_t votes = __ballot(pass);
        if (!votes) continue;
        unsigned long long first = 0;
        if (lane == 0) first = atomicAdd(cursor, (unsigned long long)__popcll(votes));
        first = __shfl(first, 0, 64);
        if (pass) {
            const uint64_t rec = mode == MK_MEMBER ? ((uint64_t)r << (2 * k)) | kmer : kmer;
            out[first + (uint64_t)__popcll(votes & ((1ull << lane) - 1))] = (Key)rec;
        }
    }
}

// One workgroup per tile; it also stages the MK_PRE positions in front of the tile.  Each wave ballots the hits of 64 positions
// into a word of LDS; the covered word of a block of 64 bases is the OR of (previous word : own word) << s over s < k, made by
// doubling; each lane writes its base in the case its bit says.  *n_lower grows by the bits, one atomic per wave.
template <typename Key>
__global__ void __launch_bounds__(MK_THREADS) apply_kernel(const uint8_t *bases, const uint64_t *read_off, const uint32_t *tile_read,
                                                           const uint32_t *tile_start, uint32_t k, const Key *mask,
                                                           const unsigned long long *n_mask, uint8_t *out, unsigned long long *n_lower) {
    __shared__ Tile T;
    __shared__ uint64_t s_hits[(MK_PRE + MK_TILE) / 64];
    const uint32_t r = tile_read[blockIdx.x], s = tile_start[blockIdx.x], lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint64_t ro = read_off[r];
    const uint32_t len = (uint32_t)(read_off[r + 1] - ro);
    const uint32_t a = s ? s - MK_PRE : 0, pre = s - a;  // tiles start at multiples of MK_TILE
    mk_stage(T, bases + ro, len, a);
    const uint64_t nm = *n_mask;
    const uint32_t n_words = (pre + MK_TILE) / 64;
    for (uint32_t w = wv; w < n_words; w += MK_WAVES) {
        const uint32_t q = w * 64 + lane;
        bool hit = false;
        if (nm && (uint64_t)a + q + k <= len) hit = mk_member(mask, nm, (Key)mk_kmer(T, q, k));
        const uint64_t votes = __ballot(hit);
        if (lane == 0) s_hits[w] = votes;
    }
    __syncthreads();
    uint64_t lower = 0;
    for (uint32_t b = wv; b < MK_TILE / 64; b += MK_WAVES) {
        const uint32_t p0 = s + 64 * b;
        if (p0 >= len) break;
        const uint32_t hb = b + pre / 64;
        uint64_t cur = s_hits[hb], prev = hb ? s_hits[hb - 1] : 0;
        for (uint32_t span = 1; span < k;) {  // bit j: a hit in [j - span + 1, j]
            const uint32_t step = span < k - span ? span : k - span;
            cur |= (cur << step) | (prev >> (64 - step));
            prev |= prev << step;  // its top bits are all the next step reads of it, and they are complete: span <= 16 here
            span += step;
        }
        lower += (uint64_t)__popcll(cur);
        if (p0 + lane < len) {  // (p0 + lane < 2^32: len is)
            uint32_t c = T.raw[pre + 64 * b + lane];
            const bool covered = (cur >> lane) & 1ull;
            if (c >= 'a' && c <= 'z') c -= 32;
            if (covered && c >= 'A' && c <= 'Z') c += 32;
            out[ro + p0 + lane] = (uint8_t)c;
        }
    }
    if (lane == 0 && lower) atomicAdd(n_lower, (unsigned long long)lower);
}

struct MoreThanOnce {
    __device__ bool operator()(uint32_t c) const { return c > 1u; }
};
struct MoreThan {
    const uint32_t *thr;
    __device__ bool operator()(uint32_t c) const { return c > *thr; }
};

// create_mask's verdict over the ascending counts of the M k-mers counted more than once: v[0] = thr, v[1] = takes all,
// v[2] = the index is out of range (the reference panics), v[3] = the mask is the k-mers counted more than v[3] times
__global__ void verdict_kernel(const uint32_t *sorted, uint64_t m, uint64_t percentile, uint32_t min_count, uint32_t *v) {
    uint64_t lo = 0, hi = m;  // below_min = the counts <= min_count (not jtk_lower_bound of min_count + 1, which is 0 at 0xffffffff)
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (sorted[mid] <= min_count)
            lo = mid + 1;
        else
            hi = mid;
    }
    v[0] = v[1] = v[2] = v[3] = 0;
    if (percentile < lo) {
        v[1] = 1;
    } else if (percentile >= m) {
        v[2] = 1;
        v[3] = 0xffffffffu;
    } else {  // element percentile - below_min of the counts above min_count
        v[0] = v[3] = sorted[percentile];
    }
}

__global__ void ascending_kernel(const uint64_t *set, uint64_t n, uint32_t *bad) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i + 1 < n; i += (uint64_t)gridDim.x * blockDim.x)
        if (set[i] >= set[i + 1]) *bad = 1;
}

// runs of (sequence, k-mer) records: a run of more than one adds its length to the sequence's count
__global__ void repeated_kernel(const uint64_t *rec, const uint32_t *count, const uint32_t *n_runs, uint32_t k, uint32_t *rep_num) {
    const uint64_t n = *n_runs;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        if (count[i] > 1u) atomicAdd(&rep_num[rec[i] >> (2 * k)], count[i]);
}

// ---- the host side

// what all three entry points ask of their sequences and k, before a device is looked for
int mk_check(size_t n, const uint8_t *bases, const uint64_t *off, uint32_t k, const char *what) {
    if (!off) return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    if (k == 0) return jtk_fail(JTK_ERR_INVALID_ARG, "k is 0");
    if (k > MK_MAX_K) return jtk_fail(JTK_ERR_UNSUPPORTED, "k is above 31 (the reference asserts k < 32)");
    if (int rc = jtk_check_offsets(n, off, what)) return rc;
    if (off[n] && !bases) return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    if (off[n] >> 32 || (uint64_t)n >> 32) return jtk_fail(JTK_ERR_UNSUPPORTED, "2^32 bases or sequences, or more: a count would not fit the reference's u32");
    return 0;
}

// the tiles of a call and where each read's k-mers go: a read shorter than k has tiles too, apply_kernel copies it
KmerPlan mk_plan(size_t n, const uint64_t *off, uint32_t k) { return jtk_plan_kmers(n, off, k, MK_TILE, KMER_TILE_BASES); }

template <typename Key>
hipError_t mk_sort(RocTemp &tmp, const Key *in, Key *out, uint64_t n, uint32_t end_bit, hipStream_t st) {
    return tmp.run([&](void *t, size_t &bytes) { return rocprim::radix_sort_keys(t, bytes, in, out, (size_t)n, 0u, end_bit, st); });
}

template <typename Key>
int mk_mask(size_t n_reads, const uint8_t *bases, const uint64_t *read_off, uint32_t k, double freq, uint32_t min_count, uint8_t *masked,
            uint64_t *mask_kmers, uint64_t mask_cap, jtk_mask_report_t *report, const KmerPlan &P) {
    const uint64_t n = P.n_kmers, half = (n + 1) / 2, n_bases = read_off[n_reads];
    DevStream s;
    JTK_HIP_TRY(s.create(4));
    DevEvents late;
    JTK_HIP_TRY(late.create(1));
    {  // keys twice, rocprim's block, the runs and their counts, the counts again for the percentile; the reads twice
        size_t sort_tmp = 0;
        if (n) JTK_HIP_TRY(rocprim::radix_sort_keys(nullptr, sort_tmp, (const Key *)nullptr, (Key *)nullptr, (size_t)n, 0u, 2 * k, s.st));
        const uint64_t work = DevSeqs::bytes(n_reads, read_off, P, true) + n_bases + (2 * (n + 1) + n) * sizeof(Key) + sort_tmp + (2 * n + 2) * 4;
        if (int rc = jtk_fits(work, "the work area")) return rc;
    }
    DevSeqs R;
    if (int rc = R.upload(n_reads, bases, read_off, P, true, s.st)) return rc;
    // raw: the keys as emitted; once they are sorted, its halves hold the k-mers counted more than once and the mask (each has
    // a count of two or more, so there are at most n / 2 of them)
    DevArr<Key> d_raw, d_sorted, d_uniq;
    DevArr<uint32_t> d_count, d_repeated, d_runs, d_verdict;  // repeated: the counts above one, then those in ascending order
    DevArr<size_t> d_sel;                                      // selected: k-mers counted more than once (twice), masked
    DevArr<unsigned long long> d_lower;
    DevArr<uint8_t> d_out;
    RocTemp tmp;
    JTK_HIP_TRY(d_raw.alloc(n + 1));
    JTK_HIP_TRY(d_sorted.alloc(n));
    JTK_HIP_TRY(d_uniq.alloc(n));
    JTK_HIP_TRY(d_count.alloc(n));
    JTK_HIP_TRY(d_repeated.alloc(n + 1));
    JTK_HIP_TRY(d_runs.alloc(1));
    JTK_HIP_TRY(d_verdict.alloc(4));
    JTK_HIP_TRY(d_sel.alloc(3));
    JTK_HIP_TRY(d_lower.alloc(1));
    JTK_HIP_TRY(d_out.alloc(n_bases));
    JTK_HIP_TRY(d_count.zero(std::max<uint64_t>(n, 1), s.st));  // the entries behind the runs are no k-mer's count
    JTK_HIP_TRY(d_runs.zero(1, s.st));
    JTK_HIP_TRY(d_verdict.zero(4, s.st));
    JTK_HIP_TRY(d_sel.zero(3, s.st));
    JTK_HIP_TRY(d_lower.zero(1, s.st));
    Key *const d_repeated_kmers = d_raw.get(), *const d_mask = d_raw.get() + half;
    uint32_t *const d_ascending = d_repeated.get() + half;
    uint32_t h_runs = 0, h_verdict[4] = {0, 0, 1, 0};
    size_t h_sel[3] = {0, 0, 0};
    unsigned long long h_lower = 0;
    JTK_HIP_TRY(hipEventRecord(s.ev[0], s.st));
    if (n) emit_kernel<Key><<<R.n_tiles, MK_THREADS, 0, s.st>>>(R.bases.cget(), R.off.cget(), R.kmer_off.cget(), R.tile_seq.cget(), R.tile_start.cget(),
                                                               k, MK_EVERY, nullptr, 0, d_raw.get(), nullptr);
    JTK_HIP_TRY(hipEventRecord(s.ev[1], s.st));
    if (n) JTK_HIP_TRY(mk_sort<Key>(tmp, d_raw.cget(), d_sorted.get(), n, 2 * k, s.st));
    JTK_HIP_TRY(hipEventRecord(s.ev[2], s.st));
    if (n) {
        JTK_HIP_TRY(tmp.run([&](void *t, size_t &bytes) {
            return rocprim::run_length_encode(t, bytes, d_sorted.cget(), (unsigned int)n, d_uniq.get(), d_count.get(), d_runs.get(), s.st);
        }));
        JTK_HIP_TRY(tmp.run([&](void *t, size_t &bytes) {
            return rocprim::select(t, bytes, d_count.cget(), d_repeated.get(), d_sel.get(), (size_t)n, MoreThanOnce(), s.st);
        }));
        JTK_HIP_TRY(tmp.run([&](void *t, size_t &bytes) {
            return rocprim::select(t, bytes, d_uniq.cget(), rocprim::make_transform_iterator(d_count.cget(), MoreThanOnce()), d_repeated_kmers,
                                   d_sel.get() + 1, (size_t)n, s.st);
        }));
        JTK_HIP_TRY(d_runs.download(&h_runs, 1, s.st));
        JTK_HIP_TRY(d_sel.download(h_sel, 1, s.st));
        JTK_HIP_TRY(hipStreamSynchronize(s.st));  // M: the percentile is an f64 expression of it
        const uint64_t m = h_sel[0];
        const uint64_t percentile = (uint64_t)std::floor((double)m * (1.0 - freq));
        if (m) JTK_HIP_TRY(mk_sort<uint32_t>(tmp, d_repeated.cget(), d_ascending, m, 32, s.st));
        verdict_kernel<<<1, 1, 0, s.st>>>(d_ascending, m, percentile, min_count, d_verdict.get());
        if (m)
            JTK_HIP_TRY(tmp.run([&](void *t, size_t &bytes) {
                return rocprim::select(t, bytes, (const Key *)d_repeated_kmers, rocprim::make_transform_iterator(d_repeated.cget(), MoreThan{d_verdict.cget() + 3}),
                                       d_mask, d_sel.get() + 2, (size_t)m, s.st);
            }));
        JTK_HIP_TRY(d_verdict.download(h_verdict, 4, s.st));
    }
    JTK_HIP_TRY(hipEventRecord(s.ev[3], s.st));
    if (R.n_tiles)
        apply_kernel<Key><<<R.n_tiles, MK_THREADS, 0, s.st>>>(R.bases.cget(), R.off.cget(), R.tile_seq.cget(), R.tile_start.cget(), k, d_mask,
                                                              (const unsigned long long *)(d_sel.cget() + 2), d_out.get(), d_lower.get());
    JTK_HIP_TRY(hipEventRecord(late[0], s.st));
    std::vector<uint8_t> h_out(n_bases);
    if (n_bases) JTK_HIP_TRY(d_out.download(h_out.data(), n_bases, s.st));
    JTK_HIP_TRY(d_sel.download(h_sel, 3, s.st));
    JTK_HIP_TRY(d_lower.download(&h_lower, 1, s.st));
    JTK_HIP_TRY(hipStreamSynchronize(s.st));
    JTK_HIP_TRY(hipGetLastError());
    const uint64_t n_mask = h_sel[2];
    std::vector<Key> h_mask;
    if (n_mask && n_mask <= mask_cap && mask_kmers) {
        h_mask.resize(n_mask);
        JTK_HIP_TRY(hipMemcpyAsync(h_mask.data(), d_mask, n_mask * sizeof(Key), hipMemcpyDeviceToHost, s.st));
        JTK_HIP_TRY(hipStreamSynchronize(s.st));
    }
    float ms[4] = {0.f, 0.f, 0.f, 0.f};
    JTK_HIP_TRY(s.elapsed(0, 1, &ms[0]));
    JTK_HIP_TRY(s.elapsed(1, 2, &ms[1]));
    JTK_HIP_TRY(s.elapsed(2, 3, &ms[2]));
    JTK_HIP_TRY(hipEventElapsedTime(&ms[3], s.ev[3], late[0]));
    for (int i = 0; i < 4; i++) g_mask_timing[i] = ms[i];
    if (n_bases) std::memcpy(masked, h_out.data(), n_bases);
    report->n_bases = n_bases;
    report->n_kmers = n;
    report->n_distinct = h_runs;
    report->n_singleton = h_runs - h_sel[0];
    report->n_masked_kmers = n_mask;
    report->n_lower = h_lower;
    report->thr = h_verdict[0];
    report->takes_all = h_verdict[1];
    if (h_verdict[2])
        return jtk_fail(JTK_ERR_CHUNK_FAILED, "no k-mer at the percentile: none is counted twice, or freq is too small (the reference's counts[percentile] panics)");
    if (!mask_kmers) return 0;  // the list is not asked for
    if (n_mask > mask_cap) return jtk_fail(JTK_ERR_INVALID_ARG, "mask_cap is below report->n_masked_kmers");
    for (uint64_t i = 0; i < n_mask; i++) mask_kmers[i] = h_mask[i];
    return 0;
}

template <typename Key>
int mk_repetitive(size_t n_reads, const uint8_t *bases, const uint64_t *read_off, uint32_t k, uint64_t *kmers, uint64_t cap, uint64_t *n_kmers,
                  const KmerPlan &P) {
    const uint64_t n = P.n_kmers;
    *n_kmers = 0;
    if (!n) return 0;
    DevStream s;
    JTK_HIP_TRY(s.create());
    {
        size_t sort_tmp = 0;
        JTK_HIP_TRY(rocprim::radix_sort_keys(nullptr, sort_tmp, (const Key *)nullptr, (Key *)nullptr, (size_t)n, 0u, 2 * k, s.st));
        if (int rc = jtk_fits(DevSeqs::bytes(n_reads, read_off, P, true) + 2 * n * sizeof(Key) + sort_tmp, "the work area")) return rc;
    }
    DevSeqs R;
    if (int rc = R.upload(n_reads, bases, read_off, P, true, s.st)) return rc;
    DevArr<Key> d_raw, d_sorted;
    DevArr<unsigned long long> d_cursor;
    DevArr<size_t> d_unique;
    RocTemp tmp;
    JTK_HIP_TRY(d_raw.alloc(n));
    JTK_HIP_TRY(d_sorted.alloc(n));
    JTK_HIP_TRY(d_cursor.alloc(1));
    JTK_HIP_TRY(d_unique.alloc(1));
    JTK_HIP_TRY(d_cursor.zero(1, s.st));
    emit_kernel<Key><<<R.n_tiles, MK_THREADS, 0, s.st>>>(R.bases.cget(), R.off.cget(), R.kmer_off.cget(), R.tile_seq.cget(), R.tile_start.cget(), k,
                                                        MK_LOWER, nullptr, 0, d_raw.get(), d_cursor.get());
    unsigned long long emitted = 0;
    JTK_HIP_TRY(d_cursor.download(&emitted, 1, s.st));
    JTK_HIP_TRY(hipStreamSynchronize(s.st));  // the sort's size is a host argument
    JTK_HIP_TRY(hipGetLastError());
    if (!emitted) return 0;
    size_t unique = 0;
    JTK_HIP_TRY(mk_sort<Key>(tmp, d_raw.cget(), d_sorted.get(), emitted, 2 * k, s.st));
    JTK_HIP_TRY(tmp.run([&](void *t, size_t &bytes) {
        return rocprim::unique(t, bytes, d_sorted.cget(), d_raw.get(), d_unique.get(), (size_t)emitted, rocprim::equal_to<Key>(), s.st);
    }));
    JTK_HIP_TRY(d_unique.download(&unique, 1, s.st));
    JTK_HIP_TRY(hipStreamSynchronize(s.st));
    *n_kmers = unique;
    if (unique > cap) return jtk_fail(JTK_ERR_INVALID_ARG, "cap is below *n_kmers");
    std::vector<Key> h(unique);
    JTK_HIP_TRY(d_raw.download(h.data(), unique, s.st));
    JTK_HIP_TRY(hipStreamSynchronize(s.st));
    for (size_t i = 0; i < unique; i++) kmers[i] = h[i];
    return 0;
}

}  // namespace

extern "C" void jtk_lc_debug_mask_timing(double *out) {
    if (out) std::memcpy(out, g_mask_timing, sizeof(g_mask_timing));
}

extern "C" int jtk_lc_mask_repeats(size_t n_reads, const uint8_t *bases, const uint64_t *read_off, uint32_t k, double freq, uint32_t min_count,
                                   uint8_t *masked, uint64_t *mask_kmers, uint64_t mask_cap, jtk_mask_report_t *report, int device) {
    g_last_error.clear();
    std::memset(g_mask_timing, 0, sizeof(g_mask_timing));
    if (!report) return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    if (!(freq >= 0.0 && freq <= 1.0)) return jtk_fail(JTK_ERR_INVALID_ARG, "freq is not in [0, 1]");
    if (int rc = mk_check(n_reads, bases, read_off, k, "read_off")) return rc;
    if ((read_off[n_reads] && !masked) || (mask_cap && !mask_kmers)) return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    if (int rc = jtk_require_device(device)) return rc;
    std::memset(report, 0, sizeof(*report));
    const KmerPlan P = mk_plan(n_reads, read_off, k);
    return 2 * k <= 32 ? mk_mask<uint32_t>(n_reads, bases, read_off, k, freq, min_count, masked, mask_kmers, mask_cap, report, P)
                       : mk_mask<uint64_t>(n_reads, bases, read_off, k, freq, min_count, masked, mask_kmers, mask_cap, report, P);
}

extern "C" int jtk_lc_repetitive_kmers(size_t n_reads, const uint8_t *bases, const uint64_t *read_off, uint32_t k, uint64_t *kmers, uint64_t cap,
                                       uint64_t *n_kmers, int device) {
    g_last_error.clear();
    if (!n_kmers || (cap && !kmers)) return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    if (int rc = mk_check(n_reads, bases, read_off, k, "read_off")) return rc;
    if (int rc = jtk_require_device(device)) return rc;
    const KmerPlan P = mk_plan(n_reads, read_off, k);
    return 2 * k <= 32 ? mk_repetitive<uint32_t>(n_reads, bases, read_off, k, kmers, cap, n_kmers, P)
                       : mk_repetitive<uint64_t>(n_reads, bases, read_off, k, kmers, cap, n_kmers, P);
}

extern "C" int jtk_lc_repetitiveness(size_t n_seqs, const uint8_t *bases, const uint64_t *seq_off, uint32_t k, const uint64_t *kmers, uint64_t n_kmers,
                                     uint32_t *rep_num, uint32_t *rep_den, int device) {
    g_last_error.clear();
    if ((n_kmers && !kmers) || (n_seqs && (!rep_num || !rep_den))) return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    if (int rc = mk_check(n_seqs, bases, seq_off, k, "seq_off")) return rc;
    const uint32_t seq_bits = n_seqs > 1 ? jtk_bits(n_seqs - 1) : 0;  // of the largest index
    if (2 * k + seq_bits > 64) return jtk_fail(JTK_ERR_UNSUPPORTED, "the sequence index does not fit above the k-mer in 64 bits");
    if (int rc = jtk_require_device(device)) return rc;
    const KmerPlan P = mk_plan(n_seqs, seq_off, k);
    for (size_t r = 0; r < n_seqs; r++) {
        const uint64_t len = seq_off[r + 1] - seq_off[r];
        rep_num[r] = 0;
        rep_den[r] = (uint32_t)((len > k ? len - k : 0) + 1);
    }
    const uint64_t n = P.n_kmers;
    DevStream s;
    JTK_HIP_TRY(s.create());
    DevArr<uint64_t> d_set;
    DevArr<uint32_t> d_bad;
    if (d_set.upload(kmers, n_kmers, s.st)) return jtk_fail(JTK_ERR_ALLOC, "device upload failed");
    JTK_HIP_TRY(d_bad.alloc(1));
    JTK_HIP_TRY(d_bad.zero(1, s.st));
    ascending_kernel<<<jtk_blocks(n_kmers, 256, 1024), 256, 0, s.st>>>(d_set.cget(), n_kmers, d_bad.get());
    uint32_t bad = 0;
    JTK_HIP_TRY(d_bad.download(&bad, 1, s.st));
    if (!n || !n_kmers) {
        JTK_HIP_TRY(hipStreamSynchronize(s.st));
        return bad ? jtk_fail(JTK_ERR_INVALID_ARG, "kmers is not ascending and unique") : 0;
    }
    const uint32_t end_bit = 2 * k + seq_bits;
    {
        size_t sort_tmp = 0;
        JTK_HIP_TRY(rocprim::radix_sort_keys(nullptr, sort_tmp, (const uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)n, 0u, end_bit, s.st));
        if (int rc = jtk_fits(DevSeqs::bytes(n_seqs, seq_off, P, true) + 3 * n * 8 + n * 4 + sort_tmp + 4 * (uint64_t)n_seqs, "the work area")) return rc;
    }
    DevSeqs R;
    if (int rc = R.upload(n_seqs, bases, seq_off, P, true, s.st)) return rc;
    DevArr<uint64_t> d_raw, d_sorted;
    DevArr<unsigned long long> d_cursor;
    DevArr<uint32_t> d_count, d_runs, d_num;
    RocTemp tmp;
    JTK_HIP_TRY(d_raw.alloc(n));
    JTK_HIP_TRY(d_sorted.alloc(n));
    JTK_HIP_TRY(d_cursor.alloc(1));
    JTK_HIP_TRY(d_count.alloc(n));
    JTK_HIP_TRY(d_runs.alloc(1));
    JTK_HIP_TRY(d_num.alloc(n_seqs));
    JTK_HIP_TRY(d_cursor.zero(1, s.st));
    JTK_HIP_TRY(d_num.zero(n_seqs, s.st));
    emit_kernel<uint64_t><<<R.n_tiles, MK_THREADS, 0, s.st>>>(R.bases.cget(), R.off.cget(), R.kmer_off.cget(), R.tile_seq.cget(), R.tile_start.cget(),
                                                             k, MK_MEMBER, d_set.cget(), n_kmers, d_raw.get(), d_cursor.get());
    unsigned long long emitted = 0;
    JTK_HIP_TRY(d_cursor.download(&emitted, 1, s.st));
    JTK_HIP_TRY(hipStreamSynchronize(s.st));  // the sort's size is a host argument
    JTK_HIP_TRY(hipGetLastError());
    if (bad) return jtk_fail(JTK_ERR_INVALID_ARG, "kmers is not ascending and unique");
    if (!emitted) return 0;
    JTK_HIP_TRY(mk_sort<uint64_t>(tmp, d_raw.cget(), d_sorted.get(), emitted, end_bit, s.st));
    JTK_HIP_TRY(tmp.run([&](void *t, size_t &bytes) {
        return rocprim::run_length_encode(t, bytes, d_sorted.cget(), (unsigned int)emitted, d_raw.get(), d_count.get(), d_runs.get(), s.st);
    }));
    repeated_kernel<<<jtk_blocks(emitted, 256, 2048), 256, 0, s.st>>>(d_raw.cget(), d_count.cget(), d_runs.cget(), k, d_num.get());
    JTK_HIP_TRY(d_num.download(rep_num, n_seqs, s.st));
    JTK_HIP_TRY(hipStreamSynchronize(s.st));
    JTK_HIP_TRY(hipGetLastError());
    return 0;
}
