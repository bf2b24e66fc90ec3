// map.hip -- jtk_lc_map_reads, jtk_lc_sketch: minimizer seeding and chaining of reads onto chunks, the step the reference leaves
// to an external minimap2 process (encode/mod.rs:41-64, :315-355; minimap2.rs).  The specification is this build's own, DESIGN.md
// section 4 "Seeding and chaining"; tests/map_reference.py restates it and the device is held to that bit for bit.
//
//   sketch     one workgroup per tile of MP_TILE k-mer positions of a sequence.  The tile's bases and a halo (w - 1 positions on
//              either side, k - 1 bases behind) are staged in LDS and packed into a 2-bit stream of forward codes and a 1-bit
//              stream "no base"; a lane forms the forward k-mer as a bit field, its reverse complement by a bit reversal, the
//              canonical one, its strand and its hash.  Window minima over w positions in LDS, then per position "the hash equals
//              the minimum of a window that holds it".  Every position belongs to exactly one tile, so a minimizer whose windows
//              straddle a seam comes out once.  Survivors are appended at a cursor, one atomic per workgroup.
//   index      radix sort of the targets' (hash, location) over the 2k hash bits, run lengths = occurrences, their scan.
//   hits       per query minimizer (sorted by location, so a query's hits are contiguous) a binary search into the distinct
//              hashes: count, exclusive scan, ONE wait to size the hit buffer, fill.  A hit is one 64-bit key
//              target << 39 | rev << 38 | (diag + 65,536) << 16 | tpos, the query's index beside it.
//   order      one segmented radix sort, a segment per query: (target, rev, diag, tpos) ascending; q' = diag + tpos follows.
//   chain      a head flag from the left neighbour, a scan for the cluster's index, a wave-segmented min / max reduction by
//              shuffles whose segment ends go to the cluster's record by atomics (a cluster may span waves and workgroups), and
//              the distinct target positions: equal tpos on different diagonals are NOT adjacent in the order above, so
//              (cluster, tpos) is sorted once more and the first of each run counted by ballots.
//   compact    clusters with n_seeds >= min_seeds, by a scan, into the placements.
#include <cstring>
#include <string>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "jtk_lc_debug.h"
#include "kmer_tile.h"
#include "prim_host.h"

namespace {

constexpr uint32_t MP_THREADS = 256;
constexpr uint32_t MP_TILE = 1024;                            // k-mer positions a workgroup owns
constexpr uint32_t MP_MAX_K = 31, MP_MAX_W = 64;
constexpr uint32_t MP_SPAN = MP_TILE + 2 * (MP_MAX_W - 1);    // positions staged at most: the tile and w - 1 on either side
constexpr uint32_t MP_BASES = 1184;                           // bytes staged: MP_SPAN + k - 1 <= 1,180, in whole 32-base words
constexpr uint32_t MP_W2 = MP_BASES / 16, MP_W1 = MP_BASES / 32;
constexpr uint32_t MP_MAX_TLEN = 65535, MP_MAX_QLEN = 4000000, MP_MAX_TARGETS = 1u << 25;
constexpr uint32_t MP_DIAG_BIAS = 65536;                      // diag + bias is in [1, 2^22): tpos <= 65,535, q' <= 4,000,000
constexpr uint64_t MP_NONE = ~0ull;                           // the hash of an invalid k-mer (a hash has 2k <= 62 bits)
constexpr uint64_t MP_C0 = 0x9E3779B97F4A7C15ull, MP_C1 = 0xBF58476D1CE4E5B9ull, MP_C2 = 0x94D049BB133111EBull;
static_assert(MP_SPAN + MP_MAX_K - 1 <= MP_BASES && MP_BASES % 32 == 0, "the staged bytes hold the last k-mer, in whole words");
static_assert(MP_MAX_QLEN + MP_DIAG_BIAS < (1u << 22), "a biased diagonal has 22 bits");

thread_local double g_map_timing[10];  // ms of the six phases; minimizers, hits; ms of the two sketch kernels alone; 0

struct SketchTile {
    uint8_t raw[MP_BASES];
    uint8_t strand[MP_SPAN];
    uint32_t fwd[MP_W2 + 2], bad[MP_W1 + 1];  // each stream and its zero words (kmer_tile.h)
    uint64_t hash[MP_SPAN], wmin[MP_SPAN];
};

// a bijection of [0, 4^k)
__device__ __forceinline__ uint64_t mp_hash(uint64_t x, uint32_t k) {
    const uint64_t m = (1ull << (2 * k)) - 1;
    uint64_t h = (x ^ MP_C0) & m;
    h = (h * MP_C1) & m;
    h ^= h >> k;
    h = (h * MP_C2) & m;
    h ^= h >> k;
    return h;
}

// the reverse complement of a forward k-mer (base i at bits 2i): complement, reverse the 64 bits, put each pair's bits back in
// order, drop the 32 - k groups that were above the k-mer
__device__ __forceinline__ uint64_t mp_revcomp(uint64_t f, uint32_t k) {
    uint64_t x = __brevll(~f);
    x = ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
    return x >> (64 - 2 * k);
}

// One workgroup per tile: the minimizers among the positions tile_start .. tile_start + MP_TILE of sequence tile_seq go to
// (out_hash, out_loc) at *cursor; loc = seq << 32 | pos << 1 | strand.  The arrays hold one entry per k-mer position of the call.
__global__ void __launch_bounds__(MP_THREADS) sketch_kernel(const uint8_t *bases, const uint64_t *seq_off, const uint32_t *tile_seq,
                                                            const uint32_t *tile_start, uint32_t k, uint32_t w, uint64_t *out_hash, uint64_t *out_loc,
                                                            unsigned long long *cursor) {
    __shared__ SketchTile T;
    __shared__ uint64_t s_votes[MP_TILE / 64];
    __shared__ unsigned long long s_first;
    const uint32_t r = tile_seq[blockIdx.x], s = tile_start[blockIdx.x], lane = threadIdx.x & 63u;
    const uint64_t so = seq_off[r];
    const uint32_t len = (uint32_t)(seq_off[r + 1] - so);
    if (len < k) return;
    const uint32_t n = len - k + 1;  // k-mer positions
    if (s >= n) return;
    const uint32_t width = w < n ? w : n;        // of a window; n < w: the one window is all positions
    const uint32_t n_win = n - width + 1;
    const uint32_t a = s >= w - 1 ? s - (w - 1) : 0;                                          // the first position staged
    const uint32_t h_end = n - s > MP_TILE + w - 1 ? s + MP_TILE + w - 1 : n;                 // behind the last
    const uint32_t n_hash = h_end - a;                                                        // <= MP_TILE + 2 w - 2 <= MP_SPAN
    const uint32_t own_end = n - s > MP_TILE ? s + MP_TILE : n;
    const uint32_t win_end = own_end < n_win ? own_end : n_win;                               // windows a .. win_end hold an owned position
    jtk_stage_bytes<MP_BASES, MP_THREADS>(T.raw, bases + so, len, a);
    __syncthreads();
    jtk_pack2<MP_W2, MP_THREADS>({T.fwd}, [&](uint32_t i) { return jtk_base_code(T.raw[i]); });
    jtk_pack1<MP_W1, MP_THREADS>(T.bad, [&](uint32_t i) { return jtk_no_base(T.raw[i]); });
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_hash; i += MP_THREADS) {  // i + k <= MP_SPAN + 30 <= MP_BASES
        const uint64_t f = jtk_field2(T.fwd, i, k);
        const uint32_t no_base = jtk_field1(T.bad, i, k);
        const uint64_t rc = mp_revcomp(f, k);
        const bool valid = !no_base && f != rc;
        T.hash[i] = valid ? mp_hash(f < rc ? f : rc, k) : MP_NONE;
        T.strand[i] = f > rc ? 1 : 0;
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < win_end - a; j += MP_THREADS) {  // window a + j: j + width <= n_hash
        uint64_t m = MP_NONE;
        for (uint32_t t = 0; t < width; t++) m = T.hash[j + t] < m ? T.hash[j + t] : m;
        T.wmin[j] = m;
    }
    __syncthreads();
    // One ballot word per 64 owned positions, then ONE atomic for the workgroup: with an atomic per wave and step the 4.8 million
    // adds to the one cursor of a 300-Mbase call were the kernel's time (57 ms; section 5 of DESIGN.md).
    for (uint32_t word = threadIdx.x >> 6; word < MP_TILE / 64; word += MP_THREADS / 64) {
        const uint32_t p = s + 64 * word + lane;
        bool pass = false;
        if (p < own_end) {
            const uint64_t h = T.hash[p - a];
            if (h != MP_NONE) {  // the windows that hold p: max(p - width + 1, 0) .. min(p, n_win - 1), all of them in a .. win_end
                const uint32_t j_lo = p >= width - 1 ? p - (width - 1) : 0, j_hi = p < n_win - 1 ? p : n_win - 1;
                for (uint32_t j = j_lo; j <= j_hi; j++) pass = pass || T.wmin[j - a] == h;
            }
        }
        const uint64_t votes = __ballot(pass);
        if (lane == 0) s_votes[word] = votes;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
        for (uint32_t word = 0; word < MP_TILE / 64; word++) total += (uint32_t)__popcll(s_votes[word]);
        s_first = total ? atomicAdd(cursor, (unsigned long long)total) : 0ull;
    }
    __syncthreads();
    for (uint32_t word = threadIdx.x >> 6; word < MP_TILE / 64; word += MP_THREADS / 64) {
        const uint64_t votes = s_votes[word];
        if (!((votes >> lane) & 1ull)) continue;
        uint32_t before = (uint32_t)__popcll(votes & ((1ull << lane) - 1));
        for (uint32_t v = 0; v < word; v++) before += (uint32_t)__popcll(s_votes[v]);
        const uint32_t p = s + 64 * word + lane;
        out_hash[s_first + before] = T.hash[p - a];
        out_loc[s_first + before] = ((uint64_t)r << 32) | ((uint64_t)p << 1) | T.strand[p - a];
    }
}

// The index as the hit kernels see it: the targets' locations in hash order, the distinct hashes, their counts and first records.
struct Index {
    const uint64_t *loc, *uniq;
    const uint32_t *count, *first, *n_runs;
    uint32_t max_occ, skip_self;
};

// the run of query minimizer (h, qseq): 0 where the hash is not indexed or occurs more than max_occ times
__device__ __forceinline__ uint32_t mp_run(const Index &X, uint64_t h, uint32_t *first) {
    const uint64_t n = *X.n_runs, at = jtk_lower_bound(X.uniq, n, h);
    if (at >= n || X.uniq[at] != h || X.count[at] > X.max_occ) return 0;
    *first = X.first[at];
    return X.count[at];
}

// count[i] = the hits of query minimizer i; count[n] = 0, so the exclusive scan over n + 1 entries ends with the total
__global__ void count_kernel(Index X, const uint64_t *q_hash, const uint64_t *q_loc, uint64_t n, uint32_t *count) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t c = 0;
        if (i < n) {
            uint32_t first = 0;
            c = mp_run(X, q_hash[i], &first);
            if (c && X.skip_self) {
                const uint32_t self = (uint32_t)(q_loc[i] >> 32);
                uint32_t other = 0;
                for (uint32_t t = 0; t < c; t++) other += (uint32_t)(X.loc[first + t] >> 32) != self;
                c = other;
            }
        }
        count[i] = c;
    }
}

// the hits of query minimizer i at hit_off[i] .. hit_off[i + 1]
__global__ void fill_kernel(Index X, const uint64_t *q_hash, const uint64_t *q_loc, uint64_t n, const uint64_t *hit_off, const uint64_t *query_off,
                            uint32_t k, uint64_t *key, uint32_t *qid) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t at = hit_off[i];
        if (hit_off[i + 1] == at) continue;
        uint32_t first = 0;
        const uint32_t c = mp_run(X, q_hash[i], &first);
        const uint64_t ql = q_loc[i];
        const uint32_t query = (uint32_t)(ql >> 32), q = (uint32_t)(ql & 0xffffffffu) >> 1, q_strand = (uint32_t)ql & 1u;
        const uint32_t qlen = (uint32_t)(query_off[query + 1] - query_off[query]);
        for (uint32_t t = 0; t < c; t++) {
            const uint64_t tl = X.loc[first + t];
            const uint32_t target = (uint32_t)(tl >> 32), tpos = (uint32_t)(tl & 0xffffffffu) >> 1, rev = q_strand ^ ((uint32_t)tl & 1u);
            if (X.skip_self && target == query) continue;
            const uint32_t oq = rev ? qlen - (q + k) : q;
            key[at] = ((uint64_t)target << 39) | ((uint64_t)rev << 38) | ((uint64_t)(oq + MP_DIAG_BIAS - tpos) << 16) | tpos;
            qid[at] = query;
            at++;
        }
    }
}

// seg[q] = the first hit of query q (q = n_queries: the total): the segments of the ordering sort
__global__ void segment_kernel(const uint64_t *q_loc, uint64_t n, const uint64_t *hit_off, uint64_t n_queries, uint32_t *seg) {
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q <= n_queries; q += (uint64_t)gridDim.x * blockDim.x)
        seg[q] = (uint32_t)hit_off[jtk_lower_bound(q_loc, n, q << 32)];
}

__global__ void head_kernel(const uint64_t *key, const uint32_t *qid, uint64_t n, uint32_t max_gap, uint32_t *head) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        bool h = i == 0;
        if (!h) {
            const uint64_t a = key[i - 1], b = key[i];
            h = qid[i - 1] != qid[i] || (a >> 38) != (b >> 38) ||
                (uint64_t)((b >> 16) & 0x3fffffu) - (uint64_t)((a >> 16) & 0x3fffffu) > (uint64_t)max_gap;  // ascending inside (target, rev)
        }
        head[i] = h ? 1u : 0u;
    }
}

// a cluster's record; the minima start at ~0, the maxima at 0
struct Clusters {
    uint32_t *head, *tmin, *tmax, *qmin, *qmax, *dlo, *dhi, *seeds;
};

__global__ void cluster_init_kernel(Clusters C, uint64_t n) {
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (uint64_t)gridDim.x * blockDim.x) {
        C.head[c] = C.tmin[c] = C.qmin[c] = C.dlo[c] = 0xffffffffu;
        C.tmax[c] = C.qmax[c] = C.dhi[c] = C.seeds[c] = 0;
    }
}

// Hit i belongs to cluster incl[i] - 1.  The lanes of a wave that share a cluster are adjacent: an inclusive segmented scan by
// shuffles leaves the segment's min / max in its last lane, which hands them to the cluster's record -- by atomics, because the
// cluster may go on in the next wave or workgroup.  seed_key[i] = cluster << 16 | tpos for the count of distinct positions.
__global__ void __launch_bounds__(256) reduce_kernel(const uint64_t *key, const uint32_t *incl, uint64_t n, Clusters C, uint64_t *seed_key) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n; base += (uint64_t)gridDim.x * blockDim.x) {  // (whole waves step together)
        const uint64_t i = base + threadIdx.x;
        const bool live = i < n;
        uint32_t c = 0xffffffffu, tlo = 0, thi = 0, qlo = 0, qhi = 0, dlo = 0, dhi = 0, first = 0;
        if (live) {
            const uint64_t kk = key[i];
            c = incl[i] - 1;
            tlo = thi = (uint32_t)(kk & 0xffffu);
            dlo = dhi = (uint32_t)(kk >> 16) & 0x3fffffu;
            qlo = qhi = dlo - MP_DIAG_BIAS + tlo;  // q' = diag + tpos
            first = (uint32_t)i;
            seed_key[i] = ((uint64_t)c << 16) | tlo;
        }
#pragma unroll
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const uint32_t oc = __shfl_up(c, o, 64);
            const uint32_t a0 = __shfl_up(tlo, o, 64), a1 = __shfl_up(thi, o, 64), a2 = __shfl_up(qlo, o, 64), a3 = __shfl_up(qhi, o, 64);
            const uint32_t a4 = __shfl_up(dlo, o, 64), a5 = __shfl_up(dhi, o, 64), a6 = __shfl_up(first, o, 64);
            if (lane >= o && oc == c) {
                tlo = a0 < tlo ? a0 : tlo;
                thi = a1 > thi ? a1 : thi;
                qlo = a2 < qlo ? a2 : qlo;
                qhi = a3 > qhi ? a3 : qhi;
                dlo = a4 < dlo ? a4 : dlo;
                dhi = a5 > dhi ? a5 : dhi;
                first = a6 < first ? a6 : first;
            }
        }
        const uint32_t next = __shfl_down(c, 1, 64);
        if (live && (lane == 63 || next != c)) {
            atomicMin(&C.head[c], first);
            atomicMin(&C.tmin[c], tlo);
            atomicMax(&C.tmax[c], thi);
            atomicMin(&C.qmin[c], qlo);
            atomicMax(&C.qmax[c], qhi);
            atomicMin(&C.dlo[c], dlo);
            atomicMax(&C.dhi[c], dhi);
        }
    }
}

// sorted (cluster, tpos): the first of each run is a distinct target position of its cluster.  Per wave, one ballot of the firsts
// and one of the lanes where a cluster begins; the last lane of a cluster's stretch adds the firsts inside the stretch.
__global__ void __launch_bounds__(256) seeds_kernel(const uint64_t *seed_key, uint64_t n, uint32_t *seeds) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n; base += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = base + threadIdx.x;
        const bool live = i < n;
        const uint64_t kk = live ? seed_key[i] : MP_NONE;
        const uint32_t c = live ? (uint32_t)(kk >> 16) : 0xffffffffu;
        const bool fresh = live && (i == 0 || seed_key[i - 1] != kk);
        const uint32_t prev = __shfl_up(c, 1, 64), next = __shfl_down(c, 1, 64);
        const uint64_t fresh_mask = __ballot(fresh), begin_mask = __ballot(lane == 0 || prev != c);
        if (live && (lane == 63 || next != c)) {
            const uint64_t upto = lane == 63 ? ~0ull : (2ull << lane) - 1;
            const uint32_t begin = 63u - (uint32_t)__clzll((long long)(begin_mask & upto));
            const uint32_t cnt = (uint32_t)__popcll(fresh_mask & upto & ~((1ull << begin) - 1));
            if (cnt) atomicAdd(&seeds[c], cnt);
        }
    }
}

// flag[c] = the cluster is reported; flag[n] = 0, so the exclusive scan over n + 1 entries ends with the number of placements
__global__ void report_kernel(const uint32_t *seeds, uint64_t n, uint32_t min_seeds, uint32_t *flag) {
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c <= n; c += (uint64_t)gridDim.x * blockDim.x)
        flag[c] = c < n && seeds[c] >= min_seeds ? 1u : 0u;
}

__global__ void place_kernel(Clusters C, uint64_t n, const uint32_t *slot, const uint64_t *key, const uint32_t *qid, const uint64_t *query_off, uint32_t k,
                             jtk_map_placement_t *out) {
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (uint64_t)gridDim.x * blockDim.x) {
        if (slot[c + 1] == slot[c]) continue;
        const uint32_t hd = C.head[c], query = qid[hd];
        const uint64_t kk = key[hd];
        const uint32_t rev = (uint32_t)(kk >> 38) & 1u, qlen = (uint32_t)(query_off[query + 1] - query_off[query]);
        jtk_map_placement_t p;
        p.query = query;
        p.target = (uint32_t)(kk >> 39);
        p.is_forward = rev ? 0u : 1u;
        p.n_seeds = C.seeds[c];
        p.oq_start = C.qmin[c];
        p.oq_end = C.qmax[c] + k;
        p.qstart = rev ? qlen - p.oq_end : p.oq_start;
        p.qend = rev ? qlen - p.oq_start : p.oq_end;
        p.tstart = C.tmin[c];
        p.tend = C.tmax[c] + k;
        p.diag_lo = (int32_t)C.dlo[c] - (int32_t)MP_DIAG_BIAS;
        p.diag_hi = (int32_t)C.dhi[c] - (int32_t)MP_DIAG_BIAS;
        out[slot[c]] = p;
    }
}

// ---- the host side

int mp_check_seqs(size_t n, const uint8_t *bases, const uint64_t *off, const char *what) {
    if (int rc = jtk_check_offsets(n, off, what)) return rc;
    if (off[n] && !bases) return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    return 0;
}

int mp_check_limits(size_t n, const uint64_t *off, uint64_t max_len, const char *what) {
    if (off[n] >> 32 || (uint64_t)n >> 32) return jtk_fail(JTK_ERR_UNSUPPORTED, std::string("2^32 bases or sequences, or more, in ") + what);
    for (size_t i = 0; i < n; i++)
        if (off[i + 1] - off[i] > max_len)
            return jtk_fail(JTK_ERR_UNSUPPORTED, std::string(what) + ": a sequence of " + std::to_string(off[i + 1] - off[i]) + " bases, above " +
                                                     std::to_string(max_len));
    return 0;
}

int mp_check_kw(uint32_t k, uint32_t w) {
    if (k == 0) return jtk_fail(JTK_ERR_INVALID_ARG, "k is 0");
    if (w == 0) return jtk_fail(JTK_ERR_INVALID_ARG, "w is 0");
    return 0;
}

int mp_check_kw_limits(uint32_t k, uint32_t w) {
    if (k > MP_MAX_K) return jtk_fail(JTK_ERR_UNSUPPORTED, "k is above 31");
    if (w > MP_MAX_W) return jtk_fail(JTK_ERR_UNSUPPORTED, "w is above 64");
    return 0;
}

// A set of sequences on the device and its minimizers: (hash, loc) as the sketch kernel appended them.
struct Sketch {
    DevSeqs seqs;  // (no kmer_off: the minimizers are appended at a cursor)
    DevArr<uint64_t> hash, loc;
    uint64_t n = 0;
    size_t n_seqs = 0;
    float kernel_ms = 0.f;  // the sketch kernel alone (run()'s events)

    int run(size_t n_seqs_, const uint8_t *h_bases, const uint64_t *h_off, uint32_t k, uint32_t w, hipStream_t st) {
        n_seqs = n_seqs_;
        const KmerPlan P = jtk_plan_kmers(n_seqs, h_off, k, MP_TILE, KMER_TILE_POSITIONS);
        if (int rc = jtk_fits(DevSeqs::bytes(n_seqs, h_off, P, false) + 16 * P.n_kmers, "the sketch")) return rc;
        DevArr<unsigned long long> d_cursor;
        if (int rc = seqs.upload(n_seqs, h_bases, h_off, P, false, st)) return rc;
        JTK_HIP_TRY(hash.alloc(P.n_kmers));
        JTK_HIP_TRY(loc.alloc(P.n_kmers));
        JTK_HIP_TRY(d_cursor.alloc(1));
        JTK_HIP_TRY(d_cursor.zero(1, st));
        DevEvents around;
        JTK_HIP_TRY(around.create(2));
        JTK_HIP_TRY(hipEventRecord(around[0], st));
        if (seqs.n_tiles)
            sketch_kernel<<<seqs.n_tiles, MP_THREADS, 0, st>>>(seqs.bases.cget(), seqs.off.cget(), seqs.tile_seq.cget(), seqs.tile_start.cget(), k, w,
                                                             hash.get(), loc.get(), d_cursor.get());
        JTK_HIP_TRY(hipEventRecord(around[1], st));
        unsigned long long emitted = 0;
        JTK_HIP_TRY(d_cursor.download(&emitted, 1, st));
        JTK_HIP_TRY(hipStreamSynchronize(st));  // a sort's size is a host argument (and the plan's host arrays live until here)
        JTK_HIP_TRY(hipGetLastError());
        JTK_HIP_TRY(around.elapsed(0, 1, &kernel_ms));
        n = emitted;
        return 0;
    }

    // the pairs by ascending `by` (hash: over its 2k bits; loc: over the sequence's index and the position)
    int sort(bool by_loc, uint32_t k, RocTemp &tmp, hipStream_t st) {
        if (!n) return 0;
        DevArr<uint64_t> h2, l2;
        JTK_HIP_TRY(h2.alloc(n));
        JTK_HIP_TRY(l2.alloc(n));
        if (by_loc) {
            const uint32_t end_bit = 32 + jtk_bits(n_seqs ? n_seqs - 1 : 0);
            JTK_HIP_TRY(tmp.run([&](void *t, size_t &bytes) {
                return rocprim::radix_sort_pairs(t, bytes, loc.cget(), l2.get(), hash.cget(), h2.get(), (size_t)n, 0u, end_bit, st);
            }));
        } else {
            JTK_HIP_TRY(tmp.run([&](void *t, size_t &bytes) {
                return rocprim::radix_sort_pairs(t, bytes, hash.cget(), h2.get(), loc.cget(), l2.get(), (size_t)n, 0u, 2 * k, st);
            }));
        }
        JTK_HIP_TRY(hipStreamSynchronize(st));  // the unsorted blocks are freed below
        std::swap(hash.buf.p, h2.buf.p);
        std::swap(loc.buf.p, l2.buf.p);
        return 0;
    }
};

int mp_map(size_t n_targets, const uint8_t *target_bases, const uint64_t *target_off, size_t n_queries, const uint8_t *query_bases,
           const uint64_t *query_off, const jtk_map_params_t &P, jtk_map_placement_t *out, uint64_t cap, uint64_t *n_placements) {
    const uint32_t k = P.k;
    DevStream s;
    JTK_HIP_TRY(s.create(4));
    DevEvents late;
    JTK_HIP_TRY(late.create(3));
    RocTemp tmp;
    Sketch T, Q;
    *n_placements = 0;
    JTK_HIP_TRY(hipEventRecord(s.ev[0], s.st));
    if (int rc = T.run(n_targets, target_bases, target_off, k, P.w, s.st)) return rc;
    if (int rc = Q.run(n_queries, query_bases, query_off, k, P.w, s.st)) return rc;
    g_map_timing[6] = (double)(T.n + Q.n);
    g_map_timing[8] = (double)T.kernel_ms + (double)Q.kernel_ms;
    JTK_HIP_TRY(hipEventRecord(s.ev[1], s.st));
    if (!T.n || !Q.n) return 0;
    if (T.n >> 32) return jtk_fail(JTK_ERR_UNSUPPORTED, "2^32 minimizers or more in the index");
    // ---- the index: the targets' records in hash order, the distinct hashes, how often each occurs and where its run begins
    if (int rc = T.sort(false, k, tmp, s.st)) return rc;
    if (int rc = Q.sort(true, k, tmp, s.st)) return rc;
    DevArr<uint64_t> d_uniq;
    DevArr<uint32_t> d_count, d_first, d_runs;
    JTK_HIP_TRY(d_uniq.alloc(T.n));
    JTK_HIP_TRY(d_count.alloc(T.n));
    JTK_HIP_TRY(d_first.alloc(T.n));
    JTK_HIP_TRY(d_runs.alloc(1));
    JTK_HIP_TRY(d_count.zero(T.n, s.st));  // the entries behind the runs are no hash's count
    JTK_HIP_TRY(tmp.run([&](void *t, size_t &bytes) {
        return rocprim::run_length_encode(t, bytes, T.hash.cget(), (unsigned int)T.n, d_uniq.get(), d_count.get(), d_runs.get(), s.st);
    }));
    JTK_HIP_TRY(tmp.run([&](void *t, size_t &bytes) {
        return rocprim::exclusive_scan(t, bytes, d_count.cget(), d_first.get(), 0u, (size_t)T.n, rocprim::plus<uint32_t>(), s.st);
    }));
    JTK_HIP_TRY(hipEventRecord(s.ev[2], s.st));
    // ---- the hits
    const Index X{T.loc.cget(), d_uniq.cget(), d_count.cget(), d_first.cget(), d_runs.cget(), P.max_occ, P.skip_self ? 1u : 0u};
    DevArr<uint32_t> d_qcount;
    DevArr<uint64_t> d_hit_off, d_query_off;
    JTK_HIP_TRY(d_qcount.alloc(Q.n + 1));
    JTK_HIP_TRY(d_hit_off.alloc(Q.n + 1));
    count_kernel<<<jtk_blocks(Q.n + 1, 256, 4096), 256, 0, s.st>>>(X, Q.hash.cget(), Q.loc.cget(), Q.n, d_qcount.get());
    JTK_HIP_TRY(tmp.run([&](void *t, size_t &bytes) {
        return rocprim::exclusive_scan(t, bytes, d_qcount.cget(), d_hit_off.get(), (uint64_t)0, (size_t)(Q.n + 1), rocprim::plus<uint64_t>(), s.st);
    }));
    uint64_t n_hits = 0;
    JTK_HIP_TRY(d_hit_off.download(&n_hits, 1, s.st, Q.n));
    JTK_HIP_TRY(hipStreamSynchronize(s.st));  // the one wait the hits need: their number sizes the buffer
    JTK_HIP_TRY(hipGetLastError());
    g_map_timing[7] = (double)n_hits;
    if (!n_hits) return 0;
    if (n_hits >> 32) return jtk_fail(JTK_ERR_UNSUPPORTED, std::to_string(n_hits) + " hits: 2^32 or more (lower max_occ)");
    const uint32_t key_bits = 39 + jtk_bits(n_targets - 1);
    {  // keys twice, the queries' indices, the head flags and their scan, the (cluster, tpos) keys twice, rocprim's blocks
        size_t seg_tmp = 0, sort_tmp = 0;
        JTK_HIP_TRY(rocprim::segmented_radix_sort_keys(nullptr, seg_tmp, (const uint64_t *)nullptr, (uint64_t *)nullptr, (unsigned int)n_hits,
                                                       (unsigned int)n_queries, (const uint32_t *)nullptr, (const uint32_t *)nullptr, 0u, key_bits, s.st));
        JTK_HIP_TRY(rocprim::radix_sort_keys(nullptr, sort_tmp, (const uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)n_hits, 0u, 48u, s.st));
        if (int rc = jtk_fits(n_hits * 44 + seg_tmp + sort_tmp + 4 * (uint64_t)(n_queries + 1), "the hit buffer")) return rc;
    }
    DevArr<uint64_t> d_key, d_sorted, d_seed_key, d_seed_sorted;
    DevArr<uint32_t> d_qid, d_seg, d_head, d_incl;
    JTK_HIP_TRY(d_key.alloc(n_hits));
    JTK_HIP_TRY(d_sorted.alloc(n_hits));
    JTK_HIP_TRY(d_qid.alloc(n_hits));
    JTK_HIP_TRY(d_seg.alloc(n_queries + 1));
    if (d_query_off.upload(query_off, n_queries + 1, s.st)) return jtk_fail(JTK_ERR_ALLOC, "device upload failed");
    fill_kernel<<<jtk_blocks(Q.n, 256, 4096), 256, 0, s.st>>>(X, Q.hash.cget(), Q.loc.cget(), Q.n, d_hit_off.cget(), d_query_off.cget(), k, d_key.get(),
                                                             d_qid.get());
    segment_kernel<<<jtk_blocks(n_queries + 1, 256, 1024), 256, 0, s.st>>>(Q.loc.cget(), Q.n, d_hit_off.cget(), n_queries, d_seg.get());
    JTK_HIP_TRY(hipEventRecord(s.ev[3], s.st));
    // ---- the order inside every query
    JTK_HIP_TRY(tmp.run([&](void *t, size_t &bytes) {
        return rocprim::segmented_radix_sort_keys(t, bytes, d_key.cget(), d_sorted.get(), (unsigned int)n_hits, (unsigned int)n_queries, d_seg.cget(),
                                                  d_seg.cget() + 1, 0u, key_bits, s.st);
    }));
    JTK_HIP_TRY(hipEventRecord(late[0], s.st));
    // ---- the clusters
    JTK_HIP_TRY(d_head.alloc(n_hits));
    JTK_HIP_TRY(d_incl.alloc(n_hits));
    head_kernel<<<jtk_blocks(n_hits, 256, 4096), 256, 0, s.st>>>(d_sorted.cget(), d_qid.cget(), n_hits, P.max_gap, d_head.get());
    JTK_HIP_TRY(tmp.run([&](void *t, size_t &bytes) {
        return rocprim::inclusive_scan(t, bytes, d_head.cget(), d_incl.get(), (size_t)n_hits, rocprim::plus<uint32_t>(), s.st);
    }));
    uint32_t n_clusters = 0;
    JTK_HIP_TRY(d_incl.download(&n_clusters, 1, s.st, n_hits - 1));
    JTK_HIP_TRY(hipStreamSynchronize(s.st));  // the clusters' records are sized by their number
    JTK_HIP_TRY(hipGetLastError());
    DevArr<uint32_t> d_cl[8], d_flag, d_slot;
    for (auto &a : d_cl) JTK_HIP_TRY(a.alloc(n_clusters));
    JTK_HIP_TRY(d_flag.alloc((uint64_t)n_clusters + 1));
    JTK_HIP_TRY(d_slot.alloc((uint64_t)n_clusters + 1));
    JTK_HIP_TRY(d_seed_key.alloc(n_hits));
    JTK_HIP_TRY(d_seed_sorted.alloc(n_hits));
    const Clusters C{d_cl[0].get(), d_cl[1].get(), d_cl[2].get(), d_cl[3].get(), d_cl[4].get(), d_cl[5].get(), d_cl[6].get(), d_cl[7].get()};
    cluster_init_kernel<<<jtk_blocks(n_clusters, 256, 4096), 256, 0, s.st>>>(C, n_clusters);
    reduce_kernel<<<jtk_blocks(n_hits, 256, 4096), 256, 0, s.st>>>(d_sorted.cget(), d_incl.cget(), n_hits, C, d_seed_key.get());
    JTK_HIP_TRY(tmp.run([&](void *t, size_t &bytes) {
        return rocprim::radix_sort_keys(t, bytes, d_seed_key.cget(), d_seed_sorted.get(), (size_t)n_hits, 0u, 16 + jtk_bits(n_clusters - 1), s.st);
    }));
    seeds_kernel<<<jtk_blocks(n_hits, 256, 4096), 256, 0, s.st>>>(d_seed_sorted.cget(), n_hits, C.seeds);
    JTK_HIP_TRY(hipEventRecord(late[1], s.st));
    // ---- the placements
    report_kernel<<<jtk_blocks((uint64_t)n_clusters + 1, 256, 4096), 256, 0, s.st>>>(C.seeds, n_clusters, P.min_seeds, d_flag.get());
    JTK_HIP_TRY(tmp.run([&](void *t, size_t &bytes) {
        return rocprim::exclusive_scan(t, bytes, d_flag.cget(), d_slot.get(), 0u, (size_t)n_clusters + 1, rocprim::plus<uint32_t>(), s.st);
    }));
    uint32_t n_out = 0;
    JTK_HIP_TRY(d_slot.download(&n_out, 1, s.st, n_clusters));
    JTK_HIP_TRY(hipStreamSynchronize(s.st));
    JTK_HIP_TRY(hipGetLastError());
    *n_placements = n_out;
    if (n_out > cap) return jtk_fail(JTK_ERR_INVALID_ARG, "cap is below *n_placements");
    if (n_out) {
        DevArr<jtk_map_placement_t> d_out;
        JTK_HIP_TRY(d_out.alloc(n_out));
        place_kernel<<<jtk_blocks(n_clusters, 256, 4096), 256, 0, s.st>>>(C, n_clusters, d_slot.cget(), d_sorted.cget(), d_qid.cget(), d_query_off.cget(), k,
                                                                         d_out.get());
        JTK_HIP_TRY(d_out.download(out, n_out, s.st));
    }
    JTK_HIP_TRY(hipEventRecord(late[2], s.st));
    JTK_HIP_TRY(hipStreamSynchronize(s.st));
    JTK_HIP_TRY(hipGetLastError());
    float ms[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    JTK_HIP_TRY(s.elapsed(0, 1, &ms[0]));
    JTK_HIP_TRY(s.elapsed(1, 2, &ms[1]));
    JTK_HIP_TRY(s.elapsed(2, 3, &ms[2]));
    JTK_HIP_TRY(hipEventElapsedTime(&ms[3], s.ev[3], late[0]));
    JTK_HIP_TRY(late.elapsed(0, 1, &ms[4]));
    JTK_HIP_TRY(late.elapsed(1, 2, &ms[5]));
    for (int i = 0; i < 6; i++) g_map_timing[i] = ms[i];
    return 0;
}

}  // namespace

extern "C" void jtk_lc_debug_map_timing(double *out) {
    if (out) std::memcpy(out, g_map_timing, sizeof(g_map_timing));
}

extern "C" int jtk_lc_map_reads(size_t n_targets, const uint8_t *target_bases, const uint64_t *target_off, size_t n_queries,
                                const uint8_t *query_bases, const uint64_t *query_off, const jtk_map_params_t *params, jtk_map_placement_t *out,
                                uint64_t cap, uint64_t *n_placements, int device) {
    g_last_error.clear();
    std::memset(g_map_timing, 0, sizeof(g_map_timing));
    if (!target_off || !query_off || !params || !n_placements || (cap && !out)) return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    if (int rc = mp_check_kw(params->k, params->w)) return rc;
    if (params->min_seeds == 0) return jtk_fail(JTK_ERR_INVALID_ARG, "min_seeds is 0");
    if (int rc = mp_check_seqs(n_targets, target_bases, target_off, "target_off")) return rc;
    if (int rc = mp_check_seqs(n_queries, query_bases, query_off, "query_off")) return rc;
    if (int rc = mp_check_kw_limits(params->k, params->w)) return rc;
    if (n_targets > MP_MAX_TARGETS) return jtk_fail(JTK_ERR_UNSUPPORTED, "more than 2^25 targets");
    if (int rc = mp_check_limits(n_targets, target_off, MP_MAX_TLEN, "targets")) return rc;
    if (int rc = mp_check_limits(n_queries, query_off, MP_MAX_QLEN, "queries")) return rc;
    if (int rc = jtk_require_device(device)) return rc;
    if (!n_targets || !n_queries) {
        *n_placements = 0;
        return 0;
    }
    return mp_map(n_targets, target_bases, target_off, n_queries, query_bases, query_off, *params, out, cap, n_placements);
}

extern "C" int jtk_lc_sketch(size_t n_seqs, const uint8_t *bases, const uint64_t *seq_off, uint32_t k, uint32_t w, uint64_t *hash, uint32_t *seq,
                             uint32_t *pos, uint8_t *strand, uint64_t cap, uint64_t *n, int device) {
    g_last_error.clear();
    if (!seq_off || !n || (cap && (!hash || !seq || !pos || !strand))) return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    if (int rc = mp_check_kw(k, w)) return rc;
    if (int rc = mp_check_seqs(n_seqs, bases, seq_off, "seq_off")) return rc;
    if (int rc = mp_check_kw_limits(k, w)) return rc;
    if (int rc = mp_check_limits(n_seqs, seq_off, (1ull << 31) - 1, "sequences")) return rc;
    if (int rc = jtk_require_device(device)) return rc;
    *n = 0;
    if (!n_seqs) return 0;
    DevStream s;
    JTK_HIP_TRY(s.create());
    RocTemp tmp;
    Sketch S;
    if (int rc = S.run(n_seqs, bases, seq_off, k, w, s.st)) return rc;
    *n = S.n;
    if (S.n > cap) return jtk_fail(JTK_ERR_INVALID_ARG, "cap is below *n");
    if (!S.n) return 0;
    if (int rc = S.sort(true, k, tmp, s.st)) return rc;
    std::vector<uint64_t> h_loc(S.n);
    JTK_HIP_TRY(S.hash.download(hash, S.n, s.st));
    JTK_HIP_TRY(S.loc.download(h_loc.data(), S.n, s.st));
    JTK_HIP_TRY(hipStreamSynchronize(s.st));
    JTK_HIP_TRY(hipGetLastError());
    for (uint64_t i = 0; i < S.n; i++) {
        seq[i] = (uint32_t)(h_loc[i] >> 32);
        pos[i] = (uint32_t)(h_loc[i] & 0xffffffffu) >> 1;
        strand[i] = (uint8_t)(h_loc[i] & 1u);
    }
    return 0;
}
