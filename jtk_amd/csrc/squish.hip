// squish.hip -- jtk_lc_squish_clusters / jtk_lc_squish_classify: the step JTK runs in front of the correction.
//
// Replaces `SquishErroneousClusters::squish_erroneous_clusters` (haplotyper/src/squish_erroneous_clusters.rs:44-60):
//   pair counts (:80-90)      every position pair i < j of biased nodes of a read adds 1 to (min chunk, max chunk)
//   retain (:96-97)           count_thr < count, then both chunks with 1 < cluster_num
//   check_correl (:213-252)   per surviving pair the adjusted Rand index (misc.rs:22-46) of the reads' minimum clusters
//   classify (:254-365)       a 0/1 labelling of the relationship graph: 10 x (one greedy sweep + 1,000 Metropolis proposals)
//   classes (:137-165)        Stiff / Suspicious / Isolated per chunk; Suspicious chunks collapse to one cluster (:45-59)
// On the device: the biased flags, per read its distinct biased chunks (multiplicity, minimum cluster) and from those one
// record per chunk pair of the read, a radix sort of the records by pair, the segment sums with both retains, and one
// contingency table per surviving pair in LDS with the index in 64-bit integers.  check_correl walks every node of every read
// once per pair in the reference; here a pair reads its own run of records.  classify is one sequential random stream over a
// graph of a few thousand edges: it runs on the host (the same code jtk_lc_squish_classify exports).
//
// The reference's pair list comes out of a HashMap under par_iter, so its node numbering (and with it sweep order, proposal
// targets and summation order) differs from process to process.  This file fixes one admissible order: pairs ascending by
// (u1, u2) -- the order the sort leaves them in.
#include <algorithm>
#include <cstring>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "device_common.h"
#include "prim_host.h"

namespace {

constexpr uint32_t SQ_NONE = 0xffffffffu;   // bkey of a node that is not biased; rank_k of a chunk id outside chunks[]
constexpr uint32_t SQ_MAX_LABEL = 64;       // the table is SQ_MAX_LABEL x SQ_MAX_LABEL counters
constexpr uint32_t SQ_READ_NODES = 65535;   // nodes per read: multiplicities are 16-bit, their products 32-bit
constexpr uint32_t SQ_READ_GRID = 1024;     // workgroups of the two per-read kernels (they loop over the reads)
constexpr uint32_t SQ_TABLE_GRID = 1024;    // workgroups of the table kernel (they loop over the surviving pairs)
constexpr int SQ_FLAG_PANIC = 1, SQ_FLAG_LABEL = 2;

// a record's value: count in bits 0-31, the minimum cluster of the smaller / larger chunk id (capped at 64) in bits 32-39 /
// 40-47, bit 48 = some biased node of either chunk in this read carries a cluster >= 64
__device__ __forceinline__ uint64_t sq_value(uint32_t count, uint32_t c_lo, uint32_t c_hi, uint32_t big) {
    return (uint64_t)count | ((uint64_t)c_lo << 32) | ((uint64_t)c_hi << 40) | ((uint64_t)big << 48);
}

// Node::is_biased(0.2), definitions/src/lib.rs:703-709 -> the node's chunk rank where biased, SQ_NONE otherwise
__global__ void biased_kernel(uint64_t n_nodes, const jtk_cc_node_t *nodes, const double *post, const uint32_t *rank, uint32_t *bkey) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_nodes; e += stride) {
        const uint32_t len = nodes[e].post_len;
        bool biased = len <= 1;
        if (!biased) {
            const double thr = 1.0 / (double)len + 0.2;
            const double *p = post + nodes[e].post_off;
            for (uint32_t q = 0; q < len && !biased; q++) biased = thr <= jtk_exp(p[q]);
        }
        bkey[e] = biased ? rank[e] : SQ_NONE;
    }
}

// One workgroup per read (looping over the reads): the distinct biased chunks of the read, packed to the front of the read's
// slice of `reps` in no particular order -- x = rank, y = multiplicity | minimum cluster << 16 | (a cluster >= 64) << 24 --
// their number, and the number of records the read will emit (every unordered pair of them, each with itself included).
__global__ void __launch_bounds__(256) distinct_kernel(uint32_t n_reads, const uint64_t *node_off, const jtk_cc_node_t *nodes,
                                                       const uint32_t *bkey, uint2 *reps, uint32_t *n_distinct, uint64_t *n_rec) {
    __shared__ uint32_t s_d;
    for (uint32_t r = blockIdx.x; r < n_reads; r += gridDim.x) {
        const uint64_t off = node_off[r];
        const uint32_t n = (uint32_t)(node_off[r + 1] - off);
        if (threadIdx.x == 0) s_d = 0;
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
            const uint32_t k = bkey[off + i];
            if (k == SQ_NONE) continue;
            bool first = true;
            for (uint32_t j = 0; j < i && first; j++) first = bkey[off + j] != k;
            if (!first) continue;
            uint32_t m = 0, minc = SQ_MAX_LABEL, big = 0;
            for (uint32_t j = i; j < n; j++)
                if (bkey[off + j] == k) {
                    const uint64_t c = nodes[off + j].cluster;
                    m++;
                    if (c >= SQ_MAX_LABEL) big = 1;
                    else if ((uint32_t)c < minc) minc = (uint32_t)c;
                }
            const uint32_t slot = atomicAdd(&s_d, 1u);  // slot < n: at most one per node
            reps[off + slot] = make_uint2(k, m | (minc << 16) | (big << 24));
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            n_distinct[r] = s_d;
            n_rec[r] = (uint64_t)s_d * (s_d + 1) / 2;
        }
        __syncthreads();
    }
}

// One wave per read: record (a, b), a <= b in the read's list, at rec_off[r] + a * d - a (a - 1) / 2 + (b - a).
// count = m_a m_b, or m (m - 1) / 2 for a chunk with itself (0 for a single node: the record still carries the read's
// observation of the (u, u) pair, :220-235).
__global__ void __launch_bounds__(64) emit_kernel(uint32_t n_reads, const uint64_t *node_off, const uint2 *reps, const uint32_t *n_distinct,
                                                  const uint64_t *rec_off, uint64_t n_ranks, uint64_t *keys, uint64_t *vals) {
    for (uint32_t r = blockIdx.x; r < n_reads; r += gridDim.x) {
        const uint2 *rp = reps + node_off[r];
        const uint64_t d = n_distinct[r], base = rec_off[r];
        for (uint64_t a = 0; a < d; a++) {
            const uint2 A = rp[a];
            const uint64_t row = base + a * d - a * (a - 1) / 2;  // (a = 0: the wrapped factor meets a zero)
            for (uint64_t b = a + threadIdx.x; b < d; b += 64) {
                const uint2 B = rp[b];
                const uint2 lo = A.x <= B.x ? A : B, hi = A.x <= B.x ? B : A;
                const uint32_t m_lo = lo.y & 0xffffu, m_hi = hi.y & 0xffffu;
                const uint32_t count = a == b ? m_lo * (m_lo - 1) / 2 : m_lo * m_hi;
                keys[row + (b - a)] = (uint64_t)lo.x * n_ranks + hi.x;
                vals[row + (b - a)] = sq_value(count, (lo.y >> 16) & 0xffu, (hi.y >> 16) & 0xffu, ((lo.y | hi.y) >> 24) & 1u);
            }
        }
    }
}

// head[i] = 1 where a run of equal keys starts (head has n_rec + 1 entries, the last one stays 0)
__global__ void head_kernel(uint64_t n_rec, const uint64_t *keys, uint32_t *head) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_rec; i += stride)
        head[i] = i == 0 || keys[i] != keys[i - 1];
}
__global__ void seg_start_kernel(uint64_t n_rec, uint32_t n_segs, const uint32_t *head, const uint32_t *seg_of, uint32_t *seg_start) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_rec; i += stride) {
        if (head[i]) seg_start[seg_of[i]] = (uint32_t)i;
        if (i == 0) seg_start[n_segs] = (uint32_t)n_rec;
    }
}

// One wave per run: its count, then the two retains of :96-97 (`1 < chunks[u1] && 1 < chunks[u2]` indexes u2 only when u1
// passes; indexing a chunk id that is not in chunks[] is the reference's panic)
__global__ void __launch_bounds__(256) retain_kernel(uint32_t n_segs, const uint32_t *seg_start, const uint64_t *keys, const uint64_t *vals,
                                                     uint64_t n_ranks, const uint32_t *rank_k, uint64_t count_thr, uint32_t *survive,
                                                     int *flags) {
    const uint32_t lane = threadIdx.x & 63u, wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t s = wave; s < n_segs; s += n_waves) {
        const uint32_t b = seg_start[s], e = seg_start[s + 1];
        unsigned long long sum = 0;
        for (uint32_t i = b + lane; i < e; i += 64) sum += vals[i] & 0xffffffffull;
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o, 64);
        if (lane == 0) {
            bool keep = count_thr < sum;
            if (keep) {
                const uint64_t key = keys[b];
                const uint32_t k1 = rank_k[key / n_ranks];
                if (k1 == SQ_NONE) {
                    atomicOr(flags, SQ_FLAG_PANIC);
                    keep = false;
                } else if (1 < k1) {
                    const uint32_t k2 = rank_k[key % n_ranks];
                    if (k2 == SQ_NONE) atomicOr(flags, SQ_FLAG_PANIC);
                    keep = k2 != SQ_NONE && 1 < k2;
                } else {
                    keep = false;
                }
            }
            survive[s] = keep;
        }
    }
}
__global__ void compact_kernel(uint32_t n_segs, const uint32_t *survive, const uint32_t *surv_idx, uint32_t *pair_seg) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < n_segs; s += stride)
        if (survive[s]) pair_seg[surv_idx[s]] = s;
}

__device__ __forceinline__ unsigned long long sq_choose(unsigned long long x) { return ((x > 1 ? x : 1) - 1) * x / 2; }
__device__ __forceinline__ unsigned long long sq_wave_sum(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;  // lane 0 holds the sum
}

// check_correl :213-252 for one surviving pair per workgroup: the pair's run of records is its list of (c1, c2) observations,
// one per read that has both chunks.  The table sits in LDS; wave 0 then sums its rows, wave 1 its columns, all four waves
// the cells, and thread 0 evaluates misc::adjusted_rand_index (misc.rs:22-46) in wrapping 64-bit integers and one division.
__global__ void __launch_bounds__(256) table_kernel(uint32_t n_pairs, const uint32_t *pair_seg, const uint32_t *seg_start, const uint64_t *keys,
                                                    const uint64_t *vals, uint64_t n_ranks, const uint32_t *rank_k, uint64_t *pair_key,
                                                    double *pair_ari, uint64_t *pair_len, int *flags) {
    __shared__ uint32_t tab[SQ_MAX_LABEL * SQ_MAX_LABEL];
    __shared__ unsigned long long s_match[3];  // lab_match, pred_match, both_match
    __shared__ uint32_t s_rows, s_cols, s_bad;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    for (uint32_t p = blockIdx.x; p < n_pairs; p += gridDim.x) {
        const uint32_t s = pair_seg[p], b = seg_start[s], e = seg_start[s + 1];
        for (uint32_t q = tid; q < SQ_MAX_LABEL * SQ_MAX_LABEL; q += 256) tab[q] = 0;
        if (tid < 3) s_match[tid] = 0;
        if (tid == 0) s_rows = s_cols = s_bad = 0;
        __syncthreads();
        for (uint32_t i = b + tid; i < e; i += 256) {
            const uint64_t v = vals[i];
            const uint32_t c1 = (uint32_t)(v >> 32) & 0xffu, c2 = (uint32_t)(v >> 40) & 0xffu;
            if (((v >> 48) & 1u) || c1 >= SQ_MAX_LABEL || c2 >= SQ_MAX_LABEL) atomicOr(&s_bad, 1u);
            else atomicAdd(&tab[c1 * SQ_MAX_LABEL + c2], 1u);
        }
        __syncthreads();
        if (tid < 128) {  // wave 0: row `lane` (skewed so that the 64 lanes read 64 banks); wave 1: column `lane`
            unsigned long long sum = 0;
            if (tid < 64)
                for (uint32_t j = 0; j < SQ_MAX_LABEL; j++) sum += tab[lane * SQ_MAX_LABEL + ((j + lane) & 63u)];
            else
                for (uint32_t j = 0; j < SQ_MAX_LABEL; j++) sum += tab[j * SQ_MAX_LABEL + lane];
            const uint32_t nonzero = (uint32_t)__popcll(__ballot(sum > 0));
            const unsigned long long m = sq_wave_sum(sq_choose(sum));
            if (lane == 0) {
                s_match[tid >> 6] = m;
                if (tid < 64) s_rows = nonzero;
                else s_cols = nonzero;
            }
        }
        {
            unsigned long long both = 0;
            for (uint32_t q = tid; q < SQ_MAX_LABEL * SQ_MAX_LABEL; q += 256) both += sq_choose(tab[q]);
            both = sq_wave_sum(both);
            if (lane == 0) atomicAdd(&s_match[2], both);
        }
        __syncthreads();
        if (tid == 0) {
            const uint64_t key = keys[b], len = (uint64_t)(e - b);
            double ari = 0.0;
            if (s_bad) {
                atomicOr(flags, SQ_FLAG_LABEL);
            } else if (len == 0) {
                ari = 0.0;
            } else if (s_rows == 1 && s_cols == 1) {  // both label vectors constant
                ari = (rank_k[key / n_ranks] == 1 && rank_k[key % n_ranks] == 1) ? 0.0 : 1.0;
            } else {
                const uint64_t lab_match = s_match[0], pred_match = s_match[1], both_match = s_match[2];
                const uint64_t num_of_pairs = sq_choose(len);
                if (!(both_match <= (lab_match + pred_match) / 2)) atomicOr(flags, SQ_FLAG_PANIC);  // assert!, misc.rs:41
                const int64_t match_prod = (int64_t)(lab_match * pred_match);
                const int64_t denom = (int64_t)(num_of_pairs * (lab_match + pred_match) / 2) - match_prod;
                const int64_t numer = (int64_t)(num_of_pairs * both_match) - match_prod;
                ari = (double)numer / (double)denom;
                if (ari != ari) ari = 0.0;  // :247-250
            }
            pair_key[p] = key;
            pair_ari[p] = ari;
            pair_len[p] = len;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host: classify :254-365 on rand_xoshiro 0.6.0's Xoshiro256PlusPlus and the sampling of rand 0.8.5
// ---------------------------------------------------------------------------------------------------------------------
struct Rng256pp {
    uint64_t s[4];
    static uint64_t rotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
    explicit Rng256pp(uint64_t seed) {  // seed_from_u64: four SplitMix64 outputs
        for (int i = 0; i < 4; i++) {
            seed += 0x9e3779b97f4a7c15ULL;
            uint64_t z = seed;
            z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
            z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
            s[i] = z ^ (z >> 31);
        }
    }
    uint64_t next_u64() {
        const uint64_t r = rotl(s[0] + s[3], 23) + s[0];
        const uint64_t t = s[1] << 17;
        s[2] ^= s[0];
        s[3] ^= s[1];
        s[1] ^= s[2];
        s[0] ^= s[3];
        s[2] ^= t;
        s[3] = rotl(s[3], 45);
        return r;
    }
    uint64_t gen_range_usize(uint64_t n) {  // gen_range(0..n), the 64-bit path
        const uint64_t zone = (n << __builtin_clzll(n)) - 1;
        for (;;) {
            const unsigned __int128 m = (unsigned __int128)next_u64() * n;
            if ((uint64_t)m <= zone) return (uint64_t)(m >> 64);
        }
    }
    bool gen_bool(double p) {  // p == 1 never draws
        if (p == 1.0) return true;
        const double scaled = p * 18446744073709551616.0;
        const uint64_t p_int = !(scaled > 0.0) ? 0 : (scaled >= 18446744073709551616.0 ? UINT64_MAX : (uint64_t)scaled);
        return next_u64() < p_int;
    }
};

struct RelEdge {
    size_t to;
    double score;  // ClassifyParam::score(ari, count) :299-304
};

// classify :254-275 + classify_nodes :281-289 on the pair list in the order given: ids in first-appearance order (`from`, then
// `to`), stiff[i] = the assignment of ids[i]
void classify_pairs(size_t n_pairs, const uint64_t *u1, const uint64_t *u2, const double *ari, const uint64_t *count,
                    const jtk_squish_config_t &cfg, std::vector<uint64_t> &ids, std::vector<uint8_t> &stiff) {
    ids.clear();
    stiff.clear();
    if (n_pairs == 0) return;  // :110-113
    std::unordered_map<uint64_t, size_t> index;
    for (size_t p = 0; p < n_pairs; p++)
        for (const uint64_t u : {u1[p], u2[p]})
            if (index.emplace(u, ids.size()).second) ids.push_back(u);
    std::vector<std::vector<RelEdge>> graph(ids.size());
    for (size_t p = 0; p < n_pairs; p++) {
        double a = ari[p];
        a = (a != a || a < 0.0) ? 0.0 : a;  // .max(0).min(1)
        a = a > 1.0 ? 1.0 : a;
        const double score = a <= cfg.ari_thr ? cfg.mismatch_score * (double)count[p] : cfg.match_score * (double)count[p];
        const size_t from = index[u1[p]], to = index[u2[p]];
        graph[from].push_back({to, score});
        graph[to].push_back({from, score});
    }
    stiff.assign(ids.size(), 1);
    auto diff_on_flip = [&](size_t target) {  // :336-351
        double sum = 0.0;
        for (const RelEdge &e : graph[target])
            if (stiff[e.to]) sum += e.score;
        return stiff[target] ? -sum : sum;
    };
    Rng256pp rng(3093240);
    for (int t = 0; t < 10; t++) {
        for (size_t i = 0; i < ids.size(); i++)  // wipe_through :324-334
            if (0.0 < diff_on_flip(i)) stiff[i] = !stiff[i];
        for (int it = 0; it < 1000; it++) {  // mcmc :353-365
            const size_t i = (size_t)rng.gen_range_usize(ids.size());
            const double diff = diff_on_flip(i);
            const double prob = jtk_exp(diff < 0.0 ? diff : 0.0);
            if (rng.gen_bool(prob)) stiff[i] = !stiff[i];
        }
    }
}

int check_config(const jtk_squish_config_t *cfg) {
    if (!cfg) return jtk_fail(JTK_ERR_INVALID_ARG, "null config");
    return 0;
}

}  // namespace

extern "C" int jtk_lc_squish_classify(size_t n_pairs, const uint64_t *u1, const uint64_t *u2, const double *ari, const uint64_t *count,
                                      const jtk_squish_config_t *cfg, uint64_t *ids, uint8_t *stiff, size_t id_cap, size_t *n_ids) {
    g_last_error.clear();
    if (int rc = check_config(cfg)) return rc;
    if (!n_ids || (n_pairs && (!u1 || !u2 || !ari || !count))) return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    std::vector<uint64_t> id_v;
    std::vector<uint8_t> stiff_v;
    classify_pairs(n_pairs, u1, u2, ari, count, *cfg, id_v, stiff_v);
    *n_ids = id_v.size();
    if (id_v.size() > id_cap || (id_v.size() && (!ids || !stiff))) return jtk_fail(JTK_ERR_INVALID_ARG, "id_cap is too small");
    for (size_t i = 0; i < id_v.size(); i++) {
        ids[i] = id_v[i];
        stiff[i] = stiff_v[i];
    }
    return 0;
}

extern "C" int jtk_lc_squish_clusters(size_t n_reads, const uint64_t *node_off, const jtk_cc_node_t *nodes, const double *posteriors,
                                      size_t n_chunks, jtk_cc_chunk_t *chunks, const jtk_squish_config_t *cfg, uint8_t *class_out,
                                      uint64_t *cluster_out, uint8_t *touched, uint64_t *pair_u1, uint64_t *pair_u2, double *pair_ari,
                                      uint64_t *pair_count, size_t pair_cap, size_t *n_pairs_out, int device) {
    g_last_error.clear();
    if (int rc = check_config(cfg)) return rc;
    if (!node_off) return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    const size_t n_nodes = (size_t)node_off[n_reads];
    if ((n_nodes && (!nodes || !cluster_out || !touched)) || (n_chunks && (!chunks || !class_out)))
        return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    const bool want_pairs = pair_u1 && pair_u2 && pair_ari && pair_count;
    if (want_pairs && !n_pairs_out) return jtk_fail(JTK_ERR_INVALID_ARG, "the pair list needs n_pairs");
    if (n_reads >= 0xffffffffull || n_nodes >= 0xffffffffull) return jtk_fail(JTK_ERR_UNSUPPORTED, "more than 2^32 - 2 reads or nodes");
    size_t n_post = 0;
    for (size_t r = 0; r < n_reads; r++) {
        if (node_off[r + 1] < node_off[r]) return jtk_fail(JTK_ERR_INVALID_ARG, "node_off decreases");
        if (node_off[r + 1] - node_off[r] > SQ_READ_NODES) return jtk_fail(JTK_ERR_UNSUPPORTED, "a read of more than 65535 nodes");
    }
    for (size_t e = 0; e < n_nodes; e++) n_post = std::max<size_t>(n_post, nodes[e].post_off + nodes[e].post_len);
    if (n_post && !posteriors) return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    if (int rc = jtk_require_device(device)) return rc;
    // chunk ids -> ranks in ascending id order (ids of nodes outside chunks[] included): a pair's key is rank1 * n_ranks + rank2,
    // so that the sorted records are in the canonical pair order
    std::vector<uint64_t> ids;
    ids.reserve(n_chunks + n_nodes);
    for (size_t c = 0; c < n_chunks; c++) ids.push_back(chunks[c].id);
    std::sort(ids.begin(), ids.end());
    if (std::adjacent_find(ids.begin(), ids.end()) != ids.end()) return jtk_fail(JTK_ERR_INVALID_ARG, "chunk ids repeat");
    for (size_t e = 0; e < n_nodes; e++) ids.push_back(nodes[e].chunk);
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    const uint64_t n_ranks = std::max<size_t>(ids.size(), 1);
    auto rank_of = [&](uint64_t id) { return (uint32_t)(std::lower_bound(ids.begin(), ids.end(), id) - ids.begin()); };
    std::vector<uint32_t> rank(n_nodes), rank_k(n_ranks, SQ_NONE);
    for (size_t e = 0; e < n_nodes; e++) rank[e] = rank_of(nodes[e].chunk);
    for (size_t c = 0; c < n_chunks; c++) rank_k[rank_of(chunks[c].id)] = chunks[c].cluster_num == SQ_NONE ? SQ_NONE - 1 : chunks[c].cluster_num;

    std::vector<uint64_t> p_key;
    std::vector<double> p_ari;
    std::vector<uint64_t> p_len;
    if (n_nodes) {
        DevStream s;
        JTK_HIP_TRY(s.create());
        const hipStream_t st = s.st;
        DevArr<uint64_t> d_off, d_nrec, d_recoff;
        DevArr<jtk_cc_node_t> d_nodes;
        DevArr<double> d_post;
        DevArr<uint32_t> d_rank, d_rank_k, d_bkey, d_nd;
        DevArr<uint2> d_reps;
        DevArr<int> d_flags;
        {
            std::vector<uint64_t> off_v(node_off, node_off + n_reads + 1);
            std::vector<jtk_cc_node_t> node_v(nodes, nodes + n_nodes);
            std::vector<double> post_v(posteriors, posteriors + n_post);
            int rc;
            if ((rc = d_off.upload(off_v, st)) || (rc = d_nodes.upload(node_v, st)) || (rc = d_post.upload(post_v, st)) ||
                (rc = d_rank.upload(rank, st)) || (rc = d_rank_k.upload(rank_k, st)))
                return jtk_fail(rc, "device upload failed");
            JTK_HIP_TRY(hipStreamSynchronize(st));  // the staging vectors go out of scope
        }
        JTK_HIP_TRY(d_bkey.alloc(n_nodes));
        JTK_HIP_TRY(d_reps.alloc(n_nodes));
        JTK_HIP_TRY(d_nd.alloc(n_reads));
        JTK_HIP_TRY(d_nrec.alloc(n_reads + 1));
        JTK_HIP_TRY(d_recoff.alloc(n_reads + 1));
        JTK_HIP_TRY(d_flags.alloc(1));
        JTK_HIP_TRY(d_flags.zero(1, st));
        JTK_HIP_TRY(d_nrec.zero(n_reads + 1, st));
        biased_kernel<<<jtk_blocks(n_nodes, 256, 4096), 256, 0, st>>>(n_nodes, d_nodes.cget(), d_post.cget(), d_rank.cget(), d_bkey.get());
        const uint32_t read_grid = jtk_blocks(n_reads, 1, SQ_READ_GRID);
        distinct_kernel<<<read_grid, 256, 0, st>>>((uint32_t)n_reads, d_off.cget(), d_nodes.cget(), d_bkey.cget(), d_reps.get(), d_nd.get(), d_nrec.get());
        RocTemp tmp;
        auto scan = [&](auto *in, auto *out, size_t n) {  // exclusive prefix sum of n entries
            using T = std::remove_pointer_t<decltype(out)>;
            return tmp.run([&](void *t, size_t &bytes) { return rocprim::exclusive_scan(t, bytes, in, out, T(0), n, rocprim::plus<T>(), st); });
        };
        JTK_HIP_TRY(scan(d_nrec.cget(), d_recoff.get(), n_reads + 1));
        uint64_t n_rec = 0;
        JTK_HIP_TRY(d_recoff.download(&n_rec, 1, st, n_reads));
        JTK_HIP_TRY(hipStreamSynchronize(st));
        JTK_HIP_TRY(hipGetLastError());
        if (n_rec >= 0x7fffffffull) return jtk_fail(JTK_ERR_UNSUPPORTED, "2^31 - 1 or more chunk-pair records");
        if (n_rec) {
            DevArr<uint64_t> d_keys, d_vals, d_keys_s, d_vals_s;
            DevArr<uint32_t> d_head, d_segof, d_segstart;
            JTK_HIP_TRY(d_keys.alloc(n_rec));
            JTK_HIP_TRY(d_vals.alloc(n_rec));
            JTK_HIP_TRY(d_keys_s.alloc(n_rec));
            JTK_HIP_TRY(d_vals_s.alloc(n_rec));
            emit_kernel<<<read_grid, 64, 0, st>>>((uint32_t)n_reads, d_off.cget(), d_reps.cget(), d_nd.cget(), d_recoff.cget(), n_ranks, d_keys.get(),
                                                  d_vals.get());
            {  // the key's significant bits only
                const unsigned __int128 top = (unsigned __int128)n_ranks * n_ranks - 1;
                unsigned end_bit = 1;
                while (end_bit < 64 && (top >> end_bit)) end_bit++;
                JTK_HIP_TRY(tmp.run([&](void *t, size_t &bytes) {
                    return rocprim::radix_sort_pairs(t, bytes, d_keys.cget(), d_keys_s.get(), d_vals.cget(), d_vals_s.get(), (size_t)n_rec, 0u, end_bit, st);
                }));
            }
            const uint64_t *ks = d_keys_s.cget(), *vs = d_vals_s.cget();
            JTK_HIP_TRY(d_head.alloc(n_rec + 1));
            JTK_HIP_TRY(d_segof.alloc(n_rec + 1));
            JTK_HIP_TRY(d_head.zero(n_rec + 1, st));
            const uint32_t rec_grid = jtk_blocks(n_rec, 256, 4096);
            head_kernel<<<rec_grid, 256, 0, st>>>(n_rec, ks, d_head.get());
            JTK_HIP_TRY(scan(d_head.cget(), d_segof.get(), n_rec + 1));
            uint32_t n_segs = 0;
            JTK_HIP_TRY(d_segof.download(&n_segs, 1, st, n_rec));
            JTK_HIP_TRY(hipStreamSynchronize(st));
            JTK_HIP_TRY(hipGetLastError());
            DevArr<uint32_t> d_survive, d_survidx, d_pairseg;
            JTK_HIP_TRY(d_segstart.alloc((size_t)n_segs + 1));
            JTK_HIP_TRY(d_survive.alloc((size_t)n_segs + 1));
            JTK_HIP_TRY(d_survidx.alloc((size_t)n_segs + 1));
            JTK_HIP_TRY(d_survive.zero((size_t)n_segs + 1, st));
            seg_start_kernel<<<rec_grid, 256, 0, st>>>(n_rec, n_segs, d_head.cget(), d_segof.cget(), d_segstart.get());
            retain_kernel<<<jtk_blocks(n_segs, 4, 4096), 256, 0, st>>>(n_segs, d_segstart.cget(), ks, vs, n_ranks, d_rank_k.cget(), cfg->count_thr,
                                                                       d_survive.get(), d_flags.get());
            JTK_HIP_TRY(scan(d_survive.cget(), d_survidx.get(), (size_t)n_segs + 1));
            uint32_t n_surv = 0;
            int flags = 0;
            JTK_HIP_TRY(d_survidx.download(&n_surv, 1, st, n_segs));
            JTK_HIP_TRY(d_flags.download(&flags, 1, st));
            JTK_HIP_TRY(hipStreamSynchronize(st));
            JTK_HIP_TRY(hipGetLastError());
            if (flags & SQ_FLAG_PANIC)
                return jtk_fail(JTK_ERR_CHUNK_FAILED, "a chunk pair above count_thr names a chunk id that is not in chunks[]");
            if (n_surv) {
                DevArr<uint64_t> d_pkey, d_plen;
                DevArr<double> d_pari;
                JTK_HIP_TRY(d_pairseg.alloc(n_surv));
                JTK_HIP_TRY(d_pkey.alloc(n_surv));
                JTK_HIP_TRY(d_pari.alloc(n_surv));
                JTK_HIP_TRY(d_plen.alloc(n_surv));
                compact_kernel<<<jtk_blocks(n_segs, 256, 4096), 256, 0, st>>>(n_segs, d_survive.cget(), d_survidx.cget(), d_pairseg.get());
                table_kernel<<<jtk_blocks(n_surv, 1, SQ_TABLE_GRID), 256, 0, st>>>(n_surv, d_pairseg.cget(), d_segstart.cget(), ks, vs, n_ranks, d_rank_k.cget(),
                                                                                   d_pkey.get(), d_pari.get(), d_plen.get(), d_flags.get());
                p_key.resize(n_surv);
                p_ari.resize(n_surv);
                p_len.resize(n_surv);
                JTK_HIP_TRY(d_pkey.download(p_key.data(), n_surv, st));
                JTK_HIP_TRY(d_pari.download(p_ari.data(), n_surv, st));
                JTK_HIP_TRY(d_plen.download(p_len.data(), n_surv, st));
                JTK_HIP_TRY(d_flags.download(&flags, 1, st));
                JTK_HIP_TRY(hipStreamSynchronize(st));
                JTK_HIP_TRY(hipGetLastError());
                if (flags & SQ_FLAG_PANIC) return jtk_fail(JTK_ERR_CHUNK_FAILED, "adjusted_rand_index: both_match above the mean of the marginals");
                if (flags & SQ_FLAG_LABEL)
                    return jtk_fail(JTK_ERR_UNSUPPORTED, "a cluster label of 64 or more enters the table of a surviving chunk pair");
            }
        }
    }
    // ---- host: the pairs back as chunk ids, classify, touch_chunks (:106-109, keyed by the smaller id only), classes :137-165
    const size_t n_pairs = p_key.size();
    std::vector<uint64_t> u1(n_pairs), u2(n_pairs);
    for (size_t p = 0; p < n_pairs; p++) {
        u1[p] = ids[p_key[p] / n_ranks];
        u2[p] = ids[p_key[p] % n_ranks];
    }
    if (n_pairs_out) *n_pairs_out = n_pairs;
    if (want_pairs && n_pairs > pair_cap) return jtk_fail(JTK_ERR_INVALID_ARG, "pair_cap is too small");
    std::vector<uint64_t> cl_ids;
    std::vector<uint8_t> cl_stiff;
    classify_pairs(n_pairs, u1.data(), u2.data(), p_ari.data(), p_len.data(), *cfg, cl_ids, cl_stiff);
    std::unordered_set<uint64_t> stiff;
    for (size_t i = 0; i < cl_ids.size(); i++)
        if (cl_stiff[i]) stiff.insert(cl_ids[i]);
    std::unordered_set<uint64_t> touch_stiff;  // ids whose touch_chunks entry holds a stiff chunk
    for (size_t p = 0; p < n_pairs; p++)
        if (stiff.count(u2[p])) touch_stiff.insert(u1[p]);
    std::unordered_set<uint64_t> suspicious;
    for (size_t c = 0; c < n_chunks; c++) {
        if (stiff.count(chunks[c].id) || 2 < chunks[c].copy_num) {
            class_out[c] = JTK_REL_STIFF;
        } else if (touch_stiff.count(chunks[c].id)) {
            class_out[c] = JTK_REL_SUSPICIOUS;
            suspicious.insert(chunks[c].id);
        } else {
            class_out[c] = JTK_REL_ISOLATED;
        }
    }
    // ---- write-back :45-59
    for (size_t c = 0; c < n_chunks; c++)
        if (class_out[c] == JTK_REL_SUSPICIOUS) chunks[c].cluster_num = 1;
    for (size_t e = 0; e < n_nodes; e++) {
        const bool hit = suspicious.count(nodes[e].chunk) != 0;
        cluster_out[e] = hit ? 0 : nodes[e].cluster;
        touched[e] = hit;
    }
    if (want_pairs)
        for (size_t p = 0; p < n_pairs; p++) {
            pair_u1[p] = u1[p];
            pair_u2[p] = u2[p];
            pair_ari[p] = p_ari[p];
            pair_count[p] = p_len[p];
        }
    return 0;
}
