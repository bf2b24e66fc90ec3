// fill.hip -- jtk_lc_fill_candidates: the candidate search of correct_deletion (haplotyper/src/encode/deletion_fill.rs), the part
// of `correct_deletion_error` (:301-337) in front of try_encoding_head / _tail:
//
//   ReadSkelton::from_rich_nodes (:1003-1030)      a read as light nodes: key (chunk, cluster, direction), the gap to the previous
//                                                  node's end and to the next node's start
//   check_alignment_by_chunkmatch (:611-637)       multiset intersection of the sorted keys, forward and with every direction flipped
//   pairwise_alignment_gotoh (:738-827)            three-state affine alignment over nodes, end gaps free, its traceback
//   alignment (:707-725)                           the verdict: matched nodes, score, no Ins next to a Del
//   get_pileup (:642-698)                          the walk of the ops into coverage and per-slot head / tail insertion lists
//   mean_cov, ins_thr (:312-314, :872-879)
//   Pileup::check_insertion_head / _tail (:940-981) with summarize (:910-933)
//
// Every value is an integer, so the outputs are the reference's bit for bit.  On the device:
//   1. pair_emit_kernel: the nodes of a (chunk, cluster) key lie back to back in `order` (the host ranks the keys); every node
//      of a target read writes one (target, query) record per node of its key.  A pair can pass the pre-filter only if the reads
//      share such a key: min_match >= 1 for a target with a node.  rocprim sorts the records and drops the repeats.
//   2. pair_kernel: one wave per pair.  The pre-filter counts, the direction, the fill by rows with lanes over the columns (state 1
//      of a row is a prefix maximum over the row's state 0), four traceback bits per cell, the traceback, the verdict and the
//      walk.  The rows, the bits and the runs of a pair live in FC_LDS_PER_WAVE bytes of LDS; a pair that needs more is left to a
//      second launch with few waves, which keeps them in a global work area.  Coverage is integer atomic adds; insertion
//      records go to a list whose order depends on the waves -- the next step sorts it.
//   3. two stable radix sorts put the records in (target, slot, side, key, direction) order; summarise_kernel reduces every run
//      of equal keys to its count and its integer offset sum, applies ins_thr and the offset rule, and compacts the candidates.
// No output depends on the order in which pairs finish.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>

#include "device_common.h"
#include "jtk_lc_debug.h"
#include "prim_host.h"
#include "wave_util.h"

namespace {

constexpr int32_t FC_MIN_ALN = -10000000;       // deletion_fill.rs:727
constexpr int32_t FC_NEG = -0x40000000;         // below every value of the table: a lane without a column
constexpr uint32_t FC_MAX_NODES = 65535;        // nodes of one read (the limit jtk_lc_squish_clusters set)
constexpr uint32_t FC_LDS_PER_WAVE = 8192;      // four waves a block: 32 KiB; the kernel's registers admit four such blocks a CU
constexpr uint32_t FC_WAVES = 4;
constexpr uint32_t FC_GRID = 2048;              // blocks of the LDS launch at most
constexpr uint64_t FC_WORK_BYTES = 1ull << 30;  // global work area of the second launch, shared out among its waves
constexpr uint32_t FC_LARGE_WAVES = 1024;
enum { FC_MATCH = 0, FC_INS = 1, FC_DEL = 2 };

// bytes one pair needs: two rows of three states, the runs of the ops, four bits per cell
__host__ __device__ inline uint64_t fc_need(uint32_t n, uint32_t m) {
    return 24ull * (m + 1) + 4ull * ((uint64_t)n + m + 2) + (uint64_t)n * ((m + 1) >> 1);
}

struct FillArgs {
    uint64_t n_pairs;
    const uint64_t *pairs;  // target << 32 | query
    const uint64_t *node_off;
    const uint32_t *ck;     // per node: rank of its chunk id << 1 | is_forward
    const uint32_t *kid;    // per node: rank of its (chunk, cluster)
    const int64_t *start, *end;
    uint32_t *coverage;     // read r's slots at node_off[r] + r
    uint64_t *rec_hi, *rec_lo;
    int64_t *rec_val;
    uint64_t rec_cap;
    unsigned long long *rec_count;
    uint8_t *work;          // LARGE only
    uint64_t work_stride;
    // jtk_lc_debug_fill_pairs (null otherwise): per pair, and ops[ops_off[pair] ..) = len << 2 | code in alignment order
    int32_t *dbg_dir, *dbg_score;
    uint8_t *dbg_pass;
    uint32_t *dbg_ops, *dbg_nops;
    const uint64_t *dbg_ops_off;
};

__device__ __forceinline__ int32_t fc_max(int32_t a, int32_t b) { return a > b ? a : b; }

// One (target, query) pair by one wave; `area` holds fc_need(n, m) bytes (LDS or global, 8-byte aligned).
__device__ void fc_pair(const FillArgs &a, uint64_t pi, uint32_t t, uint32_t q, uint8_t *area, uint32_t lane) {
    const uint64_t tb = a.node_off[t], qb = a.node_off[q];
    const uint32_t n = (uint32_t)(a.node_off[t + 1] - tb), m = (uint32_t)(a.node_off[q + 1] - qb);
    int32_t dir = -1, dist = 0;
    bool pass = false;
    uint32_t n_runs = 0;
    int32_t *rows = (int32_t *)area;
    uint32_t *runs = (uint32_t *)(area + 24ull * (m + 1));
    uint8_t *bits = area + 24ull * (m + 1) + 4ull * ((uint64_t)n + m + 2);
    const uint32_t row_bytes = (m + 1) >> 1;
    // ---- check_alignment_by_chunkmatch: sum over the target's nodes of [its rank among the target's equal keys < the query's
    // number of that key] is the multiset intersection
    uint32_t fwd_match = 0, rev_match = 0;
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t i = base + lane;
        bool f = false, r = false;
        if (i < n) {
            const uint32_t c = a.ck[tb + i], k = a.kid[tb + i];
            uint32_t rank = 0, cf = 0, cr = 0;
            for (uint32_t j = 0; j < i; j++) rank += a.kid[tb + j] == k && a.ck[tb + j] == c;
            for (uint32_t j = 0; j < m; j++) {
                const bool same = a.kid[qb + j] == k;
                cf += same && a.ck[qb + j] == c;
                cr += same && a.ck[qb + j] == (c ^ 1u);
            }
            f = rank < cf;
            r = rank < cr;
        }
        fwd_match += (uint32_t)__popcll(__ballot(f));
        rev_match += (uint32_t)__popcll(__ballot(r));
    }
    const uint32_t min_match = n < 2u ? n : 2u;
    if (n != 0 && min_match <= (fwd_match > rev_match ? fwd_match : rev_match)) {
        const bool forward = rev_match <= fwd_match;
        dir = forward ? 1 : 0;
        const uint32_t flip = forward ? 0u : 1u;
        // the query as aligned: node p is the query's node p, or for a reverse query its node m - 1 - p with the direction flipped
#define FC_ORIG(p) (forward ? (p) : m - 1 - (p))
        // ---- the fill.  rows[(b * 3 + s) * (m + 1) + j] = state s of column j of row buffer b
        const uint32_t w = m + 1;
        for (uint32_t j = lane; j <= m; j += 64) {  // row 0: (0, MIN, MIN), then (MIN, 0, MIN)
            rows[j] = j ? FC_MIN_ALN : 0;
            rows[w + j] = j ? 0 : FC_MIN_ALN;
            rows[2 * w + j] = FC_MIN_ALN;
        }
        jtk_wave_sync();
        // the end cell: (i, m) for i = 0 ..= n, then (n, j) for j = 0 ..= m; the last maximum wins, in the cell and in the chain
        int32_t best = 0;
        uint32_t best_r = 0, best_q = m, best_state = 1;  // cell (0, m) = (MIN, 0, MIN); m >= 1 here
        for (uint32_t i = 1; i <= n; i++) {
            const int32_t *prev = rows + ((i - 1) & 1u) * 3 * w;
            int32_t *cur = rows + (i & 1u) * 3 * w;
            const uint32_t tc = a.ck[tb + i - 1], tk = a.kid[tb + i - 1];
            if (lane == 0) {  // column 0 of a row below the first: (MIN, MIN, 0)
                cur[0] = FC_MIN_ALN;
                cur[w] = FC_MIN_ALN;
                cur[2 * w] = 0;
            }
            int32_t run = FC_MIN_ALN;      // state 1 of the column in front of this chunk's first
            int32_t left_s0 = FC_MIN_ALN;  // state 0 of that column
            for (uint32_t base = 0; base < m; base += 64) {
                const uint32_t j = base + lane + 1;
                const bool active = j <= m;
                int32_t s0 = FC_NEG, s2 = FC_NEG;
                uint32_t nib = 0;
                if (active) {
                    const int32_t p0 = prev[j - 1], p1 = prev[w + j - 1], p2 = prev[2 * w + j - 1];
                    const int32_t u0 = prev[j], u2 = prev[2 * w + j];
                    const int32_t mx = fc_max(p0, fc_max(p1, p2));
                    nib = p0 == mx ? 0u : (p1 == mx ? 1u : 2u);  // the first state that holds the maximum
                    const uint32_t o = FC_ORIG(j - 1);
                    const uint32_t qc = a.ck[qb + o] ^ flip;
                    const int32_t sc = qc != tc ? FC_MIN_ALN : (a.kid[qb + o] == tk ? 1 : -1);
                    s0 = mx + sc;
                    s2 = fc_max(u0 - 1, u2);
                    nib |= (s2 == u0 - 1 ? 1u : 0u) << 3;
                }
                // state 1 = max(state 1 of column 0, state 0 of every column to the left - 1)
                int32_t incl = active ? s0 - 1 : FC_NEG;
                for (uint32_t o = 1; o < 64; o <<= 1) {
                    const int32_t u = __shfl_up(incl, o, 64);
                    if (lane >= o) incl = fc_max(incl, u);
                }
                int32_t excl = __shfl_up(incl, 1, 64);
                int32_t ls0 = __shfl_up(s0, 1, 64);
                if (lane == 0) {
                    excl = FC_NEG;
                    ls0 = left_s0;
                }
                const int32_t s1 = fc_max(run, excl);
                nib |= (s1 == ls0 - 1 ? 1u : 0u) << 2;
                run = fc_max(run, __shfl(incl, 63, 64));
                left_s0 = __shfl(s0, 63, 64);
                if (active) {
                    cur[j] = s0;
                    cur[w + j] = s1;
                    cur[2 * w + j] = s2;
                }
                const uint32_t other = (uint32_t)__shfl_down((int)nib, 1, 64);  // column j + 1 shares the byte of an odd j
                if (active && !(lane & 1u)) bits[(uint64_t)(i - 1) * row_bytes + ((j - 1) >> 1)] = (uint8_t)(nib | (other << 4));
            }
            jtk_wave_sync();
            const int32_t e0 = cur[m], e1 = cur[w + m], e2 = cur[2 * w + m];
            const int32_t ev = fc_max(e0, fc_max(e1, e2));
            if (ev >= best) {
                best = ev;
                best_r = i;
                best_q = m;
                best_state = e2 == ev ? 2u : (e1 == ev ? 1u : 0u);
            }
        }
        {  // the last row, j = 0 ..= m
            const int32_t *last = rows + (n & 1u) * 3 * w;
            for (uint32_t base = 0; base <= m; base += 64) {
                const uint32_t j = base + lane;
                int32_t v = FC_NEG;
                uint32_t st = 0;
                if (j <= m) {
                    const int32_t e0 = last[j], e1 = last[w + j], e2 = last[2 * w + j];
                    v = fc_max(e0, fc_max(e1, e2));
                    st = e2 == v ? 2u : (e1 == v ? 1u : 0u);
                }
                int32_t mx = v;
                for (uint32_t o = 32; o; o >>= 1) mx = fc_max(mx, __shfl_xor(mx, o, 64));
                if (mx >= best) {
                    const uint64_t at = __ballot(v == mx);
                    const uint32_t top = 63u - (uint32_t)__builtin_clzll(at);
                    best = mx;
                    best_r = n;
                    best_q = base + top;
                    best_state = (uint32_t)__shfl((int)st, (int)top, 64);
                }
            }
        }
        dist = best;
        // ---- the traceback, every lane the same; the runs are pushed from the alignment's end
        uint32_t r = best_r, c = best_q, state = best_state, run_code = 3, run_len = 0, matched = 0;
        bool proper = true;
        auto push = [&](uint32_t code, uint32_t len) {
            if (code == run_code) {
                run_len += len;
                return;
            }
            if (run_len) {
                if (lane == 0) runs[n_runs] = run_len << 2 | run_code;
                n_runs++;
                if ((run_code == FC_INS && code == FC_DEL) || (run_code == FC_DEL && code == FC_INS)) proper = false;  // is_proper :722-725
            }
            run_code = code;
            run_len = len;
        };
        if (n != r) push(FC_DEL, n - r);
        if (m != c) push(FC_INS, m - c);
        while (r > 0 && c > 0) {
            const uint32_t nib = (bits[(uint64_t)(r - 1) * row_bytes + ((c - 1) >> 1)] >> (((c - 1) & 1u) * 4)) & 15u;
            if (state == 0) {
                state = nib & 3u;
                push(FC_MATCH, 1);
                matched++;
                r--;
                c--;
            } else if (state == 1) {
                state = (nib >> 2) & 1u ? 0u : 1u;
                push(FC_INS, 1);
                c--;
            } else {
                state = (nib >> 3) & 1u ? 0u : 2u;
                push(FC_DEL, 1);
                r--;
            }
        }
        if (r != 0) push(FC_DEL, r);
        if (c != 0) push(FC_INS, c);
        push(3, 0);  // flushes the open run
        jtk_wave_sync();
        const uint32_t min_nm = min_match < m ? min_match : m;
        pass = min_nm <= matched && 1 <= dist && proper;
        // ---- get_pileup's walk, twice: the records are counted, one reservation is made, then they are written
        if (pass && a.coverage) {
            const uint64_t cov = tb + t;
            uint64_t at = 0;
            for (int write = 0; write < 2; write++) {
                uint32_t pos = 0, qp = 0, n_rec = 0;
                auto record = [&](uint32_t side, uint32_t p) {
                    if (write && lane == 0 && at + n_rec < a.rec_cap) {
                        const uint32_t o = FC_ORIG(p);
                        // the aligned node's prev_offset (head) or after_offset (tail); a reverse query swaps the two
                        const bool want_prev = (side == 0) == forward;
                        const bool present = want_prev ? o > 0 : o + 1 < m;
                        int64_t off = 0;
                        if (present)
                            off = want_prev ? (int64_t)((uint64_t)a.start[qb + o] - (uint64_t)a.end[qb + o - 1])
                                            : (int64_t)((uint64_t)a.start[qb + o + 1] - (uint64_t)a.end[qb + o]);
                        a.rec_hi[at + n_rec] = (uint64_t)t << 17 | (uint64_t)pos << 1 | side;
                        a.rec_lo[at + n_rec] = (uint64_t)a.kid[qb + o] << 2 | (uint64_t)((a.ck[qb + o] ^ flip) & 1u) << 1 | (present ? 1u : 0u);
                        a.rec_val[at + n_rec] = off;
                    }
                    n_rec++;
                };
                for (uint32_t k = n_runs; k-- > 0;) {
                    const uint32_t code = runs[k] & 3u, len = runs[k] >> 2;
                    if (code == FC_INS) {
                        if (pos == 0) {
                            record(1, qp + len - 1);  // only the last inserted node
                        } else if (2 * (uint64_t)pos + 1 == n) {
                            record(0, qp);  // `pileups.len() - 1` of the shadowing iterator: what remains, n - pos, minus one
                        } else {            // (at pos == n that subtraction wraps and this arm runs)
                            record(0, qp);
                            if (len >= 2) record(1, qp + len - 1);
                        }
                        qp += len;
                    } else if (code == FC_DEL) {
                        pos += len;
                    } else {
                        if (!write)
                            for (uint32_t x = lane; x < len; x += 64) atomicAdd(a.coverage + cov + pos + x, 1u);
                        pos += len;
                        qp += len;
                    }
                }
                if (!write) {
                    if (n_rec == 0) break;
                    unsigned long long got = 0;
                    if (lane == 0) got = atomicAdd(a.rec_count, (unsigned long long)n_rec);
                    at = (uint64_t)__shfl((long long)got, 0, 64);
                }
            }
        }
#undef FC_ORIG
    }
    if (a.dbg_dir) {
        const uint64_t ob = a.dbg_ops_off[pi];
        for (uint32_t k = lane; k < n_runs; k += 64) a.dbg_ops[ob + k] = runs[n_runs - 1 - k];
        if (lane == 0) {
            a.dbg_dir[pi] = dir;
            a.dbg_score[pi] = dist;
            a.dbg_pass[pi] = pass ? 1 : 0;
            a.dbg_nops[pi] = n_runs;
        }
    }
    jtk_wave_sync();  // the area is the next pair's
}

// Waves take the pairs 64 at a time, a lane looks up whether its pair is this launch's kind, the wave then does them in turn.
template <bool LARGE>
__global__ void __launch_bounds__(FC_WAVES * 64) pair_kernel(FillArgs a) {
    extern __shared__ uint64_t fc_lds[];
    const uint32_t lane = threadIdx.x & 63u, wave_in_block = threadIdx.x >> 6;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + wave_in_block, n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    uint8_t *area = LARGE ? a.work + wave * a.work_stride : (uint8_t *)fc_lds + (size_t)wave_in_block * FC_LDS_PER_WAVE;
    for (uint64_t base = wave * 64; base < a.n_pairs; base += n_waves * 64) {
        const uint64_t pi = base + lane;
        uint64_t pr = 0;
        bool mine = false;
        if (pi < a.n_pairs) {
            pr = a.pairs[pi];
            const uint32_t t = (uint32_t)(pr >> 32), q = (uint32_t)pr;
            const uint32_t n = (uint32_t)(a.node_off[t + 1] - a.node_off[t]), m = (uint32_t)(a.node_off[q + 1] - a.node_off[q]);
            mine = (fc_need(n, m) > FC_LDS_PER_WAVE) == LARGE;
        }
        uint64_t todo = __ballot(mine);
        while (todo) {
            const int src = __builtin_ctzll(todo);
            todo &= todo - 1;
            const uint64_t p = (uint64_t)__shfl((long long)pr, src, 64);
            fc_pair(a, base + (uint64_t)src, (uint32_t)(p >> 32), (uint32_t)p, area, lane);
        }
    }
}

// one (target, query) record per node of the key of every node of a target read
__global__ void __launch_bounds__(256) pair_emit_kernel(uint32_t n_nodes, const uint32_t *kid, const uint32_t *read_of, const uint32_t *order,
                                                        const uint32_t *seg_start, const uint64_t *rec_off, uint64_t *out) {
    const uint32_t lane = threadIdx.x & 63u, wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t e = wave; e < n_nodes; e += n_waves) {
        const uint64_t ob = rec_off[e];
        if (rec_off[e + 1] == ob) continue;  // a node of a read that is no target
        const uint32_t sb = seg_start[kid[e]], k = seg_start[kid[e] + 1] - sb;
        const uint64_t hi = (uint64_t)read_of[e] << 32;
        for (uint32_t j = lane; j < k; j += 64) out[ob + j] = hi | read_of[order[sb + j]];
    }
}

__global__ void fc_iota_kernel(uint64_t n, uint32_t *p) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = (uint32_t)i;
}
__global__ void fc_gather_kernel(uint64_t n, const uint32_t *perm, const uint64_t *in, uint64_t *out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = in[perm[i]];
}

// mean_cov (:872-879) and ins_thr (:312-314) of every read
__global__ void ins_thr_kernel(uint32_t n_reads, const uint64_t *node_off, const uint32_t *coverage, uint32_t *ins_thr) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += stride) {
        const uint64_t b = node_off[r] + r, slots = node_off[r + 1] - node_off[r] + 1;
        uint64_t sum = 0;
        for (uint64_t i = 0; i < slots; i++) sum += coverage[b + i];
        const uint64_t thr = sum / slots / 5;
        ins_thr[r] = thr < 2 ? (uint32_t)thr : 2u;
    }
}

// The records in (target, slot, side, key, direction) order: hi[i] and lo[perm[i]].  The first record of a run of equal keys
// reduces the run (check_insertion_head / _tail with summarize).  write == 0: flag[i] = 1 where the run yields a candidate;
// write == 1: the candidate goes to cands[pos[i]] and is counted for its read.
__global__ void summarise_kernel(uint64_t n_rec, const uint64_t *hi, const uint64_t *lo, const uint32_t *perm, const int64_t *val,
                                 const uint64_t *node_off, const int64_t *start, const int64_t *end, const uint32_t *ins_thr,
                                 const uint64_t *key_chunk, const uint64_t *key_cluster, int write, uint32_t *flag, const uint32_t *pos,
                                 jtk_fill_cand_t *cands, uint32_t *per_read) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_rec; i += stride) {
        const uint64_t h = hi[i], l = lo[perm[i]] >> 1;
        const bool head = i == 0 || hi[i - 1] != h || (lo[perm[i - 1]] >> 1) != l;
        if (!write) flag[i] = 0;
        if (!head || (write && !flag[i])) continue;
        uint32_t count = 0;
        int64_t present = 0, total = 0;
        for (uint64_t j = i; j < n_rec && hi[j] == h && (lo[perm[j]] >> 1) == l; j++) {
            count++;
            if (lo[perm[j]] & 1u) {
                present++;
                total += val[perm[j]];
            }
        }
        const uint32_t read = (uint32_t)(h >> 17), slot = (uint32_t)(h >> 1) & 0xffffu, side = (uint32_t)h & 1u;
        const uint64_t nb = node_off[read], n = node_off[read + 1] - nb;
        // a head list at slot 0 is empty (an insertion at position 0 goes to the tail list only), so slot - 1 exists; the
        // tail list of slot n is not looked at (nodes.get(idx) is None, :967-970)
        const bool ok = count >= ins_thr[read] && present > 0 && !(side == 1 && slot >= n) && !(side == 0 && slot == 0);
        if (!write) {
            flag[i] = ok ? 1u : 0u;
            continue;
        }
        const int64_t off = total / present;  // truncates toward zero, like isize / isize
        jtk_fill_cand_t c;
        c.read = read;
        c.slot = slot;
        c.side = side;
        c.is_forward = (uint32_t)l & 1u;
        c.chunk = key_chunk[l >> 1];
        c.cluster = key_cluster[l >> 1];
        c.count = count;
        c.reserved = 0;
        if (side == 0) {
            c.position = (int64_t)((uint64_t)end[nb + slot - 1] + (uint64_t)off);
        } else {
            const int64_t p = (int64_t)((uint64_t)start[nb + slot] - (uint64_t)off);
            c.position = p > 0 ? p : 0;
        }
        cands[pos[i]] = c;
        atomicAdd(per_read + read, 1u);
    }
}

// The reads on the host, then on the device.
struct Reads {
    uint32_t n_reads = 0, n_nodes = 0, n_keys = 0, max_nodes = 0, max_target_nodes = 0;
    std::vector<uint32_t> ck, kid, read_of, order, seg_start;
    std::vector<int64_t> start, end;
    std::vector<uint64_t> key_chunk, key_cluster;
    DevArr<uint64_t> d_off;
    DevArr<uint32_t> d_ck, d_kid;
    DevArr<int64_t> d_start, d_end;
};

int fc_check(size_t n_reads, const uint64_t *node_off, const jtk_fill_node_t *nodes) {
    if (!node_off) return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    if (int rc = jtk_check_offsets(n_reads, node_off, "node_off")) return rc;
    if (node_off[n_reads] && !nodes) return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    for (size_t r = 0; r < n_reads; r++)
        if (node_off[r + 1] - node_off[r] > FC_MAX_NODES) return jtk_fail(JTK_ERR_UNSUPPORTED, "a read with more than 65,535 nodes");
    if (n_reads >= 0x7fffffffu || node_off[n_reads] + n_reads >= 0xffffffffull) return jtk_fail(JTK_ERR_UNSUPPORTED, "2^31 - 1 reads or 2^32 - 1 slots, or more");
    return 0;
}

// ranks of the (chunk, cluster) keys and of the chunk ids; the nodes of a key back to back in `order`
void fc_index(Reads &R, size_t n_reads, const uint64_t *node_off, const jtk_fill_node_t *nodes, const uint8_t *target) {
    R.n_reads = (uint32_t)n_reads;
    const uint32_t n = R.n_nodes = (uint32_t)node_off[n_reads];
    R.ck.resize(n);
    R.kid.resize(n);
    R.read_of.resize(n);
    R.start.resize(n);
    R.end.resize(n);
    R.order.resize(n);
    for (uint32_t r = 0; r < R.n_reads; r++) {
        const uint32_t len = (uint32_t)(node_off[r + 1] - node_off[r]);
        R.max_nodes = std::max(R.max_nodes, len);
        if (!target || target[r]) R.max_target_nodes = std::max(R.max_target_nodes, len);
        for (uint64_t e = node_off[r]; e < node_off[r + 1]; e++) R.read_of[e] = r;
    }
    std::iota(R.order.begin(), R.order.end(), 0u);
    std::sort(R.order.begin(), R.order.end(), [&](uint32_t x, uint32_t y) {
        if (nodes[x].chunk != nodes[y].chunk) return nodes[x].chunk < nodes[y].chunk;
        if (nodes[x].cluster != nodes[y].cluster) return nodes[x].cluster < nodes[y].cluster;
        return x < y;
    });
    uint32_t chunk_rank = 0;
    for (uint32_t i = 0; i < n; i++) {
        const jtk_fill_node_t &nd = nodes[R.order[i]];
        if (i && nodes[R.order[i - 1]].chunk != nd.chunk) chunk_rank++;
        if (!i || nodes[R.order[i - 1]].chunk != nd.chunk || nodes[R.order[i - 1]].cluster != nd.cluster) {
            R.seg_start.push_back(i);
            R.key_chunk.push_back(nd.chunk);
            R.key_cluster.push_back(nd.cluster);
        }
        const uint32_t e = R.order[i];
        R.kid[e] = (uint32_t)R.seg_start.size() - 1;
        R.ck[e] = chunk_rank << 1 | (nd.is_forward ? 1u : 0u);
        R.start[e] = (int64_t)nd.position;
        R.end[e] = (int64_t)(nd.position + nd.query_len);
    }
    R.n_keys = (uint32_t)R.seg_start.size();
    R.seg_start.push_back(n);
}

int fc_upload(Reads &R, const uint64_t *node_off, hipStream_t st) {
    const std::vector<uint64_t> off(node_off, node_off + R.n_reads + 1);
    int rc;
    if ((rc = R.d_off.upload(off, st)) || (rc = R.d_ck.upload(R.ck, st)) || (rc = R.d_kid.upload(R.kid, st)) || (rc = R.d_start.upload(R.start, st)) ||
        (rc = R.d_end.upload(R.end, st)))
        return jtk_fail(rc, "device upload failed");
    JTK_HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// the arguments both entry points give the pair kernel: the pair list and the reads
FillArgs fc_args(const Reads &R, uint64_t n_pairs, const uint64_t *d_pairs) {
    FillArgs a{};
    a.n_pairs = n_pairs;
    a.pairs = d_pairs;
    a.node_off = R.d_off.cget();
    a.ck = R.d_ck.cget();
    a.kid = R.d_kid.cget();
    a.start = R.d_start.cget();
    a.end = R.d_end.cget();
    return a;
}

// both launches of the pair kernel over the list in a.pairs; the work area of the second is sized for a target of
// `max_target` nodes against a query of `max_query`
int fc_run_pairs(FillArgs &a, uint32_t max_target, uint32_t max_query, hipStream_t st) {
    if (!a.n_pairs) return 0;
    pair_kernel<false><<<jtk_blocks(a.n_pairs, 64 * FC_WAVES, FC_GRID), FC_WAVES * 64, FC_WAVES * FC_LDS_PER_WAVE, st>>>(a);
    JTK_HIP_TRY(hipGetLastError());
    const uint64_t need = (fc_need(max_target, max_query) + 7) & ~7ull;
    if (need > FC_LDS_PER_WAVE) {  // some pair may be too large for the LDS launch
        const uint32_t waves = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(FC_WORK_BYTES / need, 1), FC_LARGE_WAVES);
        DevArr<uint8_t> d_work;
        JTK_HIP_TRY(d_work.alloc(need * waves));
        a.work = d_work.get();
        a.work_stride = need;
        pair_kernel<true><<<waves, 64, 0, st>>>(a);
        JTK_HIP_TRY(hipGetLastError());
        JTK_HIP_TRY(hipStreamSynchronize(st));  // d_work goes with this scope
        a.work = nullptr;
    }
    return 0;
}

thread_local double g_fill_timing[4];  // pairs aligned, insertion records, device ms of the call, ms of the pair kernels

}  // namespace

extern "C" void jtk_lc_debug_fill_timing(double *out) {
    if (out) std::memcpy(out, g_fill_timing, sizeof(g_fill_timing));
}

extern "C" int jtk_lc_fill_candidates(size_t n_reads, const uint64_t *node_off, const jtk_fill_node_t *nodes, const uint8_t *target,
                                      uint32_t *coverage, uint32_t *ins_thr, uint64_t *cand_off, jtk_fill_cand_t *cands, size_t cand_cap,
                                      size_t *n_cands, int device) {
    g_last_error.clear();
    if (int rc = fc_check(n_reads, node_off, nodes)) return rc;
    if (!coverage || !cand_off || !n_cands || (n_reads && !ins_thr)) return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    if (int rc = jtk_require_device(device)) return rc;
    Reads R;
    fc_index(R, n_reads, node_off, nodes, target);
    const uint64_t n_slots = (uint64_t)R.n_nodes + R.n_reads;
    DevStream s;
    JTK_HIP_TRY(s.create(4));
    const hipStream_t st = s.st;
    JTK_HIP_TRY(hipEventRecord(s.ev[0], st));
    if (int rc = fc_upload(R, node_off, st)) return rc;
    RocTemp tmp;
    // ---- 1. the pairs
    std::vector<uint64_t> rec_off((size_t)R.n_nodes + 1, 0);
    for (uint32_t e = 0; e < R.n_nodes; e++) {
        const bool is_target = !target || target[R.read_of[e]];
        rec_off[e + 1] = rec_off[e] + (is_target ? R.seg_start[R.kid[e] + 1] - R.seg_start[R.kid[e]] : 0u);
    }
    const uint64_t n_emit = rec_off[R.n_nodes];
    uint64_t n_pairs = 0;
    DevArr<uint64_t> d_pairs;
    if (n_emit) {
        DevArr<uint32_t> d_read_of, d_order, d_seg;
        DevArr<uint64_t> d_rec_off, d_raw, d_sorted, d_count;
        int rc;
        if ((rc = d_read_of.upload(R.read_of, st)) || (rc = d_order.upload(R.order, st)) || (rc = d_seg.upload(R.seg_start, st)) ||
            (rc = d_rec_off.upload(rec_off, st)))
            return jtk_fail(rc, "device upload failed");
        JTK_HIP_TRY(d_raw.alloc(n_emit));
        JTK_HIP_TRY(d_sorted.alloc(n_emit));
        JTK_HIP_TRY(d_pairs.alloc(n_emit));
        JTK_HIP_TRY(d_count.alloc(1));
        pair_emit_kernel<<<jtk_blocks(R.n_nodes, 4, 4096), 256, 0, st>>>(R.n_nodes, R.d_kid.cget(), d_read_of.cget(), d_order.cget(), d_seg.cget(),
                                                                        d_rec_off.cget(), d_raw.get());
        const unsigned end_bit = 32 + jtk_bits(R.n_reads);
        JTK_HIP_TRY(tmp.run([&](void *t, size_t &bytes) {
            return rocprim::radix_sort_keys(t, bytes, d_raw.cget(), d_sorted.get(), (size_t)n_emit, 0u, end_bit, st);
        }));
        JTK_HIP_TRY(tmp.run([&](void *t, size_t &bytes) {
            return rocprim::unique(t, bytes, d_sorted.cget(), d_pairs.get(), d_count.get(), (size_t)n_emit, rocprim::equal_to<uint64_t>(), st);
        }));
        JTK_HIP_TRY(d_count.download(&n_pairs, 1, st));
        JTK_HIP_TRY(hipStreamSynchronize(st));
        JTK_HIP_TRY(hipGetLastError());
    }
    // ---- 2. the pair kernel; the record list is sized by a guess and the launches repeat once if it was too small
    DevArr<uint32_t> d_cov;
    DevArr<uint64_t> d_hi, d_lo;
    DevArr<int64_t> d_val;
    DevArr<unsigned long long> d_rec_count;
    JTK_HIP_TRY(d_cov.alloc(n_slots));
    JTK_HIP_TRY(d_rec_count.alloc(1));
    uint64_t rec_cap = 4 * n_pairs + 1024, n_rec = 0;
    float pair_ms = 0.f;
    for (int attempt = 0;; attempt++) {
        JTK_HIP_TRY(d_hi.alloc(rec_cap));
        JTK_HIP_TRY(d_lo.alloc(rec_cap));
        JTK_HIP_TRY(d_val.alloc(rec_cap));
        JTK_HIP_TRY(d_cov.zero(n_slots, st));
        JTK_HIP_TRY(d_rec_count.zero(1, st));
        FillArgs a = fc_args(R, n_pairs, d_pairs.cget());
        a.coverage = d_cov.get();
        a.rec_hi = d_hi.get();
        a.rec_lo = d_lo.get();
        a.rec_val = d_val.get();
        a.rec_cap = rec_cap;
        a.rec_count = d_rec_count.get();
        JTK_HIP_TRY(hipEventRecord(s.ev[1], st));
        if (int rc = fc_run_pairs(a, R.max_target_nodes, R.max_nodes, st)) return rc;
        JTK_HIP_TRY(hipEventRecord(s.ev[2], st));
        unsigned long long got = 0;
        JTK_HIP_TRY(d_rec_count.download(&got, 1, st));
        JTK_HIP_TRY(hipStreamSynchronize(st));
        JTK_HIP_TRY(hipGetLastError());
        JTK_HIP_TRY(s.elapsed(1, 2, &pair_ms));
        n_rec = got;
        if (n_rec <= rec_cap) break;
        if (attempt) return jtk_fail(JTK_ERR_CHUNK_FAILED, "the insertion records changed between two runs");
        rec_cap = n_rec;
    }
    if (n_rec >= 0xffffffffull) return jtk_fail(JTK_ERR_UNSUPPORTED, "2^32 - 1 or more insertion records");
    // ---- 3. thresholds, the records in order, the candidates
    DevArr<uint32_t> d_thr, d_per_read;
    JTK_HIP_TRY(d_thr.alloc(R.n_reads));
    JTK_HIP_TRY(d_per_read.alloc(R.n_reads));
    JTK_HIP_TRY(d_per_read.zero(std::max<size_t>(R.n_reads, 1), st));
    ins_thr_kernel<<<jtk_blocks(R.n_reads, 256, 4096), 256, 0, st>>>(R.n_reads, R.d_off.cget(), d_cov.cget(), d_thr.get());
    uint64_t total = 0;
    DevArr<jtk_fill_cand_t> d_cands;
    std::vector<uint32_t> per_read(R.n_reads, 0);
    if (n_rec) {
        DevArr<uint32_t> d_iota, d_perm1, d_perm, d_flag, d_pos;
        DevArr<uint64_t> d_lo_s, d_hi_g, d_hi_s, d_key_chunk, d_key_cluster;
        int rc;
        if ((rc = d_key_chunk.upload(R.key_chunk, st)) || (rc = d_key_cluster.upload(R.key_cluster, st))) return jtk_fail(rc, "device upload failed");
        JTK_HIP_TRY(d_iota.alloc(n_rec));
        JTK_HIP_TRY(d_perm1.alloc(n_rec));
        JTK_HIP_TRY(d_perm.alloc(n_rec));
        JTK_HIP_TRY(d_lo_s.alloc(n_rec));
        JTK_HIP_TRY(d_hi_g.alloc(n_rec));
        JTK_HIP_TRY(d_hi_s.alloc(n_rec));
        JTK_HIP_TRY(d_flag.alloc(n_rec + 1));
        JTK_HIP_TRY(d_pos.alloc(n_rec + 1));
        const uint32_t rec_grid = jtk_blocks(n_rec, 256, 4096);
        fc_iota_kernel<<<rec_grid, 256, 0, st>>>(n_rec, d_iota.get());
        const unsigned lo_bits = 2 + jtk_bits(R.n_keys), hi_bits = 17 + jtk_bits(R.n_reads);
        // least significant part first; both sorts are stable.  Bit 0 of lo (an offset is present) is no part of the key.
        JTK_HIP_TRY(tmp.run([&](void *t, size_t &bytes) {
            return rocprim::radix_sort_pairs(t, bytes, d_lo.cget(), d_lo_s.get(), d_iota.cget(), d_perm1.get(), (size_t)n_rec, 1u, lo_bits, st);
        }));
        fc_gather_kernel<<<rec_grid, 256, 0, st>>>(n_rec, d_perm1.cget(), d_hi.cget(), d_hi_g.get());
        JTK_HIP_TRY(tmp.run([&](void *t, size_t &bytes) {
            return rocprim::radix_sort_pairs(t, bytes, d_hi_g.cget(), d_hi_s.get(), d_perm1.cget(), d_perm.get(), (size_t)n_rec, 0u, hi_bits, st);
        }));
        auto summarise = [&](int write) {
            summarise_kernel<<<rec_grid, 256, 0, st>>>(n_rec, d_hi_s.cget(), d_lo.cget(), d_perm.cget(), d_val.cget(), R.d_off.cget(), R.d_start.cget(),
                                                       R.d_end.cget(), d_thr.cget(), d_key_chunk.cget(), d_key_cluster.cget(), write, d_flag.get(),
                                                       d_pos.cget(), d_cands.get(), d_per_read.get());
        };
        JTK_HIP_TRY(d_flag.zero(n_rec + 1, st));
        summarise(0);
        JTK_HIP_TRY(tmp.run([&](void *t, size_t &bytes) {
            return rocprim::exclusive_scan(t, bytes, d_flag.cget(), d_pos.get(), 0u, (size_t)n_rec + 1, rocprim::plus<uint32_t>(), st);
        }));
        uint32_t total32 = 0;
        JTK_HIP_TRY(d_pos.download(&total32, 1, st, n_rec));
        JTK_HIP_TRY(hipStreamSynchronize(st));
        JTK_HIP_TRY(hipGetLastError());
        total = total32;
        if (total) {
            JTK_HIP_TRY(d_cands.alloc(total));
            summarise(1);
            JTK_HIP_TRY(d_per_read.download(per_read.data(), R.n_reads, st));
            JTK_HIP_TRY(hipStreamSynchronize(st));
            JTK_HIP_TRY(hipGetLastError());
        }
    }
    if (total > cand_cap || (total && !cands)) {
        *n_cands = total;
        return jtk_fail(JTK_ERR_INVALID_ARG, "cand_cap is too small (*n_cands holds the need)");
    }
    std::vector<uint32_t> cov_v(n_slots), thr_v(R.n_reads);
    std::vector<jtk_fill_cand_t> cand_v(total);
    JTK_HIP_TRY(d_cov.download(cov_v.data(), n_slots, st));
    if (R.n_reads) JTK_HIP_TRY(d_thr.download(thr_v.data(), R.n_reads, st));
    if (total) JTK_HIP_TRY(d_cands.download(cand_v.data(), total, st));
    JTK_HIP_TRY(hipEventRecord(s.ev[3], st));
    JTK_HIP_TRY(hipStreamSynchronize(st));
    JTK_HIP_TRY(hipGetLastError());
    float ms = 0.f;
    JTK_HIP_TRY(s.elapsed(0, 3, &ms));
    g_fill_timing[0] = (double)n_pairs;
    g_fill_timing[1] = (double)n_rec;
    g_fill_timing[2] = ms;
    g_fill_timing[3] = pair_ms;
    std::copy(cov_v.begin(), cov_v.end(), coverage);
    std::copy(thr_v.begin(), thr_v.end(), ins_thr);
    cand_off[0] = 0;
    for (uint32_t r = 0; r < R.n_reads; r++) cand_off[r + 1] = cand_off[r] + per_read[r];
    if (total) std::memcpy(cands, cand_v.data(), total * sizeof(jtk_fill_cand_t));
    *n_cands = total;
    return 0;
}

extern "C" int jtk_lc_debug_fill_pairs(size_t n_reads, const uint64_t *node_off, const jtk_fill_node_t *nodes, size_t n_pairs,
                                       const uint32_t *pair_target, const uint32_t *pair_query, int32_t *dir, int32_t *score, uint8_t *pass,
                                       uint64_t *ops_off, uint32_t *ops, size_t ops_cap, size_t *n_ops, int device) {
    g_last_error.clear();
    if (int rc = fc_check(n_reads, node_off, nodes)) return rc;
    if (!ops_off || !n_ops || (n_pairs && (!pair_target || !pair_query || !dir || !score || !pass))) return jtk_fail(JTK_ERR_INVALID_ARG, "null argument");
    if (n_pairs >= 0x7fffffffu) return jtk_fail(JTK_ERR_UNSUPPORTED, "2^31 - 1 pairs or more");
    std::vector<uint64_t> pairs(n_pairs), slot_off(n_pairs + 1, 0);
    uint32_t max_t = 0, max_q = 0;
    for (size_t p = 0; p < n_pairs; p++) {
        if (pair_target[p] >= n_reads || pair_query[p] >= n_reads) return jtk_fail(JTK_ERR_INVALID_ARG, "a pair names a read that is not there");
        const uint32_t n = (uint32_t)(node_off[pair_target[p] + 1] - node_off[pair_target[p]]);
        const uint32_t m = (uint32_t)(node_off[pair_query[p] + 1] - node_off[pair_query[p]]);
        pairs[p] = (uint64_t)pair_target[p] << 32 | pair_query[p];
        slot_off[p + 1] = slot_off[p] + n + m + 2;
        max_t = std::max(max_t, n);
        max_q = std::max(max_q, m);
    }
    if (int rc = jtk_require_device(device)) return rc;
    Reads R;
    fc_index(R, n_reads, node_off, nodes, nullptr);
    DevStream s;
    JTK_HIP_TRY(s.create());
    const hipStream_t st = s.st;
    if (int rc = fc_upload(R, node_off, st)) return rc;
    DevArr<uint64_t> d_pairs, d_slot_off;
    DevArr<int32_t> d_dir, d_score;
    DevArr<uint8_t> d_pass;
    DevArr<uint32_t> d_ops, d_nops;
    {
        int rc;
        if ((rc = d_pairs.upload(pairs, st)) || (rc = d_slot_off.upload(slot_off, st))) return jtk_fail(rc, "device upload failed");
    }
    JTK_HIP_TRY(d_dir.alloc(n_pairs));
    JTK_HIP_TRY(d_score.alloc(n_pairs));
    JTK_HIP_TRY(d_pass.alloc(n_pairs));
    JTK_HIP_TRY(d_nops.alloc(n_pairs));
    JTK_HIP_TRY(d_ops.alloc(slot_off[n_pairs]));
    FillArgs a = fc_args(R, n_pairs, d_pairs.cget());
    a.dbg_dir = d_dir.get();
    a.dbg_score = d_score.get();
    a.dbg_pass = d_pass.get();
    a.dbg_ops = d_ops.get();
    a.dbg_nops = d_nops.get();
    a.dbg_ops_off = d_slot_off.cget();
    if (int rc = fc_run_pairs(a, max_t, max_q, st)) return rc;
    std::vector<int32_t> dir_v(n_pairs), score_v(n_pairs);
    std::vector<uint8_t> pass_v(n_pairs);
    std::vector<uint32_t> nops_v(n_pairs), ops_v(slot_off[n_pairs]);
    if (n_pairs) {
        JTK_HIP_TRY(d_dir.download(dir_v.data(), n_pairs, st));
        JTK_HIP_TRY(d_score.download(score_v.data(), n_pairs, st));
        JTK_HIP_TRY(d_pass.download(pass_v.data(), n_pairs, st));
        JTK_HIP_TRY(d_nops.download(nops_v.data(), n_pairs, st));
        JTK_HIP_TRY(d_ops.download(ops_v.data(), ops_v.size(), st));
    }
    JTK_HIP_TRY(hipStreamSynchronize(st));
    JTK_HIP_TRY(hipGetLastError());
    uint64_t total = 0;
    for (size_t p = 0; p < n_pairs; p++) total += nops_v[p];
    if (total > ops_cap || (total && !ops)) {
        *n_ops = total;
        return jtk_fail(JTK_ERR_INVALID_ARG, "ops_cap is too small (*n_ops holds the need)");
    }
    ops_off[0] = 0;
    for (size_t p = 0; p < n_pairs; p++) {
        std::copy(ops_v.begin() + slot_off[p], ops_v.begin() + slot_off[p] + nops_v[p], ops + ops_off[p]);
        ops_off[p + 1] = ops_off[p] + nops_v[p];
    }
    std::copy(dir_v.begin(), dir_v.end(), dir);
    std::copy(score_v.begin(), score_v.end(), score);
    std::copy(pass_v.begin(), pass_v.end(), pass);
    *n_ops = total;
    return 0;
}
