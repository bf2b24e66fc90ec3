// kmer_plan.h -- the host arithmetic of the k-mer primitives (mask.hip, map.hip), without HIP: how a list of sequences is cut
// into the tiles their kernels take one workgroup each, where every sequence's k-mers go, and the bits of a sort key's field.
// The kernels trust the tile table blindly, so it is kept where a plain C++ compiler and a sanitizer reach it
// (tests/test_kmer_plan.py).  No global state, no environment.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

// bits that hold 0 ..= largest: its bit length, at least 1
inline uint32_t jtk_bits(uint64_t largest) {
    uint32_t b = 1;
    while (b < 64 && (largest >> b)) b++;
    return b;
}

// what a tile counts, and so which sequences have tiles at all
enum KmerTileUnit {
    KMER_TILE_BASES,      // tiles start at multiples of `tile` below len: a sequence shorter than k still has tiles
    KMER_TILE_POSITIONS,  // tiles start at multiples of `tile` below the k-mer positions, max(len - k + 1, 0)
};

// Tile t is the `tile` units from tile_start[t] of sequence tile_seq[t]; a sequence's tiles are adjacent and ascending, the
// sequences in their order.  kmer_off is the prefix sum of the k-mer positions, n + 1 entries; n_kmers its last.
struct KmerPlan {
    uint64_t n_kmers = 0;
    std::vector<uint64_t> kmer_off;
    std::vector<uint32_t> tile_seq, tile_start;
};

// off: n + 1 offsets that start at 0 and never decrease, below 2^32 (the callers have checked them)
inline KmerPlan jtk_plan_kmers(size_t n, const uint64_t *off, uint32_t k, uint32_t tile, KmerTileUnit unit) {
    KmerPlan P;
    P.kmer_off.assign(n + 1, 0);
    for (size_t r = 0; r < n; r++) {
        const uint64_t len = off[r + 1] - off[r], n_pos = len >= k ? len - k + 1 : 0;
        P.kmer_off[r + 1] = P.kmer_off[r] + n_pos;
        for (uint64_t s = 0; s < (unit == KMER_TILE_BASES ? len : n_pos); s += tile) {
            P.tile_seq.push_back((uint32_t)r);
            P.tile_start.push_back((uint32_t)s);
        }
    }
    P.n_kmers = P.kmer_off[n];
    return P;
}
