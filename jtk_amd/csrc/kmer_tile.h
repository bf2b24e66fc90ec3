// kmer_tile.h -- what a workgroup of the k-mer primitives (mask.hip, map.hip) does with its tile of a sequence: stage the bytes in
// LDS, pack them into bit streams, take a window out of a stream as a bit field, search a sorted list.  A stream of WORDS words
// is followed by zero words, as many as a field's last read goes past its first (2 for the 2-bit stream, 1 for the 1-bit one):
// a field may start in the last word of the stream, and what it then reads behind the stream is 0, not another array.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// base i of a k-mer sits at bits 2i: A C G T = 0 1 2 3, and every other byte is 0 too
__device__ __forceinline__ uint32_t jtk_base_code(uint32_t b) {
    const uint32_t u = b & 0xdfu;  // folds the two cases of a letter; no other byte becomes A, C, G or T
    return u == 'C' ? 1u : u == 'G' ? 2u : u == 'T' ? 3u : 0u;
}
// the complement's code: A C G T = 3 2 1 0, and every other byte is 0 here as well -- NOT 3 - jtk_base_code(b)
__device__ __forceinline__ uint32_t jtk_base_complement(uint32_t b) {
    const uint32_t u = b & 0xdfu;
    return u == 'A' ? 3u : u == 'C' ? 2u : u == 'G' ? 1u : 0u;
}
// the validity a 2-bit code lacks: 1 where the byte is none of A, C, G, T in either case
__device__ __forceinline__ uint32_t jtk_no_base(uint8_t b) {
    const uint32_t u = b & 0xdfu;
    return u == 'A' || u == 'C' || u == 'G' || u == 'T' ? 0u : 1u;
}

// raw[i] = seq[a + i] for i < BYTES, 0 behind the sequence's end (a < len), by the whole workgroup: consecutive lanes load
// consecutive bytes.  No barrier: the caller has one before anybody reads raw.
template <uint32_t BYTES, uint32_t THREADS>
__device__ __forceinline__ void jtk_stage_bytes(uint8_t *raw, const uint8_t *seq, uint32_t len, uint32_t a) {
    const uint32_t left = len - a;
    for (uint32_t i = threadIdx.x; i < BYTES; i += THREADS) raw[i] = i < left ? seq[(uint64_t)a + i] : (uint8_t)0;
}

// words[s][0 .. WORDS + 2) of every stream s: its code(i) of the local indices i < 16 * WORDS, 16 to a word, and the two zero
// words.  The streams of one call share the loop (mask.hip packs its two strands in one pass over the words).
template <uint32_t WORDS, uint32_t THREADS, typename... Code>
__device__ __forceinline__ void jtk_pack2(uint32_t *const (&words)[sizeof...(Code)], Code... code) {
    for (uint32_t w = threadIdx.x; w < WORDS + 2; w += THREADS) {
        uint32_t v[sizeof...(Code)] = {};
        if (w < WORDS) {
#pragma unroll
            for (uint32_t i = 0; i < 16; i++) {
                uint32_t s = 0;
                ((v[s++] |= code(16 * w + i) << (2 * i)), ...);
            }
        }
        for (uint32_t s = 0; s < sizeof...(Code); s++) words[s][w] = v[s];
    }
}

// words[0 .. WORDS + 1): bit(i), 0u or 1u, of the local indices i < 32 * WORDS, 32 to a word, and the zero word
template <uint32_t WORDS, uint32_t THREADS, typename Bit>
__device__ __forceinline__ void jtk_pack1(uint32_t *words, Bit bit) {
    for (uint32_t w = threadIdx.x; w < WORDS + 1; w += THREADS) {
        uint32_t v = 0;
        if (w < WORDS) {
#pragma unroll
            for (uint32_t i = 0; i < 32; i++) v |= bit(32 * w + i) << i;
        }
        words[w] = v;
    }
}

// k <= 31 codes from position pos of a 2-bit stream: three words, two shifts
__device__ __forceinline__ uint64_t jtk_field2(const uint32_t *words, uint32_t pos, uint32_t k) {
    const uint32_t w = pos >> 4, s = (pos & 15u) * 2;
    uint64_t v = ((uint64_t)words[w] | ((uint64_t)words[w + 1] << 32)) >> s;
    if (s) v |= (uint64_t)words[w + 2] << (64 - s);
    return v & ((1ull << (2 * k)) - 1);
}

// k <= 31 bits from position pos of a 1-bit stream: two words, one shift
__device__ __forceinline__ uint32_t jtk_field1(const uint32_t *words, uint32_t pos, uint32_t k) {
    const uint32_t w = pos >> 5, s = pos & 31u;
    const uint64_t v = ((uint64_t)words[w] | ((uint64_t)words[w + 1] << 32)) >> s;
    return (uint32_t)v & ((1u << k) - 1);
}

// the first index of the ascending list whose entry is not below x; n where there is none
template <typename T>
__device__ __forceinline__ uint64_t jtk_lower_bound(const T *list, uint64_t n, T x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (list[mid] < x)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}
