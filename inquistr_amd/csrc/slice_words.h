// slice_words.h — a packed slice read 16 bases at a time: what the kernels that compare a record's bases share (read_motif_kernel of
// read_motifs.hip, locus_motif_kernel of locus_motifs.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace inq {

constexpr uint64_t kNibbleOnes = 0x1111111111111111ull;

// Bytes [8 w, 8 w + 8) of a segment of nb bytes as a little-endian word, cut to the segment: a byte at or past nb is 0 and is not read.
// The segment starts wherever its slice does, so the loads are unaligned ones
__device__ __forceinline__ uint64_t load_segment_word(const uint8_t *seg, uint64_t nb, uint64_t w) {
    const uint64_t o = w * 8u;
    uint64_t v = 0;
    if (o >= nb) return v;
    if (nb - o >= 8u) {
        __builtin_memcpy(&v, seg + o, 8);
        return v;
    }
    for (uint32_t i = 0; i < (uint32_t)(nb - o); ++i) v |= (uint64_t)seg[o + i] << (8u * i);
    return v;
}

// a loaded word with base t of its sixteen in nibble t (the slice packs the earlier base of a byte into the high nibble)
__device__ __forceinline__ uint64_t bases_in_order(uint64_t s) {
    return (s & 0x0f0f0f0f0f0f0f0full) << 4 | (s >> 4 & 0x0f0f0f0f0f0f0f0full);
}

// bit t of the result: nibble t of x is zero
__device__ __forceinline__ uint32_t zero_nibbles(uint64_t x) {
    uint64_t t = ~x;
    t &= t >> 1;
    t &= t >> 2;
    t &= kNibbleOnes;  // bit 4 t: nibble t was all ones
    t = (t | t >> 3) & 0x0303030303030303ull;
    t = (t | t >> 6) & 0x000f000f000f000full;
    t = (t | t >> 12) & 0x000000ff000000ffull;
    return (uint32_t)(t | t >> 24) & 0xffffu;
}

// the number of set bits in each nibble of x, nibble by nibble (0 .. 4)
__device__ __forceinline__ uint64_t nibble_popcounts(uint64_t x) {
    return (x & kNibbleOnes) + (x >> 1 & kNibbleOnes) + (x >> 2 & kNibbleOnes) + (x >> 3 & kNibbleOnes);
}

// a motif word of inq_read_motif_t names a motif: k = nibble 15 is not 0 and each of nibbles 0 .. k - 1 is one of 1, 2, 4, 8
__device__ __forceinline__ bool motif_word_ok(uint64_t word) {
    const uint32_t k = (uint32_t)(word >> 60);
    if (!k) return false;
    const uint64_t mask = ~0ull >> (64u - 4u * k);
    return nibble_popcounts(word & mask) == (kNibbleOnes & mask);
}

}  // namespace inq
