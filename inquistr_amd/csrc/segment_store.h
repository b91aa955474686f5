// segment_store.h — what the segmented byte gathers share (name_copy_kernel of read_names.hip, seq_slice_kernel of read_seqs.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace inq {

// The kLanes lanes of a segment (this one is `sub`) store its len bytes at dst as aligned words of the DESTINATION: [0, head) up to the
// destination's first word boundary, then n_words whole words strided over the lanes, then what is left (< 4 bytes).  The up to three
// bytes in front of the first whole word and behind the last go one by one, since the word they lie in is shared with the neighbouring
// segment, whose lanes write it at the same time.  byte_at(d) / word_at(d): the byte / the four bytes (little-endian) that belong at
// dst + d; the caller has cut len to what the destination and the source hold.
template <uint32_t kLanes, class ByteAt, class WordAt>
__device__ __forceinline__ void store_segment(uint8_t *dst, uint64_t len, uint32_t sub, ByteAt byte_at, WordAt word_at) {
    uint64_t head = (4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u;
    if (head > len) head = len;
    const uint64_t n_words = (len - head) / 4u, tail = head + n_words * 4u;
    if (sub < head) dst[sub] = byte_at(sub);
    for (uint64_t w = sub; w < n_words; w += kLanes) {
        const uint64_t d = head + w * 4u;
        *reinterpret_cast<uint32_t *>(dst + d) = word_at(d);
    }
    if (tail + sub < len) dst[tail + sub] = byte_at(tail + sub);
}

}  // namespace inq
