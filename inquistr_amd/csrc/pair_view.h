// pair_view.h — what the kernels behind the locus kernels (evidence.hip, read_calls.hip) read of a called batch
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace inq {

// the batch's pairs and what the locus kernels wrote for each; capi.hip fills one per call, both argument structs begin with it
struct PairView {
    const uint64_t *locus_pair_off;  // [n_loci + 1]
    const uint8_t *pair_bits;        // [n_pairs] INQ_PAIR_*, as the locus kernels left them
    const int64_t *pair_call;        // [n_pairs]
    const uint32_t *pair_read;       // [n_pairs]
    const uint32_t *read_words;      // inq_read_t as four words: word 3 = mapq | bits << 8 | phase << 16 | promise << 24  (phased only)
    uint64_t n_reads, n_pairs, n_loci;
};

// The HP of read r, the phased group of a kept pair.  (An index outside the descriptors is the locus kernels' INQ_ERR_INDEX: nothing
// is read through it here, the pair belongs to no group.)
__device__ __forceinline__ uint32_t phase_group(const PairView &v, uint32_t r) {
    return r < v.n_reads ? (v.read_words[4 * (uint64_t)r + 3] >> 16) & 0xffu : 0u;
}

}  // namespace inq
