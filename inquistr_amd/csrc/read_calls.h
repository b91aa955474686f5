// read_calls.h — the compaction kernels behind inq_read_call_t (read_calls.hip), launched by capi.hip behind the locus kernels
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/inquistr_hip.h"
#include "pair_view.h"

namespace inq {

constexpr uint32_t kReadCallTile = 4096;  // pairs per workgroup of the count and the scatter launch: 16 B of pair_bits per lane

struct ReadCallArgs : PairView {
    uint64_t *kept_off;              // [n_loci + 1]
    inq_read_call_t *kept;           // [n_pairs]: records [0, kept_off[n_loci]) are written, 16-byte aligned
    uint32_t *tile_count;            // [n_tiles]      context scratch
    uint64_t *tile_base;             // [n_tiles + 1]  context scratch; the last entry is the total
};

inline uint64_t read_call_tiles(uint64_t n_pairs) { return (n_pairs + kReadCallTile - 1) / kReadCallTile; }
// the tile arrays of a batch of n_pairs pairs: tile_base first (8-byte entries), tile_count behind it
inline size_t read_call_scratch_bytes(uint64_t n_pairs) { return (size_t)(read_call_tiles(n_pairs) + 1) * 8 + (size_t)read_call_tiles(n_pairs) * 4; }

// the three launches on s (a.n_pairs > 0; a batch without pairs is a fill of kept_off, done by the caller)
void launch_read_calls(const ReadCallArgs &a, bool unphased, hipStream_t s);

}  // namespace inq
