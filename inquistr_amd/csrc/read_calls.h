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
    uint64_t *kept_pair = nullptr;   // [n_pairs] or null: the pair each record came from (what the slices of read_seqs.hip are indexed by)
};

inline uint64_t read_call_tiles(uint64_t n_pairs) { return (n_pairs + kReadCallTile - 1) / kReadCallTile; }
// the tile arrays of a batch of n_pairs pairs: tile_base first (8-byte entries), tile_count behind it
inline size_t read_call_scratch_bytes(uint64_t n_pairs) { return (size_t)(read_call_tiles(n_pairs) + 1) * 8 + (size_t)read_call_tiles(n_pairs) * 4; }

// the three launches on s (a.n_pairs > 0; a batch without pairs is a fill of kept_off, done by the caller)
void launch_read_calls(const ReadCallArgs &a, bool unphased, hipStream_t s);

// ---- read_names.hip: the names and origins of the kept reads (inq_read_origin_t)
constexpr uint32_t kReadNameLanes = 8;                    // lanes that share one segment of the byte gather
constexpr uint32_t kReadNameTile = 256 / kReadNameLanes;  // segments per workgroup (inq_read_name_tile)
constexpr uint32_t kReadNameMax = 254;                    // l_read_name is a byte and counts the terminator

// The segmented byte gather: segment i copies dst_off[i + 1] - dst_off[i] bytes from src + src_off[r] + src_add to dst + dst_off[i],
// r = index[i].read, or index64[i] (a plain index: the kept records' pairs), or i where both are null.  dst_off is an exclusive prefix
// sum ([n + 1]).  A segment is cut to [dst, dst + dst_bytes) and to [src, src + src_bytes); r >= n_src copies nothing.
struct NameCopyArgs {
    const uint8_t *src;
    uint64_t src_bytes;
    const uint64_t *src_off;       // [n_src]
    uint64_t n_src, src_add;
    const inq_read_call_t *index;  // [n] or null
    uint8_t *dst;
    uint64_t dst_bytes;
    const uint64_t *dst_off;       // [n + 1]
    uint64_t n;
    const uint64_t *index64 = nullptr;  // [n] or null; read where index is null
};
void launch_name_copy(const NameCopyArgs &a, uint32_t grid_side, hipStream_t s);  // n == 0 launches nothing

// one inq_read_origin_t per record the compaction wrote, k < min(*n_kept, n_pairs): reads[kept[k].read] and that read's name length
struct ReadOriginArgs {
    const inq_read_call_t *kept;
    const uint64_t *n_kept;      // DEVICE: kept_off[n_loci]
    const uint32_t *read_words;  // inq_read_t as four words (PairView::read_words)
    uint64_t n_reads;
    const uint64_t *name_off;    // [n_reads + 1] the batch's names
    inq_read_origin_t *origins;  // [n_pairs], 8-byte aligned
    uint64_t n_pairs;
};
void launch_read_origins(const ReadOriginArgs &a, uint32_t grid_side, hipStream_t s);

}  // namespace inq
