// read_names.hip — the names (QNAME) and origins of the reads behind the per-read Calls (inq_read_origin_t): a segmented byte gather.
//
// A record's name lives only in the inflated bytes of a span slot, which a later span reuses, so it is gathered twice:
//   span time   out of the inflated bytes (rec_off[i] + 36) into the deferred batch's names, behind cigar_gather_kernel
//   flush time  for the kept records only, out of the batch's names into context scratch, behind read_call_scatter: what crosses
//               PCIe is proportional to the table, not to the BAM
// Both are ONE kernel, name_copy_kernel, over (source offset, destination offset, length) triples.  The destination offsets are an
// exclusive prefix sum of the lengths (bam_scan.hip's scan templates through LoadNameLen / LoadRunBytes), so segment i's length is
// dst_off[i + 1] - dst_off[i] and the segments tile the destination without gap or overlap.
//
// Layout: kReadNameLanes = 8 lanes per segment, 32 segments per 256-thread workgroup (kReadNameTile).  A name is 0 - 254 bytes,
// typically 10 - 60: a wave per segment would leave 50 of 64 lanes idle, a lane per segment would serialise 60 dependent byte
// moves.  Eight lanes move 32 bytes a step as aligned words of the DESTINATION (store_segment of segment_store.h; the source is read
// with unaligned word loads).  No atomics, no LDS, no workgroup waits for another; every output byte is a plain function of the inputs.
//
// Bounds hold whatever the offsets and lengths are: a segment is cut to what the destination and the source hold before a byte of
// it moves, and an index outside the source's offsets copies nothing.
#include <hip/hip_runtime.h>

#include "kept_view.h"
#include "read_calls.h"
#include "segment_store.h"

namespace inq {
namespace {

constexpr uint32_t kThreads = 256;
static_assert(kReadNameTile * kReadNameLanes == kThreads, "a workgroup's lanes are dealt among its segments");
static_assert(sizeof(inq_read_origin_t) == 8, "an origin is one 8-byte store");

__global__ __launch_bounds__(256) void name_copy_kernel(NameCopyArgs a) {
    const uint32_t sub = threadIdx.x % kReadNameLanes;
    // (the grid is capped, launch_name_copy: a workgroup takes every gridDim.x-th tile)
    for (uint64_t i = (uint64_t)blockIdx.x * kReadNameTile + threadIdx.x / kReadNameLanes; i < a.n; i += (uint64_t)gridDim.x * kReadNameTile) {
        const uint64_t d0 = a.dst_off[i];
        uint64_t d1 = a.dst_off[i + 1];
        if (d1 > a.dst_bytes) d1 = a.dst_bytes;
        if (d0 >= d1) continue;  // an empty name (or offsets that do not ascend): nothing moves
        const uint64_t r = a.index ? (uint64_t)a.index[i].read : a.index64 ? a.index64[i] : i;
        if (r >= a.n_src) continue;
        const uint64_t s0 = a.src_off[r] + a.src_add;
        if (s0 >= a.src_bytes) continue;
        uint64_t len = d1 - d0;
        if (len > a.src_bytes - s0) len = a.src_bytes - s0;
        const uint8_t *src = a.src + s0;
        store_segment<kReadNameLanes>(
            a.dst + d0, len, sub, [&](uint64_t d) { return src[d]; },
            [&](uint64_t d) {
                uint32_t v;
                __builtin_memcpy(&v, src + d, 4);  // the source lies wherever the record does
                return v;
            });
    }
}

__global__ __launch_bounds__(256) void read_origin_kernel(ReadOriginArgs a) {
    const uint64_t total = kept_total(a.n_kept, a.n_pairs);
    for (uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x; k < total; k += (uint64_t)gridDim.x * kThreads) {
        const uint32_t r = a.kept[k].read;
        uint32_t pos = 0, tail = 0;  // (an index outside the descriptors is the locus kernels' INQ_ERR_INDEX: the record is all zero)
        if (r < a.n_reads) {
            const uint64_t len = a.name_off[r + 1] - a.name_off[r];
            pos = a.read_words[4 * (uint64_t)r + 2];
            // mapq | bits << 8 of the descriptor's last word, name_len behind them: the 8 bytes of inq_read_origin_t in one store
            tail = (a.read_words[4 * (uint64_t)r + 3] & 0xffffu) | (uint32_t)(len < kReadNameMax ? len : kReadNameMax) << 16;
        }
        *reinterpret_cast<uint2 *>(a.origins + k) = make_uint2(pos, tail);
    }
}

constexpr uint32_t kNameGridCap = 1u << 20;  // workgroups of a launch of this file (side_grid), not the shared kGridCap

}  // namespace

void launch_name_copy(const NameCopyArgs &a, uint32_t grid_side, hipStream_t s) {
    if (!a.n) return;
    hipLaunchKernelGGL(name_copy_kernel, dim3(side_grid((a.n + kReadNameTile - 1) / kReadNameTile, grid_side, kNameGridCap)), dim3(kThreads), 0, s, a);
}

void launch_read_origins(const ReadOriginArgs &a, uint32_t grid_side, hipStream_t s) {
    if (!a.n_pairs) return;
    hipLaunchKernelGGL(read_origin_kernel, dim3(side_grid((a.n_pairs + kThreads - 1) / kThreads, grid_side, kNameGridCap)), dim3(kThreads), 0, s, a);
}

}  // namespace inq
