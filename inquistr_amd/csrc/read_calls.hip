// read_calls.hip — the per-read Calls behind each row (inq_read_call_t): an order-preserving compaction of the kept pairs.
//
// The pairs of a batch are CSR: locus j owns [locus_pair_off[j], locus_pair_off[j + 1]).  A flat compaction of the INQ_PAIR_KEPT flags
// over all n_pairs therefore already yields the per-locus lists in file order, and kept_off[j] is the number of kept pairs in front of
// pair locus_pair_off[j].  Nothing here depends on a locus's depth: a locus of a million reads is simply 245 tiles.
//
// Three launches behind the locus kernels (and the evidence launches), reading only what those wrote; no workgroup waits for another.
//   read_call_count    one workgroup per tile of kReadCallTile pairs: 16 B of pair_bits per lane, the tile's kept pairs -> tile_count
//   read_call_scan     one workgroup: exclusive scan of tile_count into tile_base (u64), 256 tiles per step with a carry, and the total
//   read_call_scatter  one workgroup per tile: the exclusive prefix of every position (wave scan of the lanes' counts, wave totals
//                      through LDS) is kept in LDS as u16; the kept pairs are then stored position by position, so that neighbouring
//                      lanes read neighbouring pairs and write neighbouring records (one 16-byte store each), all loads of a lane's
//                      16 positions in flight together.  The loci whose first pair
//                      lies in the tile are found by one search on locus_pair_off (256 probes per step, by the whole workgroup) and
//                      take their kept_off from the same prefix; the last tile also serves the loci that begin at n_pairs,
//                      kept_off[n_loci] among them.
#include <hip/hip_runtime.h>

#include "read_calls.h"
#include "wave_primitives.h"

namespace inq {
namespace {

constexpr uint32_t kThreads = 256, kPerLane = kReadCallTile / kThreads;
static_assert(kPerLane == 16, "a lane takes the 16 bytes of one load");
static_assert(kReadCallTile < 65536, "prefixes inside a tile are kept as u16");
constexpr uint32_t kKeptShift = 2;
static_assert(INQ_PAIR_KEPT == 1u << kKeptShift, "the kept bit of four pairs at once");

// pair_bits of the 16 pairs from p0 on, zero for pairs at and behind n
__device__ __forceinline__ uint4 load_bits16(const uint8_t *bits, uint64_t p0, uint64_t n) {
    if (p0 + kPerLane <= n && (((uintptr_t)(bits + p0)) & 15u) == 0) return *(const uint4 *)(bits + p0);
    uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        if (p0 + k < n) w0 |= (uint32_t)bits[p0 + k] << (8 * k);
        if (p0 + 4 + k < n) w1 |= (uint32_t)bits[p0 + 4 + k] << (8 * k);
        if (p0 + 8 + k < n) w2 |= (uint32_t)bits[p0 + 8 + k] << (8 * k);
        if (p0 + 12 + k < n) w3 |= (uint32_t)bits[p0 + 12 + k] << (8 * k);
    }
    return make_uint4(w0, w1, w2, w3);
}
// one bit per byte: the pair is kept
__device__ __forceinline__ uint32_t kept4(uint32_t w) { return (w >> kKeptShift) & 0x01010101u; }
__device__ __forceinline__ uint32_t kept_count(const uint4 &w) {
    return (uint32_t)(__popc(kept4(w.x)) + __popc(kept4(w.y)) + __popc(kept4(w.z)) + __popc(kept4(w.w)));
}

// The workgroup's exclusive prefix of x per thread and its total (all 256 threads must call; wtot: 4 words of LDS, free again after
// the barrier that follows the caller's next use)
__device__ __forceinline__ uint32_t block_exclusive(uint32_t x, uint32_t *wtot, uint32_t &total) {
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t inc = wave_inclusive_scan_u32(x);
    if (lane_id() == kWave - 1) wtot[wave] = inc;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t v = wtot[k];
        before += k < wave ? v : 0u;
        total += v;
    }
    return before + inc - x;
}

// The first j in [0, n) with off[j] >= key, n if there is none, searched by the whole workgroup (all 256 threads must call): 256 probes
// per step instead of one, so 100 000 offsets take three round trips to memory, not seventeen - a tile's workgroup has little else
// to hide them behind.  wcnt: 4 words of LDS nobody else uses meanwhile.  Offsets that do not ascend end the search all the same,
// somewhere in [0, n].
__device__ __forceinline__ uint64_t block_lower_bound(const uint64_t *off, uint64_t n, uint64_t key, uint32_t *wcnt) {
    uint64_t lo = 0, hi = n;  // the answer lies in [lo, hi]; both are the same in every thread
    while (lo < hi) {
        const uint64_t step = (hi - lo + kThreads - 1) / kThreads;
        const uint64_t idx = lo + threadIdx.x * step;
        const bool below = idx < hi && off[idx] < key;  // (ascending offsets: true for the first c probes)
        const uint64_t m = ballot64(below);
        if (lane_id() == 0) wcnt[threadIdx.x >> 6] = (uint32_t)__popcll(m);
        __syncthreads();
        const uint32_t c = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();  // wcnt is free for the next step
        if (c == 0) {
            hi = lo;  // off[lo] >= key
        } else {
            const uint64_t last = lo + (uint64_t)(c - 1) * step;  // the last probe below the key (it lies in front of hi)
            lo = last + 1;
            hi = last + step < hi ? last + step : hi;
        }
    }
    return lo;
}

__global__ __launch_bounds__(256) void read_call_count(ReadCallArgs a) {
    __shared__ uint32_t wtot[4];
    const uint64_t p0 = (uint64_t)blockIdx.x * kReadCallTile + threadIdx.x * kPerLane;
    uint32_t total;
    (void)block_exclusive(kept_count(load_bits16(a.pair_bits, p0, a.n_pairs)), wtot, total);
    if (threadIdx.x == 0) a.tile_count[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void read_call_scan(ReadCallArgs a, uint64_t n_tiles) {
    __shared__ uint32_t wtot[4];
    uint64_t carry = 0;
    for (uint64_t base = 0; base < n_tiles; base += kThreads) {  // (256 tiles hold at most 2^20 kept pairs: u32 inside a step)
        const uint64_t i = base + threadIdx.x;
        uint32_t total;
        const uint32_t excl = block_exclusive(i < n_tiles ? a.tile_count[i] : 0u, wtot, total);
        if (i < n_tiles) a.tile_base[i] = carry + excl;
        carry += total;
        __syncthreads();  // wtot is free for the next step
    }
    if (threadIdx.x == 0) a.tile_base[n_tiles] = carry;
}

template <bool UNPHASED>
__global__ __launch_bounds__(256) void read_call_scatter(ReadCallArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t sbits[kReadCallTile];
    __shared__ uint16_t prefix[kReadCallTile + 1];  // kept pairs of the tile in front of each position; [kReadCallTile]: the tile's total
    __shared__ uint32_t wtot[4];
    const uint32_t tid = threadIdx.x;
    const uint64_t tile_start = (uint64_t)blockIdx.x * kReadCallTile;
    const uint64_t tile_end = a.n_pairs - tile_start < kReadCallTile ? a.n_pairs : tile_start + kReadCallTile;
    const bool last_tile = tile_end == a.n_pairs;

    const uint4 w = load_bits16(a.pair_bits, tile_start + tid * kPerLane, a.n_pairs);
    *(uint4 *)(sbits + tid * kPerLane) = w;
    uint32_t total;
    uint32_t run = block_exclusive(kept_count(w), wtot, total);
    const uint32_t words[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (uint32_t k = 0; k < kPerLane; ++k) {
        prefix[tid * kPerLane + k] = (uint16_t)run;
        run += (words[k >> 2] >> (8 * (k & 3) + kKeptShift)) & 1u;
    }
    if (tid == kThreads - 1) prefix[kReadCallTile] = (uint16_t)run;  // (= total; pairs behind n_pairs count as not kept)
    __syncthreads();

    const uint64_t base = a.tile_base[blockIdx.x];
    // the records: position by position, so that a wave reads 64 neighbouring pairs and writes its kept ones side by side.  A kept
    // pair at p has at most p kept pairs in front of it: the record's index is below n_pairs whatever the flags are.
    // The three passes are unrolled over the lane's 16 positions, every load of a pass in flight before the next pass waits for
    // any of them: a workgroup pays three round trips to memory, not sixteen times three (a batch of 10 000 shallow loci is 74 tiles,
    // far fewer workgroups than the device has compute units, and nothing else would hide the latency).
    int64_t call[kPerLane];
    uint32_t read[kPerLane], tail[kPerLane];  // tail: group | flags << 8 (reserved = 0)
#pragma unroll
    for (uint32_t k = 0; k < kPerLane; ++k) {
        const uint32_t pos = k * kThreads + tid;
        const bool keep = sbits[pos] & INQ_PAIR_KEPT;  // (zero behind tile_end)
        call[k] = keep ? a.pair_call[tile_start + pos] : 0;
        read[k] = keep ? a.pair_read[tile_start + pos] : 0u;
    }
#pragma unroll
    for (uint32_t k = 0; k < kPerLane; ++k) {
        const uint32_t bits = sbits[k * kThreads + tid];
        const uint32_t group = !UNPHASED && (bits & INQ_PAIR_KEPT) ? phase_group(a, read[k]) : 0u;  // phased: the read's HP
        tail[k] = group | ((bits & INQ_PAIR_CLIP) ? INQ_READ_CALL_CLIP : 0u) << 8;
    }
#pragma unroll
    for (uint32_t k = 0; k < kPerLane; ++k) {
        const uint32_t pos = k * kThreads + tid;
        if (!(sbits[pos] & INQ_PAIR_KEPT)) continue;
        // call | read | group, flags, reserved: the 16 bytes of inq_read_call_t in one store
        *(uint4 *)(a.kept + (base + prefix[pos])) =
            make_uint4((uint32_t)(uint64_t)call[k], (uint32_t)((uint64_t)call[k] >> 32), read[k], tail[k]);
        if (a.kept_pair) a.kept_pair[base + prefix[pos]] = tile_start + pos;  // (a call with sequences only)
    }

    // kept_off of the loci that begin in this tile: from the first j with locus_pair_off[j] >= tile_start on, until one begins at or
    // behind tile_end.  Runs of empty loci share an offset and are all written.  The last tile takes the loci that begin at n_pairs as
    // well (prefix[n_pairs - tile_start] is the tile's total, full tile or not), kept_off[n_loci] among them.  Every j is checked on its
    // own, so offsets that do not ascend (the call then ends in an error) write nothing out of place.
    const uint64_t first = block_lower_bound(a.locus_pair_off, a.n_loci + 1, tile_start, wtot);
    for (uint64_t j = first + tid; j <= a.n_loci; j += kThreads) {
        const uint64_t o = a.locus_pair_off[j];
        if (o > tile_end || (o == tile_end && !last_tile)) break;
        if (o >= tile_start) a.kept_off[j] = base + prefix[o - tile_start];
    }
}

}  // namespace

void launch_read_calls(const ReadCallArgs &a, bool unphased, hipStream_t s) {
    const uint64_t n_tiles = read_call_tiles(a.n_pairs);
    if (n_tiles == 0) return;
    hipLaunchKernelGGL(read_call_count, dim3((uint32_t)n_tiles), dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(read_call_scan, dim3(1), dim3(kThreads), 0, s, a, n_tiles);
    if (unphased)
        hipLaunchKernelGGL(read_call_scatter<true>, dim3((uint32_t)n_tiles), dim3(kThreads), 0, s, a);
    else
        hipLaunchKernelGGL(read_call_scatter<false>, dim3((uint32_t)n_tiles), dim3(kThreads), 0, s, a);
}

}  // namespace inq
