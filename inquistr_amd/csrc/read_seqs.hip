// read_seqs.hip — the bases behind each Call (inq_read_seq_t): which part of a read's SEQ lies over a locus window, and its gather.
//
// The device front end inflates every SEQ byte of the BAM; a span slot's inflated bytes are reused by a later span, so the slice of
// every (locus, read) pair is cut while they are there:
//   span time   seq_window_kernel  walks the pair's CIGAR as far as the window and writes (q_beg, n_bases)
//               seq_slice_kernel   packs bases [q_beg, q_beg + n_bases) of the record's SEQ, two to a byte, first base in the high nibble
//   flush time  read_seq_record_kernel: one inq_read_seq_t per kept record; the kept pairs' packed bytes are then a plain byte gather
//               (name_copy_kernel of read_names.hip through its u64 index)
//
// The window walk.  Q(x) of the contract is a sum over the ops, each term a function of the op and of the reference position in front
// of it alone.  So one 16-lane row walks one pair in pieces of 64 ops (one dwordx4 per lane, as the row walk of cigar_walk.h): the
// positions are an in-lane prefix plus a DPP row scan plus a carry, the two sums stay in the lanes' registers and are reduced once,
// when the pair is done.  A pair stops after the piece that takes the position to end_ext - 1 or past it: no later op contributes
// to either sum (an M there starts at or past x, an I or S has r_op >= x).  Positions and sums are 64-bit: a piece alone can span 2^34.
// Loads go through one buffer descriptor over the batch's CIGAR; a lane past the read's padded length gets an offset past the range
// and loads `0M`, which adds nothing.  (A batch of 4 GiB of CIGAR or more does not fit a descriptor and is read with plain loads.)
// No atomics, no LDS allocation, no workgroup waits for another: every output is a plain function of the inputs.
//
// Bounds: a pair whose read index, descriptor or locus lies outside the batch gets (0, 0) and loads nothing through it; the slice
// kernel cuts every segment to the destination, to the record's own l_seq and to the inflated bytes before a byte moves.
#include <hip/hip_runtime.h>

#include "cigar_walk.h"
#include "kept_view.h"
#include "read_seqs.h"
#include "segment_store.h"

namespace inq {
namespace {

constexpr uint32_t kThreads = 256;
static_assert(kSeqWindowTile * kSeqRowLanes == kThreads && kSeqSliceTile * kSeqSliceLanes == kThreads, "a workgroup's lanes are dealt among its rows");
static_assert(kSeqRowLanes == (uint32_t)kRowLanes, "a row is one DPP row");
static_assert(sizeof(inq_read_seq_t) == 8, "a record is one 8-byte store");

// ops that consume query AND reference (M = X: bits 0, 7, 8) and query only (I S: bits 1, 4)
constexpr uint32_t kMatchOps = 0x181u, kInsertOps = 0x012u;

__device__ __forceinline__ uint32_t load_le32(const uint8_t *p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

// l_seq of read ri, 0xffffffff where nothing cuts
__device__ __forceinline__ uint32_t seq_len_of(const SeqLenSource &L, uint32_t ri) {
    if (L.l_seq) return L.l_seq[ri];
    if (!L.u) return 0xffffffffu;
    if (ri < L.read_base || ri - L.read_base >= L.n_records) return 0u;
    const uint64_t x = L.rec_off[ri - L.read_base];
    if (x >= L.u_bytes || L.u_bytes - x < 24u) return 0u;
    return load_le32(L.u + x + 20u);
}

__device__ __forceinline__ uint32_t capped_u32(uint64_t q, uint32_t cap) { return q < (uint64_t)cap ? (uint32_t)q : cap; }

__global__ __launch_bounds__(256) void seq_window_kernel(SeqWindowArgs a) {
    const int lane = lane_id();
    const uint32_t rl = (uint32_t)lane & (kSeqRowLanes - 1u);
    const int row_shift = lane & ~(int)(kSeqRowLanes - 1u);  // where this row's bits lie in a ballot
    const bool small = a.n_cigar4 < (1ull << 28);
    const __amdgpu_buffer_rsrc_t rsrc =
        __builtin_amdgcn_make_buffer_rsrc((void *)a.cigar4, (short)0, small ? (int)(uint32_t)(a.n_cigar4 * 16u) : 0, 0x00020000);
    // (the grid is capped, launch_seq_window: a workgroup takes every gridDim.x-th tile)
    for (uint64_t base = (uint64_t)blockIdx.x * kSeqWindowTile; base < a.n_pairs; base += (uint64_t)gridDim.x * kSeqWindowTile) {
        const uint64_t p = base + threadIdx.x / kSeqRowLanes;
        const bool has = p < a.n_pairs;

        // the pair's locus: the j with off[j] <= p < off[j + 1]; what the search found is checked here
        const uint64_t lo = row_find_interval(a.locus_pair_off, a.n_loci, p, has, rl, row_shift);
        bool live = has && lo < a.n_loci && a.locus_pair_off[lo] <= p && p < a.locus_pair_off[lo + 1];
        int64_t x1 = 0, x2 = 0;  // start_ext and end_ext - 1
        if (live) {
            const Window W = make_window(a.locus_start[lo], a.locus_end[lo], 0u);
            x1 = (int64_t)W.se, x2 = (int64_t)W.ee - 1;
            live = x2 > x1;  // width 0, and start = 9, where start_ext wraps to 2^32 - 1 and the width does not come out 0
        }
        uint32_t cur = 0, left = 0, lseq = 0;
        int64_t carry = 0;
        if (live) {
            const uint32_t ri = a.pair_read[p];
            live = (uint64_t)ri < a.n_reads;
            if (live) {
                const uint4 r = a.reads[ri];
                cur = r.x, left = cigar_groups(r.y & 0x0fffffffu), carry = (int64_t)(int32_t)r.z;
                // a descriptor outside the batch is no read of it; an empty CIGAR or a start at or past end_ext - 1 settles the pair
                if (r.y >= 0x10000000u || (uint64_t)cur + left > a.n_cigar4)
                    live = false;
                else
                    lseq = seq_len_of(a.len, ri);
            }
        }
        const bool counted = live;
        live = live && left != 0u && carry < x2;

        uint64_t acc1 = 0, acc2 = 0;  // this lane's share of Q(x1) and Q(x2)
        while (ballot64(live)) {
            const bool on = live && rl < left;
            u32x4 w = {0u, 0u, 0u, 0u};
            if (small)
                w = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(on ? (cur + rl) * 16u : 0xfffffff0u), 0, 0);
            else if (on)
                w = *reinterpret_cast<const u32x4 *>(a.cigar4 + ((uint64_t)cur + rl));
            const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
            uint32_t tot = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) tot += ref_advance(ws[k] & 15u, ws[k] >> 4);
            const uint64_t incl = row_inclusive_scan_u64(tot);
            const uint64_t rtot = row_last_u64(incl);
            int64_t r = carry + (int64_t)(incl - tot);  // the reference position in front of this lane's first op
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t op = ws[k] & 15u;
                const int64_t len = (int64_t)(ws[k] >> 4), d1 = x1 - r, d2 = x2 - r;
                if ((kMatchOps >> op) & 1u) {
                    acc1 += (uint64_t)(d1 < 0 ? 0 : d1 < len ? d1 : len);
                    acc2 += (uint64_t)(d2 < 0 ? 0 : d2 < len ? d2 : len);
                } else if ((kInsertOps >> op) & 1u) {
                    acc1 += (uint64_t)(d1 > 0 ? len : 0);
                    acc2 += (uint64_t)(d2 > 0 ? len : 0);
                }
                r += (int64_t)ref_advance(op, ws[k] >> 4);
            }
            if (live) {
                carry += (int64_t)rtot;
                cur += kSeqRowLanes;
                left = left > kSeqRowLanes ? left - kSeqRowLanes : 0u;
                live = left != 0u && carry < x2;
            }
        }
        const uint64_t q1 = row_last_u64(row_inclusive_scan_u64(acc1)), q2 = row_last_u64(row_inclusive_scan_u64(acc2));
        if (has && rl == 0u) {
            const uint32_t b = counted ? capped_u32(q1, lseq) : 0u, e = counted ? capped_u32(q2, lseq) : 0u;
            a.q_beg[p] = b;
            a.n_bases[p] = e >= b ? e - b : 0u;
        }
    }
}

// where a record's SEQ lies and how many bases of it the inflated bytes hold
struct SeqSource {
    const uint8_t *seq;
    uint64_t n_bases;
};
__device__ __forceinline__ SeqSource locate_seq(const SeqSliceArgs &a, uint32_t ri) {
    SeqSource s{nullptr, 0u};
    if (ri < a.read_base || ri - a.read_base >= a.n_records) return s;
    const uint64_t x = a.rec_off[ri - a.read_base];
    if (x >= a.u_bytes || a.u_bytes - x < 36u) return s;  // (36: block_size + the fixed fields in front of the name)
    const uint8_t *rec = a.u + x;
    // the STORED op count places SEQ, whatever CIGAR the batch holds for the read
    const uint64_t s0 = x + 36u + rec[12] + 4u * ((uint64_t)rec[16] | (uint64_t)rec[17] << 8);
    if (s0 >= a.u_bytes) return s;
    const uint64_t l_seq = load_le32(rec + 20), room = (a.u_bytes - s0) * 2u;
    s.seq = a.u + s0;
    s.n_bases = l_seq < room ? l_seq : room;
    return s;
}

__global__ __launch_bounds__(256) void seq_slice_kernel(SeqSliceArgs a) {
    const uint32_t sub = threadIdx.x % kSeqSliceLanes;
    for (uint64_t p = (uint64_t)blockIdx.x * kSeqSliceTile + threadIdx.x / kSeqSliceLanes; p < a.n_pairs; p += (uint64_t)gridDim.x * kSeqSliceTile) {
        const uint64_t d0 = a.dst_off[p];
        uint64_t d1 = a.dst_off[p + 1];
        if (d1 > a.dst_bytes) d1 = a.dst_bytes;
        if (d0 >= d1) continue;  // an empty slice (or offsets that do not ascend): nothing moves
        const uint64_t q = a.q_beg[p], n = a.n_bases[p];
        uint64_t len = d1 - d0;
        if (len > (n + 1u) / 2u) len = (n + 1u) / 2u;
        const SeqSource src = locate_seq(a, a.pair_read[p]);
        // destination byte d: base q + 2d in the high nibble, base q + 2d + 1 in the low one; a base at or behind the slice's end or
        // the record's is 0
        const uint64_t end = q + n < src.n_bases ? q + n : src.n_bases;
        auto base_at = [&](uint64_t k) -> uint32_t { return k < end ? (src.seq[k >> 1] >> ((~k & 1u) * 4u)) & 15u : 0u; };
        auto byte_at = [&](uint64_t d) -> uint8_t { return (uint8_t)(base_at(q + 2u * d) << 4 | base_at(q + 2u * d + 1u)); };
        // (a soft clip in the window is tens of kilobases: the lanes stride over the words)
        store_segment<kSeqSliceLanes>(a.dst + d0, len, sub, byte_at, [&](uint64_t d) -> uint32_t {
            const uint64_t k = q + 2u * d;
            if (k + 9u > end)
                return (uint32_t)byte_at(d) | (uint32_t)byte_at(d + 1u) << 8 | (uint32_t)byte_at(d + 2u) << 16 | (uint32_t)byte_at(d + 3u) << 24;
            // all eight bases and the one behind them are the record's: five source bytes at most
            const uint8_t *s = src.seq + (k >> 1);
            if (!(k & 1u)) return load_le32(s);
            const uint64_t x = (uint64_t)load_le32(s) | (uint64_t)s[4] << 32;
            return ((uint32_t)x & 0x0f0f0f0fu) << 4 | ((uint32_t)(x >> 12) & 0x0f0f0f0fu);
        });
    }
}

__global__ __launch_bounds__(256) void read_seq_record_kernel(ReadSeqArgs a) {
    const uint64_t total = kept_total(a.n_kept, a.n_pairs);
    for (uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x; k < total; k += (uint64_t)gridDim.x * kThreads) {
        const uint64_t p = a.kept_pair[k];
        uint2 rec = make_uint2(0u, 0u);
        if (p < a.n_pairs) rec = make_uint2(a.q_beg[p], a.n_bases[p]);
        *reinterpret_cast<uint2 *>(a.recs + k) = rec;
    }
}

}  // namespace

void launch_seq_window(const SeqWindowArgs &a, uint32_t grid_side, hipStream_t s) {
    if (!a.n_pairs) return;
    hipLaunchKernelGGL(seq_window_kernel, dim3(side_grid((a.n_pairs + kSeqWindowTile - 1) / kSeqWindowTile, grid_side)), dim3(kThreads), 0, s, a);
}

void launch_seq_slice(const SeqSliceArgs &a, uint32_t grid_side, hipStream_t s) {
    if (!a.n_pairs) return;
    hipLaunchKernelGGL(seq_slice_kernel, dim3(side_grid((a.n_pairs + kSeqSliceTile - 1) / kSeqSliceTile, grid_side)), dim3(kThreads), 0, s, a);
}

void launch_read_seq_records(const ReadSeqArgs &a, uint32_t grid_side, hipStream_t s) {
    if (!a.n_pairs) return;
    hipLaunchKernelGGL(read_seq_record_kernel, dim3(side_grid((a.n_pairs + kThreads - 1) / kThreads, grid_side)), dim3(kThreads), 0, s, a);
}

}  // namespace inq
