// read_seqs.h — the bases behind each Call (inq_read_seq_t): the window walk and the packed gather of read_seqs.hip
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/inquistr_hip.h"

namespace inq {

constexpr uint32_t kSeqRowLanes = 16;                      // lanes of one row = one (locus, read) pair of the window walk
constexpr uint32_t kSeqWindowTile = 256 / kSeqRowLanes;    // pairs per workgroup and turn (inq_seq_window_tile)
constexpr uint32_t kSeqSliceLanes = 8;                     // lanes that share one segment of the packed gather
constexpr uint32_t kSeqSliceTile = 256 / kSeqSliceLanes;   // segments per workgroup

// Where a read's SEQ length comes from: an array over the batch's reads, or the records of a span in its inflated bytes (read r is
// record r - read_base, its l_seq the four bytes at rec_off + 20).  Both null: no cut.
struct SeqLenSource {
    const uint32_t *l_seq = nullptr;  // [n_reads]
    const uint8_t *u = nullptr;
    uint64_t u_bytes = 0;
    const uint64_t *rec_off = nullptr;  // [n_records]
    uint64_t n_records = 0, read_base = 0;
};

// seq_window_kernel: q_beg[p], n_bases[p] of pair p < n_pairs (the contract: include/inquistr_hip.h, inq_read_seq_t)
struct SeqWindowArgs {
    const uint4 *cigar4;  // packed ops as 16-byte groups
    uint64_t n_cigar4;
    const uint4 *reads;   // inq_read_t as uint4
    uint64_t n_reads;
    const uint32_t *pair_read;       // [n_pairs]
    const uint64_t *locus_pair_off;  // [n_loci + 1]; pair p belongs to the locus j with off[j] <= p < off[j + 1]
    const uint32_t *locus_start, *locus_end;
    uint64_t n_loci, n_pairs;
    SeqLenSource len;
    uint32_t *q_beg, *n_bases;  // [n_pairs]
};
void launch_seq_window(const SeqWindowArgs &a, uint32_t grid_side, hipStream_t s);  // n_pairs == 0 launches nothing

// seq_slice_kernel: segment p writes (n_bases[p] + 1) / 2 bytes at dst + dst_off[p], the bases [q_beg[p], q_beg[p] + n_bases[p]) of
// record pair_read[p] - read_base, first base in the high nibble of the first byte
struct SeqSliceArgs {
    const uint8_t *u;
    uint64_t u_bytes;
    const uint64_t *rec_off;  // [n_records]
    uint64_t n_records, read_base;
    const uint32_t *pair_read, *q_beg, *n_bases;  // [n_pairs]
    uint8_t *dst;
    uint64_t dst_bytes;
    const uint64_t *dst_off;  // [n_pairs + 1]
    uint64_t n_pairs;
};
void launch_seq_slice(const SeqSliceArgs &a, uint32_t grid_side, hipStream_t s);

// one inq_read_seq_t per record the compaction wrote, k < min(*n_kept, n_pairs): that of pair kept_pair[k]
struct ReadSeqArgs {
    const uint64_t *kept_pair;  // [n_pairs]
    const uint64_t *n_kept;     // DEVICE: kept_off[n_loci]
    const uint32_t *q_beg, *n_bases;
    inq_read_seq_t *recs;  // [n_pairs], 8-byte aligned
    uint64_t n_pairs;
};
void launch_read_seq_records(const ReadSeqArgs &a, uint32_t grid_side, hipStream_t s);

}  // namespace inq
