// read_motifs.h — the motif runs of the bases behind each Call (inq_read_motif_t): read_motif_kernel of read_motifs.hip
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/inquistr_hip.h"

namespace inq {

constexpr uint32_t kMotifRowLanes = 16;                     // lanes of one row = one kept record; lane r owns rotation r
constexpr uint32_t kReadMotifTile = 256 / kMotifRowLanes;   // records per workgroup and turn (inq_read_motif_tile)

// read_motif_kernel: one inq_read_motif_t per record k < min(*n_kept, n_recs) (the contract: include/inquistr_hip.h, inq_read_motif_t).
// Record k's bases are segment kept_pair[k] (null: segment k) of `bytes`: seg_len[p] bases packed from byte seg_off[p] on; its locus is
// the j with kept_off[j] <= k < kept_off[j + 1], its motif word motif[j]
struct ReadMotifArgs {
    const uint64_t *kept_pair;  // [n_recs] or null
    const uint64_t *n_kept;     // DEVICE: kept_off[n_loci]; null: n_recs
    const uint64_t *kept_off;   // [n_loci + 1]
    const uint64_t *motif;      // [n_loci]
    uint64_t n_loci;
    const uint8_t *bytes;
    uint64_t n_bytes;
    const uint64_t *seg_off;  // [n_segs]
    const uint32_t *seg_len;  // [n_segs]
    uint64_t n_segs;
    inq_read_motif_t *recs;  // [n_recs], 16-byte aligned
    uint64_t n_recs;
};
void launch_read_motifs(const ReadMotifArgs &a, hipStream_t s);  // n_recs == 0 or no motif array launches nothing

}  // namespace inq
