// read_motifs.h — the motif runs of the bases behind each Call (inq_read_motif_t): read_motif_kernel of read_motifs.hip
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/inquistr_hip.h"
#include "kept_view.h"

namespace inq {

constexpr uint32_t kMotifRowLanes = 16;                     // lanes of one row = one kept record; lane r owns rotation r
constexpr uint32_t kReadMotifTile = 256 / kMotifRowLanes;   // records per workgroup and turn (inq_read_motif_tile)

// read_motif_kernel: one inq_read_motif_t per record k < min(*n_kept, n_recs) (the contract: include/inquistr_hip.h, inq_read_motif_t).
// Record k's bases and its locus j are KeptSlices' (kept_view.h), its motif word motif[j]
struct ReadMotifArgs : KeptSlices {
    const uint64_t *motif;   // [n_loci]
    inq_read_motif_t *recs;  // [n_recs], 16-byte aligned
};
void launch_read_motifs(const ReadMotifArgs &a, uint32_t grid_side, hipStream_t s);  // n_recs == 0 or no motif array launches nothing

}  // namespace inq
