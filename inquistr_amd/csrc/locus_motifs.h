// locus_motifs.h — which short motif a locus's kept reads repeat (inq_locus_motif_t): locus_motif_kernel of locus_motifs.hip
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/inquistr_hip.h"
#include "kept_view.h"

namespace inq {

constexpr uint32_t kLocusMotifMaxPeriod = 6;  // the periods tried, 1 .. 6: 4^6 classes of the histogram

// locus_motif_kernel: one inq_locus_motif_t per locus j < n_loci (the contract: include/inquistr_hip.h, inq_locus_motif_t) out of the
// records kept_off[j] .. kept_off[j + 1], cut to min(*n_kept, n_recs).  The records and their bases are KeptSlices' (kept_view.h), as
// ReadMotifArgs has them.  use[j] (where use is not null) is what read_motif_kernel measures locus j with: given[j] where given is not
// null and given[j] names a motif, else found[j].word
struct LocusMotifArgs : KeptSlices {
    const uint64_t *given;    // [n_loci] or null
    inq_locus_motif_t *found;  // [n_loci]
    uint64_t *use;             // [n_loci] or null
};
void launch_locus_motifs(const LocusMotifArgs &a, uint32_t grid_side, hipStream_t s);  // n_loci == 0 launches nothing

}  // namespace inq
