// locus_motifs.h — which short motif a locus's kept reads repeat (inq_locus_motif_t): locus_motif_kernel of locus_motifs.hip
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/inquistr_hip.h"

namespace inq {

constexpr uint32_t kLocusMotifMaxPeriod = 6;  // the periods tried, 1 .. 6: 4^6 classes of the histogram

// locus_motif_kernel: one inq_locus_motif_t per locus j < n_loci (the contract: include/inquistr_hip.h, inq_locus_motif_t) out of the
// records kept_off[j] .. kept_off[j + 1], cut to min(*n_kept, n_recs).  Record k's bases are segment kept_pair[k] (null: segment k) of
// `bytes`, as ReadMotifArgs has them.  use[j] (where use is not null) is what read_motif_kernel measures locus j with: given[j] where
// given is not null and given[j] names a motif, else found[j].word
struct LocusMotifArgs {
    const uint64_t *kept_pair;  // [n_recs] or null
    const uint64_t *n_kept;     // DEVICE: kept_off[n_loci]; null: n_recs
    const uint64_t *kept_off;   // [n_loci + 1]
    uint64_t n_loci;
    const uint8_t *bytes;
    uint64_t n_bytes;
    const uint64_t *seg_off;  // [n_segs]
    const uint32_t *seg_len;  // [n_segs]
    uint64_t n_segs;
    uint64_t n_recs;
    const uint64_t *given;     // [n_loci] or null
    inq_locus_motif_t *found;  // [n_loci]
    uint64_t *use;             // [n_loci] or null
};
void launch_locus_motifs(const LocusMotifArgs &a, hipStream_t s);  // n_loci == 0 launches nothing

}  // namespace inq
