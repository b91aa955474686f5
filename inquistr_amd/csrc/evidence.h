// evidence.h — the counting kernels behind inq_locus_evidence_t (evidence.hip), launched by capi.hip behind the locus kernels
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/inquistr_hip.h"
#include "pair_view.h"

namespace inq {

constexpr uint32_t kEvidenceWaveMax = 256;  // a locus of up to this many pairs is counted by one wave of the first launch
constexpr uint32_t kEvidenceSlice = 16384;  // a deeper one in slices of this many pairs, one workgroup of the second launch each

// one slice of a deep locus: pairs [off[locus] + slice * kEvidenceSlice, ... + kEvidenceSlice) cut at the locus's end
struct EvidenceSlice {
    uint32_t locus, slice;
};

// Context scratch of the evidence path: the header (the memset in front of the launches zeroes exactly these 16 bytes), then the list
struct EvidenceWork {
    unsigned long long n_slices;  // slices listed by the first launch (may exceed list_cap: the surplus was not stored)
    unsigned long long pad;
};

struct EvidenceArgs : PairView {  // (pair_read is read for a phased batch only)
    inq_locus_evidence_t *evidence;  // [n_loci]
    EvidenceWork *work;
    EvidenceSlice *list;             // [list_cap]
    uint64_t list_cap;               // 0: the depth hint rules deep loci out, none is listed
};

// slices the deep loci of a batch of n_pairs pairs can make: every deep locus has more than kEvidenceWaveMax pairs and at most one
// slice that is not full
inline uint64_t evidence_list_cap(uint64_t n_pairs) { return n_pairs / (kEvidenceWaveMax + 1) + n_pairs / kEvidenceSlice + 1; }
inline size_t evidence_scratch_bytes(uint64_t list_cap) { return sizeof(EvidenceWork) + (size_t)list_cap * sizeof(EvidenceSlice); }

// the launches (one, or two when a.list_cap > 0) on s; a.work's header must have been zeroed on s in front
void launch_evidence(const EvidenceArgs &a, bool unphased, uint32_t grid_deep, hipStream_t s);

}  // namespace inq
