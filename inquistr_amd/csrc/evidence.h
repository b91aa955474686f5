// evidence.h — the counting kernels behind inq_locus_evidence_t (evidence.hip), launched by capi.hip behind the locus kernels
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/inquistr_hip.h"

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

struct EvidenceArgs {
    const uint64_t *locus_pair_off;  // [n_loci + 1]
    const uint8_t *pair_bits;        // [n_pairs] INQ_PAIR_*, as the locus kernels left them
    const int64_t *pair_call;        // [n_pairs]
    const uint32_t *pair_read;       // [n_pairs]  (phased only)
    const uint32_t *read_words;      // inq_read_t as four words: word 3 = mapq | bits << 8 | phase << 16 | promise << 24  (phased only)
    uint64_t n_reads, n_pairs, n_loci;
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
