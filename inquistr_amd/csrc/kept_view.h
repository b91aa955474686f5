// kept_view.h — what the kernels behind the compaction (read_names.hip, read_seqs.hip, read_motifs.hip, locus_motifs.hip) read of a flush
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wave_primitives.h"

namespace inq {

// The kept records of a flush, locus by locus, and the packed bases behind each: record k belongs to the locus j with
// kept_off[j] <= k < kept_off[j + 1]; its bases are segment kept_pair[k] (null: segment k) of `bytes`, seg_len[p] bases packed from byte
// seg_off[p] on.  capi.hip fills one per flush, side_outputs.hip one per stand-alone call; both motif argument structs begin with it
struct KeptSlices {
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
};

// the records the compaction wrote: *n_kept (null: all of them), never more than the arrays hold
__device__ __forceinline__ uint64_t kept_total(const uint64_t *n_kept, uint64_t cap) {
    const uint64_t total = n_kept ? *n_kept : cap;
    return total < cap ? total : cap;
}

// a record's slice: n bases packed from seg on; n = 0: nothing to read
struct Slice {
    const uint8_t *seg;
    uint64_t n;
};
// A record whose segment index, offset or length lies outside what the launch holds has no slice, and nothing is read through it
__device__ __forceinline__ Slice slice_of(const KeptSlices &v, uint64_t rec, bool has) {
    Slice S{v.bytes, 0};
    if (!has) return S;
    const uint64_t p = v.kept_pair ? v.kept_pair[rec] : rec;
    if (p >= v.n_segs) return S;
    const uint64_t o = v.seg_off[p], n = v.seg_len[p], nb = (n + 1u) / 2u;
    if (o > v.n_bytes || nb > v.n_bytes - o) return S;
    S.seg += o, S.n = n;
    return S;
}

// The j with off[j] <= x < off[j + 1] among off[0 .. n], found by a 16-lane row (this lane is rl of it, its bits lie at row_shift of a
// ballot), sixteen probes a step: 1, 2, 3, 4 steps for n <= 16, <= 256, <= 4 096 and above.  Every row of the wave takes part, one
// without a question with has = false.  The answer lies in [lo, hi); offsets that do not ascend end the search all the same, so the
// caller checks that what comes back (possibly n) is the interval
__device__ __forceinline__ uint64_t row_find_interval(const uint64_t *off, uint64_t n, uint64_t x, bool has, uint32_t rl, int row_shift) {
    uint64_t lo = 0, hi = has ? n : 0;
    while (ballot64(hi - lo > 1u)) {
        const uint64_t size = hi - lo, step = (size + (uint32_t)kRowLanes - 1u) / (uint32_t)kRowLanes, idx = lo + rl * step;
        const bool below = size > 1u && idx < hi && off[idx + 1] <= x;
        const uint32_t c = (uint32_t)__popc((uint32_t)(ballot64(below) >> row_shift) & 0xffffu);
        if (size > 1u) {
            if (c == 0u) {
                hi = lo + 1u;
            } else {
                const uint64_t last = lo + (uint64_t)(c - 1u) * step;  // the last probe at or below x; it lies in front of hi
                lo = last + 1u;
                hi = last + step + 1u < hi ? last + step + 1u : hi;
            }
        }
    }
    return lo;
}

}  // namespace inq
