// evidence.hip — per-locus read evidence (inq_locus_evidence_t): a segmented reduction over the per-pair outputs of the locus kernels.
//
// What is counted is what the reference's two per-locus functions see on their way to median_str_length:
//   n_fetched            records fetch() yields                          src/call.rs:288,338      -> INQ_PAIR_FETCHED
//   n_kept               records that pass the read filter               src/call.rs:297-302 / 349-355 -> INQ_PAIR_KEPT
//   n_group1 / n_group2  Calls handed to median_str_length for phase1 / phase2: phased = kept reads with HP 1 / HP 2 (:358), unphased =
//                        the two halves of the sorted kept reads, len / 2 and the rest (:312-314)
//   n_clip               of those, Call::Clip                            src/call.rs:67-71,405    -> INQ_PAIR_CLIP
//   call_min / call_max  the extremes of their values
// None of it needs the sort or the tie rule of the reduces, so it runs BEHIND the locus kernels and reads only what they wrote:
// 1 B of bits and 8 B of Call per pair, and for a phased batch 4 B of pair_read and one word of the read's descriptor for every kept pair.
//
// Two launches.  evidence_shallow: one wave per locus, the lanes stride over the pairs (64 B of bits, 512 B of calls per step), sums and
// extremes are reduced across the wave in registers (DPP, readlane; no LDS), lane 0 stores the record.  A locus of more than
// kEvidenceWaveMax pairs is cut into slices of kEvidenceSlice pairs instead, which the wave appends to a list in context scratch, and
// its record is set to the neutral element of the merge.  evidence_deep (fixed grid; skipped when the depth hint rules deep loci out):
// one workgroup per listed slice, partials merged into the record with device-scope integer atomics (add, min, max: any order gives
// the same bits); the workgroup that arrives last at a locus writes what needs the totals.  No workgroup waits for another.
#include <hip/hip_runtime.h>

#include "evidence.h"
#include "wave_primitives.h"

namespace inq {
namespace {

constexpr int64_t kI64Max = 0x7fffffffffffffffll, kI64Min = -kI64Max - 1;

// the counts of up to kEvidenceSlice pairs, two to a word (16 384 fits 16 bits), and the extremes of the grouped Calls
struct Partial {
    uint32_t fetched_kept;  // fetched | kept << 16
    uint32_t group12;       // HP 1 | HP 2 << 16  (phased only)
    uint32_t clip;
    int64_t mn, mx;
};
__device__ __forceinline__ Partial no_pairs() { return Partial{0u, 0u, 0u, kI64Max, kI64Min}; }

template <bool UNPHASED>
__device__ __forceinline__ void count_pair(const EvidenceArgs &a, uint64_t i, Partial &p) {
    const uint32_t bits = a.pair_bits[i];
    p.fetched_kept += (bits & INQ_PAIR_FETCHED) ? 1u : 0u;
    if (!(bits & INQ_PAIR_KEPT)) return;
    p.fetched_kept += 1u << 16;
    if (!UNPHASED) {
        // a kept read of a phased batch has an HP tag (:349); HP 0 is kept and belongs to no group
        const uint32_t phase = phase_group(a, a.pair_read[i]);
        if (phase != 1u && phase != 2u) return;
        p.group12 += phase == 1u ? 1u : 1u << 16;
    }
    p.clip += (bits & INQ_PAIR_CLIP) ? 1u : 0u;
    const int64_t v = a.pair_call[i];
    p.mn = v < p.mn ? v : p.mn;
    p.mx = v > p.mx ? v : p.mx;
}

// x moved along the DPP pattern CTRL; a lane the move does not reach (row start, rows outside ROW_MASK) keeps its own x, which min
// and max absorb
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int64_t dpp_move_i64(int64_t x) {
    const int lo = (int)(uint32_t)x, hi = (int)(uint32_t)((uint64_t)x >> 32);
    const uint32_t mlo = (uint32_t)__builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xf, false);
    const uint32_t mhi = (uint32_t)__builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xf, false);
    return (int64_t)(((uint64_t)mhi << 32) | mlo);
}
// min (or max) over the 64 lanes, the same steps as wave_inclusive_scan_u32; every lane receives lane 63's result
template <bool MAX>
__device__ __forceinline__ int64_t wave_extreme_i64(int64_t x) {
    auto pick = [](int64_t a, int64_t b) { return MAX ? (a > b ? a : b) : (a < b ? a : b); };
    x = pick(x, dpp_move_i64<DPP_ROW_SHR1, 0xf>(x));
    x = pick(x, dpp_move_i64<DPP_ROW_SHR2, 0xf>(x));
    x = pick(x, dpp_move_i64<DPP_ROW_SHR4, 0xf>(x));
    x = pick(x, dpp_move_i64<DPP_ROW_SHR8, 0xf>(x));
    x = pick(x, dpp_move_i64<DPP_ROW_BCAST15, 0xa>(x));
    x = pick(x, dpp_move_i64<DPP_ROW_BCAST31, 0xc>(x));
    return readlane_i64(x, kWave - 1);
}

// every lane of the wave receives the wave's totals (all 64 lanes must be active)
__device__ __forceinline__ Partial wave_reduce(const Partial &p) {
    Partial t;
    t.fetched_kept = wave_sum_u32(p.fetched_kept);
    t.group12 = wave_sum_u32(p.group12);
    t.clip = wave_sum_u32(p.clip);
    t.mn = wave_extreme_i64<false>(p.mn);
    t.mx = wave_extreme_i64<true>(p.mx);
    return t;
}

// The fields that need a locus's totals.  Unphased: the sorted kept reads are split at len / 2 (:314), so the group sizes follow from
// n_kept alone.  No Call in either group: min = max = 0.
template <bool UNPHASED>
__device__ __forceinline__ void store_totals(inq_locus_evidence_t *rec, uint32_t kept, uint32_t g1, uint32_t g2, int64_t mn, int64_t mx) {
    if (UNPHASED) g1 = kept / 2u, g2 = kept - kept / 2u;
    const bool none = g1 + g2 == 0u;
    rec->n_group1 = g1;
    rec->n_group2 = g2;
    rec->reserved = 0u;
    rec->call_min = none ? 0 : mn;
    rec->call_max = none ? 0 : mx;
}

template <bool UNPHASED>
__global__ __launch_bounds__(256) void evidence_shallow(EvidenceArgs a) {
    const uint64_t j = (uint64_t)blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (j >= a.n_loci) return;  // (the whole wave)
    const int lane = lane_id();
    const uint64_t b = a.locus_pair_off[j];
    uint64_t e = a.locus_pair_off[j + 1];
    if (e < b || e > a.n_pairs) e = b;  // offsets the batch's own checks reject: the call ends in an error, nothing is read through them
    const uint64_t n = e - b;
    inq_locus_evidence_t *rec = a.evidence + j;
    if (n > kEvidenceWaveMax) {
        // the second launch's: one list entry per slice, and the record set to what add / min / max start from.  reserved counts the
        // slices that have been merged; the last one puts it back to 0.
        const uint64_t n_slices = (n + kEvidenceSlice - 1) / kEvidenceSlice;
        unsigned long long base = 0;
        if (lane == 0) base = __hip_atomic_fetch_add(&a.work->n_slices, (unsigned long long)n_slices, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        base = (unsigned long long)readlane_i64((int64_t)base, 0);
        // (every slice fits for offsets that ascend and a depth hint that was kept; a batch that breaks either ends in an error, and
        // the slices that do not fit are dropped: the list is never written or read past its end)
        for (uint64_t k = (uint64_t)lane; k < n_slices; k += kWave)
            if (base + k < a.list_cap) a.list[base + k] = EvidenceSlice{(uint32_t)j, (uint32_t)k};
        if (lane == 0) {
            rec->n_fetched = rec->n_kept = rec->n_group1 = rec->n_group2 = rec->n_clip = rec->reserved = 0u;
            rec->call_min = kI64Max;
            rec->call_max = kI64Min;
        }
        return;
    }
    Partial p = no_pairs();
    for (uint64_t i = b + (uint64_t)lane; i < e; i += kWave) count_pair<UNPHASED>(a, i, p);
    const Partial t = wave_reduce(p);
    if (lane == 0) {
        const uint32_t kept = t.fetched_kept >> 16;
        rec->n_fetched = t.fetched_kept & 0xffffu;
        rec->n_kept = kept;
        rec->n_clip = t.clip;
        store_totals<UNPHASED>(rec, kept, t.group12 & 0xffffu, t.group12 >> 16, t.mn, t.mx);
    }
}

template <bool UNPHASED>
__global__ __launch_bounds__(256) void evidence_deep(EvidenceArgs a) {
    __shared__ Partial part[4];
    const int lane = lane_id();
    const uint32_t wave = threadIdx.x >> 6;
    const unsigned long long listed = a.work->n_slices;  // (written by the launch in front)
    const uint64_t n_listed = listed < a.list_cap ? listed : a.list_cap;
    for (uint64_t s = blockIdx.x; s < n_listed; s += gridDim.x) {
        const EvidenceSlice ent = a.list[s];
        // (a listed locus has passed evidence_shallow's checks of its offsets)
        const uint64_t lb = a.locus_pair_off[ent.locus], le = a.locus_pair_off[ent.locus + 1];
        const uint64_t b = lb + (uint64_t)ent.slice * kEvidenceSlice;
        const uint64_t e = le - b < kEvidenceSlice ? le : b + kEvidenceSlice;
        Partial p = no_pairs();
        for (uint64_t i = b + threadIdx.x; i < e; i += 256u) count_pair<UNPHASED>(a, i, p);
        const Partial w = wave_reduce(p);
        if (lane == 0) part[wave] = w;
        __syncthreads();
        if (threadIdx.x == 0) {
            Partial t = part[0];
            for (int k = 1; k < 4; ++k) {
                t.fetched_kept += part[k].fetched_kept, t.group12 += part[k].group12, t.clip += part[k].clip;
                t.mn = part[k].mn < t.mn ? part[k].mn : t.mn;
                t.mx = part[k].mx > t.mx ? part[k].mx : t.mx;
            }
            inq_locus_evidence_t *rec = a.evidence + ent.locus;
            constexpr int kRlx = __ATOMIC_RELAXED, kAgent = __HIP_MEMORY_SCOPE_AGENT;
            (void)__hip_atomic_fetch_add(&rec->n_fetched, t.fetched_kept & 0xffffu, kRlx, kAgent);
            (void)__hip_atomic_fetch_add(&rec->n_kept, t.fetched_kept >> 16, kRlx, kAgent);
            (void)__hip_atomic_fetch_add(&rec->n_clip, t.clip, kRlx, kAgent);
            if (!UNPHASED) {
                (void)__hip_atomic_fetch_add(&rec->n_group1, t.group12 & 0xffffu, kRlx, kAgent);
                (void)__hip_atomic_fetch_add(&rec->n_group2, t.group12 >> 16, kRlx, kAgent);
            }
            (void)__hip_atomic_fetch_min(&rec->call_min, t.mn, kRlx, kAgent);
            (void)__hip_atomic_fetch_max(&rec->call_max, t.mx, kRlx, kAgent);
            // the arrival: this slice's merges are released before the ticket is drawn; whoever draws the last one acquires them all
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const uint32_t n_slices = (uint32_t)((le - lb + kEvidenceSlice - 1) / kEvidenceSlice);
            const uint32_t ticket = __hip_atomic_fetch_add(&rec->reserved, 1u, kRlx, kAgent);
            if (ticket + 1u == n_slices) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                const uint32_t kept = __hip_atomic_load(&rec->n_kept, kRlx, kAgent);
                const uint32_t g1 = __hip_atomic_load(&rec->n_group1, kRlx, kAgent), g2 = __hip_atomic_load(&rec->n_group2, kRlx, kAgent);
                const int64_t mn = __hip_atomic_load(&rec->call_min, kRlx, kAgent), mx = __hip_atomic_load(&rec->call_max, kRlx, kAgent);
                store_totals<UNPHASED>(rec, kept, g1, g2, mn, mx);
            }
        }
        __syncthreads();  // part[] is free for the next slice
    }
}

}  // namespace

void launch_evidence(const EvidenceArgs &a, bool unphased, uint32_t grid_deep, hipStream_t s) {
    if (a.n_loci == 0) return;
    const uint32_t grid = (uint32_t)((a.n_loci + 3) / 4);
    if (unphased)
        hipLaunchKernelGGL(evidence_shallow<true>, dim3(grid), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(evidence_shallow<false>, dim3(grid), dim3(256), 0, s, a);
    if (a.list_cap == 0) return;
    if (unphased)
        hipLaunchKernelGGL(evidence_deep<true>, dim3(grid_deep), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(evidence_deep<false>, dim3(grid_deep), dim3(256), 0, s, a);
}

}  // namespace inq
