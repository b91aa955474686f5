// read_motifs.hip — the motif runs of the bases behind each Call (inq_read_motif_t): where the longest pure run of the locus's motif
// lies in a kept record's slice, how many bases pure runs of at least one motif copy cover, and how many such runs there are.
//
// Layout: one 16-lane row per kept record, four records per wave, sixteen per workgroup (kReadMotifTile); LANE r OF A ROW OWNS
// ROTATION r, lanes >= k idle.  All lanes of a row read the same 8 bytes of the slice per step, 16 bases, and each compares them with
// its own view of the motif: the word repeated to 32 nibbles, shifted by (16 * step + r) mod k.  XOR and a zero-nibble test give a
// 16-bit hit mask; the lane walks the mask's runs with count-trailing-zero steps and carries its open run's length (u32) to the next
// word, so a 40 000-base soft clip is the same loop as a 30-base window.  Whether a base lies in a run of >= k is known once the run
// has ended or has reached k: at a word's end at most k - 1 <= 14 trailing bases are undecided, all of them in that word, and the
// next word decides them.  So the coverage mask of word w - 1 is final while word w is handled; it is ORed across the row (four DPP
// steps) and pop-counted.  At the end a row maximum of (run_len, -run_beg), a row sum of the run counts and one 16-byte store.
// No LDS, no atomics, no workgroup waits for another: every output is a plain function of the inputs.
//
// Bounds: a record whose segment index, locus, offset or length lies outside what the launch holds gets four zeros and reads nothing
// of the bases; every byte read lies in [seg_off[p], seg_off[p] + (n + 1) / 2) and inside `bytes`; the odd last nibble is masked out
// of the hits, so neither it nor the next segment's first base can extend a run.
#include <hip/hip_runtime.h>

#include "read_motifs.h"
#include "slice_words.h"

namespace inq {
namespace {

constexpr uint32_t kThreads = 256;
static_assert(kReadMotifTile * kMotifRowLanes == kThreads, "a workgroup's lanes are dealt among its rows");
static_assert(kMotifRowLanes == (uint32_t)kRowLanes, "a row is one DPP row");
static_assert(sizeof(inq_read_motif_t) == 16, "a record is one 16-byte store");

// the motif repeated to 32 nibbles (nibble j = m[j mod k]); k = 0: no motif
struct Motif {
    unsigned __int128 rep;
    uint32_t k;
};
__device__ __forceinline__ Motif decode_motif(uint64_t word) {
    Motif M{0, (uint32_t)(word >> 60)};
    if (!M.k) return M;
    if (!motif_word_ok(word)) {  // every nibble one of 1, 2, 4, 8
        M.k = 0;
        return M;
    }
    M.rep = word & ~0ull >> (64u - 4u * M.k);
    for (uint32_t len = M.k; len < 32u; len *= 2u) M.rep |= M.rep << (4u * len);
    return M;
}

__global__ __launch_bounds__(256) void read_motif_kernel(ReadMotifArgs a) {
    const int lane = lane_id();
    const uint32_t rl = (uint32_t)lane & (kMotifRowLanes - 1u);
    const int row_shift = lane & ~(int)(kMotifRowLanes - 1u);  // where this row's bits lie in a ballot
    const uint64_t total = kept_total(a.n_kept, a.n_recs);
    // (the grid is capped, launch_read_motifs: a workgroup takes every gridDim.x-th tile)
    for (uint64_t base = (uint64_t)blockIdx.x * kReadMotifTile; base < total; base += (uint64_t)gridDim.x * kReadMotifTile) {
        const uint64_t rec = base + threadIdx.x / kMotifRowLanes;
        const bool has = rec < total;

        // the record's locus: the j with kept_off[j] <= rec < kept_off[j + 1]; what the search found is checked here
        const uint64_t lo = row_find_interval(a.kept_off, a.n_loci, rec, has, rl, row_shift);
        const bool found = has && lo < a.n_loci && a.kept_off[lo] <= rec && rec < a.kept_off[lo + 1];
        Motif M{0, 0u};
        if (found) M = decode_motif(a.motif[lo]);
        // (a record without a motif or without a slice has n = 0: no word is read, no lane has a hit)
        const Slice S = slice_of(a, rec, M.k != 0u);
        const uint8_t *const seg = S.seg;
        const uint64_t n = S.n, n_words = (n + 15u) / 16u, nb = (n + 1u) / 2u;
        const uint32_t k = M.k;
        const bool mine = rl < k;                 // this lane has a rotation
        const uint32_t step16 = k ? 16u % k : 0u;  // what 16 bases add to the phase
        uint32_t ph = mine ? rl : 0u;             // (16 w + r) mod k

        // the lane's runs: the open one's length at the last word's end, the longest and its start, the runs of >= k; the coverage of
        // the word before (cov_prev) and what of it waits for the open run to reach k (pend)
        uint32_t open = 0, best_len = 0, best_beg = 0, n_runs = 0, cov_prev = 0, pend = 0, covered = 0;
        auto finish = [&](uint32_t len, uint32_t beg) -> bool {
            if (len > best_len) best_len = len, best_beg = beg;  // (runs come in ascending order of their start: a tie keeps the first)
            if (len < k) return false;
            ++n_runs;
            return true;
        };
        for (uint64_t w = 0; ballot64(w < n_words); ++w) {
            const bool on = w < n_words;
            uint32_t h = 0, cov_cur = 0;
            if (on) {
                const uint64_t s = bases_in_order(load_segment_word(seg, nb, w));
                const uint64_t left = n - w * 16u;
                h = zero_nibbles(s ^ (uint64_t)(M.rep >> (4u * ph))) & (left >= 16u ? 0xffffu : (1u << (uint32_t)left) - 1u);
                if (!mine) h = 0u;
                ph += step16;
                if (ph >= k) ph -= k;
                const uint32_t pos0 = (uint32_t)(w * 16u);
                const uint32_t lead = (uint32_t)__builtin_ctz(~h | 0x10000u);  // hits that carry the open run on
                if (lead == 16u) {  // the whole word: the run is longer than any motif
                    open += 16u;
                    cov_prev |= pend;
                    pend = 0u;
                    cov_cur = 0xffffu;
                } else {
                    if (open + lead != 0u && finish(open + lead, pos0 - open)) cov_prev |= pend, cov_cur = (1u << lead) - 1u;
                    pend = 0u, open = 0u;
                    uint32_t hh = h & ~((1u << lead) - 1u);
                    while (hh) {
                        const uint32_t b = (uint32_t)__builtin_ctz(hh), len = (uint32_t)__builtin_ctz(~(hh >> b)), bits = ((1u << len) - 1u) << b;
                        if (b + len == 16u) {  // open at the word's end
                            open = len;
                            if (len >= k)
                                cov_cur |= bits;
                            else
                                pend = bits;
                        } else if (finish(len, pos0 + b)) {
                            cov_cur |= bits;
                        }
                        hh &= ~bits;
                    }
                }
            }
            // word w - 1 is decided now
            covered += (uint32_t)__popc(row_or(on ? cov_prev : 0u));
            if (on) cov_prev = cov_cur;
        }
        if (open != 0u && finish(open, (uint32_t)n - open)) cov_prev |= pend;
        covered += (uint32_t)__popc(row_or(cov_prev));
        // the longest run of the row, the smallest start among equals
        const uint64_t best = row_max_u64((uint64_t)best_len << 32 | (uint64_t)(0xffffffffu - best_beg));
        const uint32_t runs = row_inclusive_scan_u32(n_runs);
        if (has && rl == kMotifRowLanes - 1u)
            *reinterpret_cast<uint4 *>(a.recs + rec) = make_uint4(0xffffffffu - (uint32_t)best, (uint32_t)(best >> 32), covered, runs);
    }
}

}  // namespace

void launch_read_motifs(const ReadMotifArgs &a, uint32_t grid_side, hipStream_t s) {
    if (!a.n_recs || !a.motif) return;
    hipLaunchKernelGGL(read_motif_kernel, dim3(side_grid((a.n_recs + kReadMotifTile - 1) / kReadMotifTile, grid_side)), dim3(kThreads), 0, s, a);
}

}  // namespace inq
