// locus_motifs.hip — which short motif a locus's kept reads repeat (inq_locus_motif_t): the lag counts T_1 .. T_6 over all of the
// locus's slices, the period p they point to, the tandem copies at that period counted by rotation class, the winning class reduced to
// its primitive root as a motif word.
//
// Layout: ONE WORKGROUP OF FOUR WAVES PER LOCUS, the loci dealt to the grid by stride.  The workgroup's 256 lanes are sixteen 16-lane
// rows; row r takes the locus's records r, r + 16, ..., and lane l of a row takes the 16-base words l, l + 16, ... of its record's
// slice, each together with the word in front of it: six bases of look-back are all a lag of at most 6 needs, and they lie in that one
// word.  The slices are read twice.  Pass 1: XOR of the word against itself shifted by k nibbles (the word before shifted in), the
// zero-nibble test and a mask of the nibbles that are bases give 16 hit bits per lag; six pop-counts a word, u64 sums per lane, one
// reduction per locus.  Pass 2, p known: a tandem copy that ENDS at position e is p consecutive lag-p hits ending at e, so a lane
// owns the copies that end in its word; it needs the hits of the last p - 1 <= 5 positions of the word before, which compare with
// bases of that same word.  Each copy's p-mer, two bits a base with the first base on top so that numeric order is A < C < G < T
// order, is one integer add into a histogram of 4^p u64 bins in LDS (32 KB for p = 6): integer adds give the same sums in any order.
// Then every bin is added to the bin of its smallest rotation, the largest class (the smallest among equals) is found, and lane 0
// writes the record and use[j] with plain stores.  A locus of any depth is the same loop; no workgroup waits for another.
// While a row compares one record's words the next record's descriptor (kept_pair, seg_off, seg_len) is already loaded, so a record
// costs one round trip for its bases, not three in a chain.
//
// Bounds: a record whose segment index, offset or length lies outside what the launch holds contributes nothing, not to `bases`
// either, and nothing of it is read; every byte read lies in [seg_off[p], seg_off[p] + (n + 1) / 2) and inside `bytes`; positions at
// or past n are masked out of the hits, so neither the odd last nibble nor the next segment's first base is compared.
#include <hip/hip_runtime.h>

#include "locus_motifs.h"
#include "slice_words.h"

namespace inq {
namespace {

constexpr uint32_t kThreads = 256, kRows = kThreads / (uint32_t)kRowLanes, kWaves = kThreads / (uint32_t)kWave;
constexpr uint32_t kBins = 1u << (2u * kLocusMotifMaxPeriod);
static_assert(sizeof(inq_locus_motif_t) == 40, "five u64");

// bit t of the result: nibble t of x is a base, one of 1, 2, 4, 8
__device__ __forceinline__ uint32_t base_nibbles(uint64_t x) { return zero_nibbles(nibble_popcounts(x) ^ kNibbleOnes); }

// the positions t of the word cur at which base t equals the base k places in front of it (prev: the word before) and is a base
__device__ __forceinline__ uint32_t lag_hits(uint64_t prev, uint64_t cur, uint32_t k, uint32_t bases) {
    return zero_nibbles(cur ^ (cur << (4u * k) | prev >> (64u - 4u * k))) & bases;
}

// the sixteen bases of x as two bits each (A C G T = 0 1 2 3; what is no base gives bits nobody reads), base t in bits 2 t, 2 t + 1
__device__ __forceinline__ uint64_t two_bit_codes(uint64_t x) {
    uint64_t c = ((x >> 1 | x >> 3) & kNibbleOnes) | ((x >> 2 | x >> 3) & kNibbleOnes) << 1;
    c = (c | c >> 2) & 0x0f0f0f0f0f0f0f0full;
    c = (c | c >> 4) & 0x00ff00ff00ff00ffull;
    c = (c | c >> 8) & 0x0000ffff0000ffffull;
    return (c | c >> 16) & 0xffffffffull;
}
// the 32 two-bit groups of x in reverse order
__device__ __forceinline__ uint64_t reverse_pairs(uint64_t x) {
    const uint64_t r = __brevll(x);
    return (r >> 1 & 0x5555555555555555ull) | (r & 0x5555555555555555ull) << 1;
}

// a p-mer (first base on top) turned left by one base, and the smallest of its p rotations
__device__ __forceinline__ uint32_t turn(uint32_t v, uint32_t p) { return ((v << 2) | v >> (2u * (p - 1u))) & ((1u << (2u * p)) - 1u); }
__device__ __forceinline__ uint32_t smallest_rotation(uint32_t v, uint32_t p) {
    uint32_t best = v;
    for (uint32_t t = 1; t < p; ++t) {
        v = turn(v, p);
        best = v < best ? v : best;
    }
    return best;
}

// every 16-base word of the records [beg, end), the rows taking a record each and a row's lanes a word each: per_word(prev, cur, tail)
// with the word, the word before it (0 in front of the first) and the mask of cur's positions that lie inside the slice; per_record(n)
// once a record in lane 0 of its row.  No lane waits for another in here
template <class PerRecord, class PerWord>
__device__ __forceinline__ void walk_slices(const LocusMotifArgs &a, uint64_t beg, uint64_t end, PerRecord &&per_record, PerWord &&per_word) {
    const uint32_t row = threadIdx.x / kRowLanes, rl = threadIdx.x % kRowLanes;
    uint64_t rec = beg + row;
    Slice next = slice_of(a, rec, rec < end);
    while (rec < end) {
        const Slice S = next;
        rec += kRows;
        next = slice_of(a, rec, rec < end);  // in flight while this record's words are compared
        if (rl == 0u) per_record(S.n);
        const uint64_t nb = (S.n + 1u) / 2u, n_words = (S.n + 15u) / 16u;
        for (uint64_t w = rl; w < n_words; w += kRowLanes) {
            const uint64_t cur = bases_in_order(load_segment_word(S.seg, nb, w));
            const uint64_t prev = w ? bases_in_order(load_segment_word(S.seg, nb, w - 1u)) : 0ull;
            const uint64_t left = S.n - w * 16u;
            per_word(prev, cur, left >= 16u ? 0xffffu : (1u << (uint32_t)left) - 1u);
        }
    }
}

__global__ __launch_bounds__(256) void locus_motif_kernel(LocusMotifArgs a) {
    __shared__ unsigned long long bins[kBins];
    __shared__ unsigned long long sums[kLocusMotifMaxPeriod + 1];  // T_1 .. T_6, bases
    __shared__ unsigned long long wave_best[kWaves];               // a wave's best class: its count
    __shared__ uint32_t wave_best_class[kWaves];
    const uint32_t tid = threadIdx.x, lane = (uint32_t)lane_id(), wave = tid / (uint32_t)kWave;
    const uint64_t total = kept_total(a.n_kept, a.n_recs);
    for (uint64_t j = blockIdx.x; j < a.n_loci; j += gridDim.x) {
        uint64_t end = a.kept_off[j + 1], beg = a.kept_off[j];
        end = end < total ? end : total;
        beg = beg < end ? beg : end;

        // pass 1: the lag counts and the bases
        if (tid <= kLocusMotifMaxPeriod) sums[tid] = 0ull;
        __syncthreads();
        uint64_t t1 = 0, t2 = 0, t3 = 0, t4 = 0, t5 = 0, t6 = 0, n_bases = 0;
        walk_slices(
            a, beg, end, [&](uint64_t n) { n_bases += n; },
            [&](uint64_t prev, uint64_t cur, uint32_t tail) {
                const uint32_t bases = base_nibbles(cur) & tail;
                t1 += (uint32_t)__popc(lag_hits(prev, cur, 1u, bases));
                t2 += (uint32_t)__popc(lag_hits(prev, cur, 2u, bases));
                t3 += (uint32_t)__popc(lag_hits(prev, cur, 3u, bases));
                t4 += (uint32_t)__popc(lag_hits(prev, cur, 4u, bases));
                t5 += (uint32_t)__popc(lag_hits(prev, cur, 5u, bases));
                t6 += (uint32_t)__popc(lag_hits(prev, cur, 6u, bases));
            });
        t1 = wave_sum_u64(t1), t2 = wave_sum_u64(t2), t3 = wave_sum_u64(t3), t4 = wave_sum_u64(t4), t5 = wave_sum_u64(t5), t6 = wave_sum_u64(t6);
        n_bases = wave_sum_u64(n_bases);
        if (lane == 0u) {
            atomicAdd(&sums[0], (unsigned long long)t1), atomicAdd(&sums[1], (unsigned long long)t2), atomicAdd(&sums[2], (unsigned long long)t3);
            atomicAdd(&sums[3], (unsigned long long)t4), atomicAdd(&sums[4], (unsigned long long)t5), atomicAdd(&sums[5], (unsigned long long)t6);
            atomicAdd(&sums[6], (unsigned long long)n_bases);
        }
        __syncthreads();
        // the period: the smallest k whose count is the largest, none when every count is 0.  The same in every lane
        uint32_t p = 0;
        uint64_t tandem = 0;
        for (uint32_t k = 1; k <= kLocusMotifMaxPeriod; ++k)
            if (sums[k - 1u] > tandem) tandem = sums[k - 1u], p = k;
        n_bases = sums[kLocusMotifMaxPeriod];

        // pass 2: the tandem copies at lag p by their p-mer, then by their class
        uint32_t word_class = 0, root = 0;
        uint64_t copies = 0;
        if (p) {
            const uint32_t n_bins = 1u << (2u * p);
            for (uint32_t i = tid; i < n_bins; i += kThreads) bins[i] = 0ull;
            __syncthreads();
            // the copies that end in this word: their first hit u lies in [17 - p, 32 - p] of the two words' 32 positions
            const uint32_t owned = (uint32_t)((1ull << (33u - p)) - 1ull) & ~((1u << (17u - p)) - 1u);
            walk_slices(
                a, beg, end, [](uint64_t) {},
                [&](uint64_t prev, uint64_t cur, uint32_t tail) {
                    // (the first p positions of prev compare with zeros here and hit nothing: no owned copy reaches back to them)
                    const uint32_t h = lag_hits(0ull, prev, p, base_nibbles(prev)) | lag_hits(prev, cur, p, base_nibbles(cur) & tail) << 16;
                    uint32_t run = h;  // bit u: hits at u .. u + p - 1
                    for (uint32_t t = 1; t < p; ++t) run &= h >> t;
                    run &= owned;
                    if (!run) return;
                    const uint64_t codes = reverse_pairs(two_bit_codes(prev) | two_bit_codes(cur) << 32);  // position u in bits 2 (31 - u)
                    while (run) {
                        const uint32_t u = (uint32_t)__builtin_ctz(run);  // the copy is [u - p, u) and again [u, u + p)
                        run &= run - 1u;
                        atomicAdd(&bins[(uint32_t)(codes >> (2u * (32u - u))) & (n_bins - 1u)], 1ull);
                    }
                });
            __syncthreads();
            // a class's count is the sum over its members: every bin that is not its class's smallest rotation goes to the one that is.
            // Only such bins are read here and only the others are added to
            for (uint32_t i = tid; i < n_bins; i += kThreads) {
                const uint32_t c = smallest_rotation(i, p);
                const unsigned long long v = c != i ? bins[i] : 0ull;
                if (v) atomicAdd(&bins[c], v);
            }
            __syncthreads();
            // the largest class, the smallest among equals: a lane meets its classes in ascending order
            uint64_t best = 0;
            uint32_t best_class = 0xffffffffu;
            for (uint32_t i = tid; i < n_bins; i += kThreads) {
                const unsigned long long v = smallest_rotation(i, p) == i ? bins[i] : 0ull;
                if (v > best) best = v, best_class = i;
            }
            for (int d = 1; d < kWave; d *= 2) {
                const uint64_t o = __shfl_xor((unsigned long long)best, d, kWave);
                const uint32_t oc = (uint32_t)__shfl_xor((int)best_class, d, kWave);
                if (o > best || (o == best && oc < best_class)) best = o, best_class = oc;
            }
            if (lane == 0u) wave_best[wave] = best, wave_best_class[wave] = best_class;
            __syncthreads();
            best = 0, best_class = 0xffffffffu;
            for (uint32_t w = 0; w < kWaves; ++w)
                if (wave_best[w] > best || (wave_best[w] == best && wave_best_class[w] < best_class)) best = wave_best[w], best_class = wave_best_class[w];
            copies = best;
            if (copies) {
                // the primitive root: the shortest d dividing p such that turning the p-mer by d bases leaves it as it is
                uint32_t d = 1, turned = turn(best_class, p);
                for (; d < p; ++d, turned = turn(turned, p))
                    if (p % d == 0u && turned == best_class) break;
                word_class = best_class >> (2u * (p - d));  // its first d bases
                root = d;
            }
        }
        if (tid == 0u) {
            uint64_t word = 0;
            if (root) {
                word = (uint64_t)root << 60;
                for (uint32_t t = 0; t < root; ++t) word |= (uint64_t)(1u << (word_class >> (2u * (root - 1u - t)) & 3u)) << (4u * t);
            }
            inq_locus_motif_t *const f = a.found + j;
            f->word = word, f->period = p, f->bases = n_bases, f->tandem = p ? tandem : 0ull, f->copies = copies;
            if (a.use) {
                const uint64_t g = a.given ? a.given[j] : 0ull;
                a.use[j] = motif_word_ok(g) ? g : word;
            }
        }
        __syncthreads();  // the shared words are the next locus's from here on
    }
}

}  // namespace

void launch_locus_motifs(const LocusMotifArgs &a, uint32_t grid_side, hipStream_t s) {
    if (!a.n_loci) return;
    hipLaunchKernelGGL(locus_motif_kernel, dim3(side_grid(a.n_loci, grid_side)), dim3(kThreads), 0, s, a);
}

}  // namespace inq
