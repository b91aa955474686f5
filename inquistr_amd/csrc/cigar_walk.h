// cigar_walk.h — the per-read CIGAR walk of inquiSTR `call`, one wavefront per read.
//
// Restates, for a whole wave at once, what the reference does one op at a time:
//   call_from_cigar          src/call.rs:377-413   (indel / soft-clip sum inside the window)
//   Record::reference_end    src/call.rs:298,351   ([3P] htslib bam_endpos: second CIGAR walk)
//   read filters             src/call.rs:297-302 (unphased), 349-355 (phased)
//   fetch() overlap rule     src/call.rs:288,338   ([3P] htslib iterator)
// Both CIGAR walks of the reference are fused into ONE pass over the packed ops.  Two walks make that pass: walk_pairs_whole
// (every op of every read) and walk_pairs_rows (reads whose producer set INQ_READ_CHECKED, only as far as the window needs);
// walk_pairs picks one per block of <= 64 reads.  What they share stands above them, once: advance4, bad_ops,
// push_window_lanes, drain_queue, read_epilogue.
//
// Data path (per wave):
//   * both: one buffer_load_dwordx4 per lane (4 ops, 16 B), four loads in flight per wave, never predicated: the buffer
//     descriptor's range check returns 0 (= `0M`, a no-op) for an offset past num_records.
//   * whole: the wave is on one read at a time, in 256-op chunks (1 KiB per wave instruction, coalesced), flattened over reads
//     and the chunks of long reads.  Reference positions: advance4 in the lane + DPP wave scan + scalar carry between chunks.
//   * rows: every row of the wave is a read stream of its own.  Head: eight rows of 8 lanes walk the first four 128-byte lines of
//     every read, a line at a time, read k in a fixed row; the reads it does not settle go on from a list in LDS, in four rows
//     of 16 lanes and pieces of two lines.  Positions: advance4 + DPP row scan + a carry per row.
//   * both: only the few lanes whose ops can start inside [start_ext, end_ext) matter for the call: they are compacted into an
//     LDS queue (push_window_lanes) and evaluated 64 at a time (drain_queue, one entry per lane); their signed lengths land in
//     the owning read's LDS accumulator (ds_add_u64).  The per-op window/minlen/sign logic runs once per ~64 window lanes.
#pragma once
#include <type_traits>

#include "wave_primitives.h"

namespace inq {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// device status word bits (mapped to INQ_ERR_* by the host, same precedence as the oracle)
constexpr uint32_t ST_INDEX = 1u, ST_CIGAR_OP = 2u, ST_RANGE = 4u, ST_PHASE = 8u, ST_LOCUS = 16u, ST_HINT = 32u, ST_AUX = 64u,
                   ST_INTERNAL = 128u;  // a grid barrier of locus_call_tail gave up waiting (never seen; the grid drains all the same)

// per-pair meta byte: low 3 bits are the public INQ_PAIR_* bits
constexpr uint32_t PM_CLIP = 1u, PM_FETCHED = 2u, PM_KEPT = 4u;
constexpr int PM_GRP_SHIFT = 4;  // bits 4-5: haplotype group 0 (none) / 1 / 2
constexpr uint32_t PM_CHOSEN = 64u;

constexpr uint32_t RB_UNMAPPED = 1u, RB_REVERSE = 2u, RB_HAS_HP = 4u, RB_IS_2D = 8u, RB_SA_PANIC = 16u;

constexpr int kQueueCap = 128;  // window-lane queue entries per wave

struct Window {
    uint32_t se;     // start_ext = start - 10            (src/call.rs:285,335)
    uint32_t ee;     // end_ext   = end + 10              (src/call.rs:286,336)
    uint32_t se1;    // se + 1
    uint32_t width;  // ee - se1: an op at refpos counts iff (refpos - se1) <u width  ==  se < refpos < ee; 0 when ee < se1
    uint32_t minlen;
};

// The window of a locus.  end + 10 may pass 2^32 and wrap, as it does in the reference's release build
// (src/call.rs:286,336); then end_ext < start_ext and `start_ext < refpos && refpos < end_ext` (:387-403) holds
// for no position at all.  ee - se1 would instead describe the positions from start_ext + 1 round to end_ext - 1,
// 0 .. end + 9 - 2^32 among them, so a wrapped window gets width 0: no op counts.
__device__ __forceinline__ Window make_window(uint32_t start, uint32_t end, uint32_t minlen) {
    Window W;
    W.se = start - 10u;
    W.ee = end + 10u;
    W.se1 = W.se + 1u;
    W.width = W.ee >= W.se1 ? W.ee - W.se1 : 0u;
    W.minlen = minlen;
    return W;
}

struct BatchView {
    const uint4 *cigar4;  // packed ops viewed as 16-byte groups
    const uint4 *reads;   // inq_read_t as uint4: x=cigar_off4 y=n_cigar z=pos w=mapq|bits<<8|phase<<16
    const uint32_t *pair_read;
    uint64_t n_reads;
    uint64_t n_cigar4;  // n_cigar_words / 4
};

// LDS owned by one wave
struct QueueEntry {
    u32x4 w;     // the lane's 4 packed ops
    uint2 info;  // .x = reference position of the first op minus (start_ext+1); .y = read slot | is2d<<6
    uint2 pad;   // 32-byte stride: one address register serves both stores; holds the continuation list (cont_put)
};
struct WaveLds {
    QueueEntry q[kQueueCap];
    unsigned long long acc[64];  // per read slot: the Call value (two's complement)
    unsigned int flags[64];      // per read slot: bit0 = a soft clip was counted
    unsigned int endc[64];       // per read slot: reference_position after the last op walked (walk_pairs_rows)
};

// four waves x 5 120 B = 20 480 B per workgroup: eight workgroups fill a CU's 160 KB at 8 waves per SIMD
static_assert(sizeof(WaveLds) == 5120, "a larger WaveLds costs resident workgroups per CU");
// The continuation list of walk_pairs_rows, up to 64 reads to go on behind the head: entry i is the read's next group and its
// row word (rw_pack) in q[i].pad, the position reached in q[64 + i].pad.x.  It outlives the queue's pushes and drains because
// push_window_lanes, the one store to the queue, writes .w and .info and never a whole QueueEntry.  (i is unsigned in put and
// signed in get, as the two callers hold it: a cast at either changes the addresses the compiler forms.)
static_assert(kQueueCap >= 128, "the list takes the spare words of 128 queue entries");
__device__ __forceinline__ void cont_put(WaveLds &L, uint32_t i, uint32_t cur4, uint32_t rw, uint32_t carry) {
    L.q[i].pad = make_uint2(cur4, rw);
    L.q[64u + i].pad.x = carry;
}
__device__ __forceinline__ void cont_get(const WaveLds &L, int i, uint32_t &cur4, uint32_t &rw, uint32_t &carry) {
    const uint2 r = L.q[i].pad;
    cur4 = r.x, rw = r.y;
    carry = L.q[64 + i].pad.x;
}

// Per-lane descriptor of the pair this lane "owns" inside a block of <= 64 pairs.
struct PairMeta {
    uint32_t off4, nc, pos, misc;
};

// Loads descriptors for pairs [first, first+cnt): lane l < cnt owns pair first+l.
// A descriptor that points outside the buffers is replaced by an empty read and flagged.
__device__ __forceinline__ PairMeta load_pair_meta(const BatchView &b, uint64_t first, int cnt, int lane,
                                                    uint32_t &status, bool &valid) {
    PairMeta m{0u, 0u, 0u, 0u};
    valid = false;
    if (lane < cnt) {
        uint32_t ri = b.pair_read[first + (uint64_t)lane];
        if ((uint64_t)ri < b.n_reads) {
            uint4 r = b.reads[ri];
            uint64_t n4 = ((uint64_t)r.y + 3u) >> 2;
            if (r.y < 0x10000000u && (uint64_t)r.x + n4 <= b.n_cigar4) {
                m.off4 = r.x;
                m.nc = r.y | ((r.w & (RB_IS_2D << 8)) ? 0x80000000u : 0u);  // bit 31 = is_accidental_2d
                m.pos = r.z;
                m.misc = r.w;
                valid = true;
            } else {
                status |= ST_INDEX;
            }
        } else {
            status |= ST_INDEX;
        }
    }
    return m;
}

// The same in two stages, so a wave can fetch the descriptors of its NEXT block of reads while it walks
// the current one: stage A (pair index) one block ahead of stage B (descriptor), checks at use time.
__device__ __forceinline__ uint32_t meta_stage_a(const BatchView &b, uint64_t first, int cnt, int lane) {
    return lane < cnt ? b.pair_read[first + (uint64_t)lane] : 0xffffffffu;
}
__device__ __forceinline__ uint4 meta_stage_b(const BatchView &b, uint32_t ri) {
    // ri comes from a completed stage A; out-of-range indices load nothing and are flagged in stage C
    return (uint64_t)ri < b.n_reads ? b.reads[ri] : make_uint4(0u, 0xffffffffu, 0u, 0u);
}
__device__ __forceinline__ PairMeta meta_stage_c(const BatchView &b, const uint4 r, int cnt, int lane, uint32_t &status,
                                                  bool &valid) {
    PairMeta m{0u, 0u, 0u, 0u};
    valid = false;
    if (lane < cnt) {
        const uint64_t n4 = ((uint64_t)r.y + 3u) >> 2;
        if (r.y < 0x10000000u && (uint64_t)r.x + n4 <= b.n_cigar4) {
            m.off4 = r.x;
            m.nc = r.y | ((r.w & (RB_IS_2D << 8)) ? 0x80000000u : 0u);
            m.pos = r.z;
            m.misc = r.w;
            valid = true;
        } else {
            status |= ST_INDEX;
        }
    }
    return m;
}

// ops that consume the reference: M D N = X -> bits 0,2,3,7,8 (src/call.rs:384-392,404)
constexpr uint32_t kConsume = 0x18Du;

// len if the op consumes the reference, else 0 (v_bfe_i32 + v_and): drain_queue's form
__device__ __forceinline__ uint32_t ref_advance(uint32_t op, uint32_t len) {
    return len & (uint32_t)__builtin_amdgcn_sbfe((int)kConsume, op, 1u);
}
// Same from the raw packed word, without extracting the op: v_bfe_i32 takes its bit offset from
// the low FIVE bits of the word (op | len&1 << 4), so the 9-entry table is laid down twice.
// The table's answer (-1 or 0) is then the WIDTH of a v_bfe_u32 at offset 4 in place of a shift and an and: the
// instruction takes its width from the low five bits of that operand, so -1 asks for 31 bits from bit 4 - the word
// has only the 28 length bits there and none is lost - and 0 asks for none, which yields 0.  Two instructions per op.
constexpr uint32_t kConsume32 = kConsume | (kConsume << 16);
__device__ __forceinline__ uint32_t ref_advance_raw(uint32_t w) {
    return __builtin_amdgcn_ubfe(w, 4u, (uint32_t)__builtin_amdgcn_sbfe((int)kConsume32, w, 1u));
}
// bit 0 of (kBadOp32 >> (w & 31)) is set iff the op code is 9..15 (rust-htslib cigar() panics)
constexpr uint32_t kBadOp32 = 0xFE00FE00u;
__device__ __forceinline__ uint32_t bad_ops(const u32x4 w) {
    return (kBadOp32 >> (w.x & 31u)) | (kBadOp32 >> (w.y & 31u)) | (kBadOp32 >> (w.z & 31u)) | (kBadOp32 >> (w.w & 31u));
}
// Reference span of a lane's four ops: up to the second, third and fourth op, and of all four.
__device__ __forceinline__ void advance4(const u32x4 w, uint32_t &e1, uint32_t &e2, uint32_t &e3, uint32_t &tot) {
    e1 = ref_advance_raw(w.x), e2 = e1 + ref_advance_raw(w.y);
    e3 = e2 + ref_advance_raw(w.z), tot = e3 + ref_advance_raw(w.w);
}

// Evaluates the queued window lanes: entry e -> lane e.  src/call.rs:387-403 for 4 ops per lane.  (The ops are extracted here
// anyway, so the advance is taken from (op, len): through advance4 the compiler lays the whole kernel out differently.)
__device__ __forceinline__ void drain_queue(WaveLds &L, uint32_t &qcount, const Window &W, int lane) {
    // single-wave LDS traffic: DS instructions of one wave execute in issue order, so the queue
    // writes above are visible to the reads below without a fence; wave_barrier only pins the
    // compiler's schedule
    __builtin_amdgcn_wave_barrier();
    for (uint32_t base = 0; base < qcount; base += 64u) {
        const uint32_t e = base + (uint32_t)lane;
        if (e < qcount) {
            const u32x4 w = L.q[e].w;
            const uint2 info = L.q[e].info;
            const uint32_t rel = info.x;
            const uint32_t slot = info.y & 63u;
            // soft clips of an accidental-2D read never count (src/call.rs:394): drop S from the candidates
            const uint32_t cand_mask = (info.y & 64u) ? 0x06u : 0x16u;  // I=1, D=2, S=4
            const uint32_t op0 = w.x & 15u, op1 = w.y & 15u, op2 = w.z & 15u, op3 = w.w & 15u;
            const uint32_t l0 = w.x >> 4, l1 = w.y >> 4, l2 = w.z >> 4, l3 = w.w >> 4;
            const uint32_t e1 = ref_advance(op0, l0), e2 = e1 + ref_advance(op1, l1), e3 = e2 + ref_advance(op2, l2);
            int32_t s = 0;
            uint32_t clip = 0;
#define INQ_OP(op, len, ee_)                                                                              \
    {                                                                                                     \
        const bool hit = ((cand_mask >> (op)) & 1u) && (len) > W.minlen && (rel + (ee_)) < W.width;        \
        const int32_t v = ((op) == 2u) ? -(int32_t)(len) : (int32_t)(len);                                \
        s += hit ? v : 0;                                                                                 \
        clip |= (hit && (op) == 4u) ? 1u : 0u;                                                            \
    }
            INQ_OP(op0, l0, 0u)
            INQ_OP(op1, l1, e1)
            INQ_OP(op2, l2, e2)
            INQ_OP(op3, l3, e3)
#undef INQ_OP
            if (s != 0) atomicAdd(&L.acc[slot], (unsigned long long)(long long)s);  // |s| < 4 * 2^28
            if (clip) atomicOr(&L.flags[slot], 1u);
        }
    }
    qcount = 0;
    __builtin_amdgcn_wave_barrier();
}

// Compacts the lanes with `inw` set behind the queue's qcount entries.  x = position after the lane's ops relative to
// start_ext + 1, tot = their span, info & info_mask = read slot | is_2d << 6: x - tot and the mask are taken under `inw`, where
// only window lanes pay for them.  True when the queue has grown past 64 entries: the caller drains it.
__device__ __forceinline__ bool push_window_lanes(WaveLds &L, uint32_t &qcount, bool inw, const u32x4 w, uint32_t x,
                                                  uint32_t tot, uint32_t info, uint32_t info_mask) {
    const uint64_t mask = ballot64(inw);
    if (mask) {
        QueueEntry *const tail = &L.q[qcount];  // wave-uniform
        if (inw) {
            const uint32_t idx = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
            tail[idx].w = w;  // .w and .info, never a whole QueueEntry: .pad is the continuation list's
            tail[idx].info = make_uint2(x - tot, info & info_mask);
        }
        qcount += (uint32_t)__popcll(mask);
    }
    return mask != 0ull && qcount > 64u;
}

// Per-read epilogue, one read per lane: lane k < cnt turns read k's walk (end_carry = reference_position after
// the last op walked, the LDS accumulators) into the pair's Call and meta bits.
template <bool UNPHASED>
__device__ __forceinline__ void read_epilogue(const PairMeta &m, bool valid, int cnt, const Window &W, int lane,
                                              uint32_t end_carry, uint32_t &status, WaveLds &L, int64_t &val,
                                              uint32_t &meta) {
    val = 0;
    meta = 0;
    if (lane < cnt && valid) {
        const uint32_t pos = m.pos;
        const uint32_t mapq = m.misc & 0xffu, bits = (m.misc >> 8) & 0xffu, phase = (m.misc >> 16) & 0xffu;
        // [3P] bam_endpos: rlen = unmapped ? 0 : sum(ref-consuming); rlen == 0 -> 1
        uint32_t rlen = end_carry - (pos + 1u);
        if ((bits & RB_UNMAPPED) || rlen == 0u) rlen = 1u;
        const uint32_t rend = pos + rlen;  // reference_end() as u32
        // fetch(): pos < end_ext && endpos > start_ext (signed pos, pos >= -1 inside the domain)
        const bool fetched = ((int32_t)pos < 0 || pos < W.ee) && rend > W.se;
        bool skip;
        if (UNPHASED)
            skip = W.se < pos || rend < W.ee || mapq <= 10u;  // src/call.rs:297-302
        else
            skip = !(bits & RB_HAS_HP) || (W.se < pos && rend < W.ee) || mapq <= 10u;  // :349-355
        const bool kept = fetched && !skip;
        uint32_t grp = 0u;
        bool bad_phase = false;
        if (!UNPHASED && kept) {
            if (phase > 2u)
                bad_phase = true;  // calls.get_mut(&phase).unwrap() panics, src/call.rs:358
            else
                grp = phase;
        }
        if (bad_phase) status |= ST_PHASE;
        // is_accidental_2d panics on this read's SA, but the reference only calls it from call_from_cigar,
        // i.e. for reads that passed the filter (src/call.rs:303,357 -> :394)
        if (kept && (bits & RB_SA_PANIC)) status |= ST_AUX;
        val = (int64_t)L.acc[lane];
        meta = ((L.flags[lane] & 1u) ? PM_CLIP : 0u) | (fetched ? PM_FETCHED : 0u) | (kept ? PM_KEPT : 0u) |
               (grp << PM_GRP_SHIFT);
    }
}

// Walks the WHOLE CIGAR of the reads of pairs [0, cnt) described by `m` (lane k owns pair k), the whole
// wave on one read at a time.  On return lane k holds the pair's Call (src/call.rs:67-71) in `val` and
// PM_CLIP | PM_FETCHED | PM_KEPT | group in `meta`.
template <bool UNPHASED, int AUX>
__device__ __forceinline__ void walk_pairs_whole(const BatchView &b, const PairMeta &m, bool valid, int cnt,
                                           const Window &W, int lane, uint32_t &status, WaveLds &L, int64_t &val,
                                           uint32_t &meta) {
    L.acc[lane] = 0ull;
    L.flags[lane] = 0u;
    uint32_t qcount = 0;
    uint32_t lane_range = 0, lane_bad = 0;
    uint32_t end_carry = 0;  // lane k: reference_position after the last op of read k

    // (a scalar pair of its own for the CIGAR's base: taken from the kernel's argument block at every load, that whole block has
    // to stay in scalar registers through the loop, or be restored from spill lanes in every step)
    const uint4 *cigar4 = b.cigar4;
    asm volatile("" : "+s"(cigar4));
    // ---- load cursor: runs 4 chunk loads ahead of the compute cursor ----
    int hk = 0;
    uint32_t hc = 0, h_nchunks = 1, h_off4 = 0, h_n4 = 0;
    auto head_load = [&]() {
        if (hk < cnt) {
            h_off4 = readlane_u32(m.off4, hk);
            const uint32_t nc = readlane_u32(m.nc, hk) & 0x7fffffffu;
            h_n4 = (nc + 3u) >> 2;
            h_nchunks = max(1u, (nc + 255u) >> 8);
        } else {
            h_off4 = 0;
            h_n4 = 0;
            h_nchunks = 1;
        }
    };
    auto issue = [&]() -> u32x4 {
        // raw buffer load: offsets at or beyond num_records return 0, no exec masking needed
        const __amdgpu_buffer_rsrc_t rsrc =
            __builtin_amdgcn_make_buffer_rsrc((void *)(cigar4 + h_off4), (short)0, (int)(h_n4 * 16u), 0x00020000);
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)((hc * 64u + (uint32_t)lane) * 16u), 0, AUX);
        ++hc;
        if (hc >= h_nchunks) {
            ++hk;
            hc = 0;
            head_load();
        }
        return v;
    };
    head_load();
    u32x4 qa = issue(), qb = issue(), qc = issue(), qd = issue();

    // ---- compute cursor ----
    int tk = 0;
    uint32_t tc = 0, t_nchunks = 1, t_nc = 0, t_info = 0, carry = 0;
    auto tail_load = [&]() {
        if (tk < cnt) {
            const uint32_t ncp = readlane_u32(m.nc, tk);
            t_nc = ncp & 0x7fffffffu;
            t_nchunks = max(1u, (t_nc + 255u) >> 8);
            carry = readlane_u32(m.pos, tk) + 1u;  // (reference_start + 1) as u32, src/call.rs:380
            t_info = (uint32_t)tk | ((ncp >> 31) << 6);
            lane_range |= carry;
        }
    };
    tail_load();

    auto step = [&](const u32x4 w) {
        uint32_t e1, e2, e3, tot;
        advance4(w, e1, e2, e3, tot);
        const uint32_t incl = wave_inclusive_scan_u32(tot);
        lane_bad |= bad_ops(w);
        lane_range |= carry + incl;
        // x = position after this lane's ops, relative to start_ext + 1.  One of the lane's ops can start
        // inside the window only if 0 <= x and x - tot < width  <=>  x <u width + tot  (all < 2^31 inside
        // the parity domain).  Zero-filled lanes behind a read that ends inside the window pass the test too;
        // they queue four `0M` that contribute nothing, which is cheaper than a second compare on every chunk.
        const uint32_t x = (carry - W.se1) + incl;
        if (push_window_lanes(L, qcount, x < W.width + tot, w, x, tot, t_info, ~0u)) drain_queue(L, qcount, W, lane);
        carry += readlane_u32(incl, 63);
        ++tc;
        if (tc >= t_nchunks) {
            end_carry = writelane_u32(end_carry, carry, tk);  // lane tk <- carry
            ++tk;
            tc = 0;
            tail_load();
        }
    };

    // four named buffers, no register rotation: each step waits only for its own load (vmcnt(3))
    while (tk < cnt) {
        step(qa);
        qa = issue();
        if (tk < cnt) step(qb);
        qb = issue();
        if (tk < cnt) step(qc);
        qc = issue();
        if (tk < cnt) step(qd);
        qd = issue();
    }
    if (qcount) drain_queue(L, qcount, W, lane);
    if (ballot64((lane_bad & 1u) != 0u)) status |= ST_CIGAR_OP;  // rust-htslib cigar() would panic
    if (ballot64((lane_range >> 31) != 0u)) status |= ST_RANGE;

    read_epilogue<UNPHASED>(m, valid, cnt, W, lane, end_carry, status, L, val, meta);
}

// ---- window-bounded walk ---------------------------------------------------------------------------------
// A read whose descriptor carries INQ_READ_CHECKED (inq_read_t.promise, bits 24-31 of the uint4's .w) has had
// the domain rules checked by its producer: op codes <= 8, pos >= -1, pos + 1 + reference span < 2^31.  Its
// CIGAR is then only needed up to the window: no op that starts at or past end_ext counts (reference positions
// never decrease), and a lower bound of bam_endpos that is already >= end_ext settles the fetch rule and both
// filters (rend > start_ext, rend < end_ext) exactly as the true value does.
//
// Shape: four load slots per wave, as in the whole walk, but every row of a slot is a read stream of its own (one
// buffer_load_dwordx4 per lane, see kLineMask below for where the pieces lie).  In the head a slot is 8 rows of kHeadLanes = 8
// lanes and a piece one line of up to 32 ops; behind it 4 rows of kRowLanes = 16 lanes and a piece two lines.  The stop is
// tested after every piece, so nothing is loaded past the piece in which a read stops.  A checked read stops after the
// piece that takes carry = pos + 1 + consumed past end_ext (carry > end_ext <=> pos + consumed >= end_ext, without the
// u32 wrap of pos = -1); an unchecked one is walked to its end, with the device's own domain checks.
constexpr uint32_t RP_CHECKED = 1u;  // INQ_READ_CHECKED

// (a row behind the head = one read stream = one DPP row of kRowLanes lanes: its scan and its last lane are wave_primitives.h's)

// The head phase's rows are half DPP rows: kHeadLanes = 8 lanes, one 128-byte line per load.
constexpr int kHeadLanes = 8;
constexpr int kHeadLines = 4;  // lines of a read the head phase walks before the list takes it
// Inclusive prefix sum and total inside each 8-lane row, exact in wrapping u32: the 16-lane scan, less the lower half's
// total (lane 7 of the DPP row) in the upper half; the total is then lane 7 of the half.  ds_swizzle in bit-mask mode reads
// lane ((l & and) | or): and = 0x10 keeps the DPP row, and = 0x18 the half.
__device__ __forceinline__ void head_row_scan_u32(uint32_t x, bool upper, uint32_t &incl, uint32_t &tot) {
    const uint32_t s = row_inclusive_scan_u32(x);
    const uint32_t lower = (uint32_t)__builtin_amdgcn_ds_swizzle((int)s, 0x10 | (0x07 << 5));
    incl = s - (upper ? lower : 0u);
    tot = (uint32_t)__builtin_amdgcn_ds_swizzle((int)incl, 0x18 | (0x07 << 5));
}

// One read stream: the same value in every lane of a row.
struct RowStream {
    uint32_t cur4;   // the next 16-byte group of the read this row loads (the piece's first); in the head see head_issue
    uint32_t carry;  // (reference_start + 1) + reference span of the ops walked so far, u32
    uint32_t st;     // groups left << RS_LEFT | RS_LIVE | RS_STOP | is_2d << 6 | read slot; 0 = idle
};
constexpr uint32_t RS_STOP = 128u, RS_LIVE = 256u;
constexpr int RS_LEFT = 9;
// Where the pieces lie.  A read starts on a 16-byte boundary, off4 & 7 groups into a 128-byte line of the batch's CIGAR.
// Every piece ends on a line boundary, so no line is asked for by two loads of one read.  The head's pieces are single lines:
// the first holds the read's groups from off4 to the end of its line, 8 - (off4 & 7) of them, every later one a whole line.
// Behind the head a piece ends on the second line boundary behind its start: lane rl of the row loads group (cur4 & ~7) + rl,
// and the lanes before cur4 and past the read's end get the out-of-range offset; the head hands a read over on a line
// boundary, so these are two whole lines each.
constexpr uint32_t kLineMask = 7u;  // groups of a 128-byte line - 1
// st holds at most 2^23 - 1 groups left: a read of kRowMaxGroups groups or more (n_cigar > 2^25 - 4) sends its block to
// the whole walk
constexpr uint32_t kRowMaxGroups = 1u << (32 - RS_LEFT);
__host__ __device__ constexpr uint32_t cigar_groups(uint32_t nc) { return (nc + 3u) >> 2; }
static_assert(cigar_groups((1u << 25) - 4u) == kRowMaxGroups - 1u && cigar_groups((1u << 25) - 3u) == kRowMaxGroups,
              "the longest read the row walk takes is 2^25 - 4 ops");
// The row word, what a row needs of a read besides where it is and how far it has got: groups left (< kRowMaxGroups) |
// slot << 23 | is_2d << 30 | promised << 31.  The owning lane's register holds it with slot 0, the continuation list with the slot.
constexpr int RW_SLOT = 23, RW_2D = 30, RW_PROMISED = 31;
static_assert((kRowMaxGroups - 1u) >> RW_SLOT == 0u && (63u << RW_SLOT) >> RW_2D == 0u, "the fields of the row word lie apart");
__device__ __forceinline__ uint32_t rw_pack(uint32_t groups, uint32_t is_2d, bool promised) {
    return groups | (is_2d << RW_2D) | (promised ? 1u << RW_PROMISED : 0u);
}
__device__ __forceinline__ uint32_t rw_groups(uint32_t rw) { return rw & (kRowMaxGroups - 1u); }
// of a word with slot 0, for `assign`: with rw_groups' 23-bit mask there the compiler allocates locus_call_small's registers
// differently (60 VGPRs, 76 instructions fewer, a kernel nobody has timed), so `assign` keeps the 30-bit mask it always had
__device__ __forceinline__ uint32_t rw_groups_slot0(uint32_t rw) { return rw & ((1u << RW_2D) - 1u); }
__device__ __forceinline__ uint32_t rw_slot(uint32_t rw) { return (rw >> RW_SLOT) & 63u; }
__device__ __forceinline__ uint32_t rw_2d(uint32_t rw) { return (rw >> RW_2D) & 1u; }
__device__ __forceinline__ bool rw_promised(uint32_t rw) { return (rw >> RW_PROMISED) != 0u; }
__device__ __forceinline__ uint32_t row_state(uint32_t groups, uint32_t slot, uint32_t is_2d, bool promised) {  // RowStream::st
    return (groups << RS_LEFT) | slot | (is_2d << 6) | (promised ? RS_STOP : 0u) | RS_LIVE;
}

// Same contract as walk_pairs_whole.  Needs a window that does not wrap (end_ext >= start_ext + 1) and a batch
// CIGAR under 4 GiB (one buffer descriptor over all of it; 32-bit byte offsets).  `checks` (wave-uniform): some
// read of the block is not promised, so every piece gets the device's own domain checks; a block whose reads are
// all promised walks without them.
//
// Two phases.  The head: a block is walked in passes of 32 reads, read k of the pass in row k % 8 of slot k / 8 for up to
// kHeadLines lines - no claim, no list, no ballot but the wave-uniform one that skips a slot whose rows are all idle; most
// promised reads stop inside it.  The reads that have not (long, far from their window, or unpromised) are then compacted into
// a list in LDS (cont_put: the spare words of the lane queue's entries) and walked on in two-line pieces by 16-lane rows that
// take the next of them whenever they fall idle.
template <bool UNPHASED, int AUX>
__device__ __forceinline__ void walk_pairs_rows(const BatchView &b, const PairMeta &m, bool valid, int cnt,
                                                const Window &W, int lane, bool checks, uint32_t &status, WaveLds &L,
                                                int64_t &val, uint32_t &meta) {
    L.acc[lane] = 0ull;
    L.flags[lane] = 0u;
    L.endc[lane] = m.pos + 1u;  // (reference_start + 1) as u32, src/call.rs:380: where a read with nothing to load ends
    uint32_t qcount = 0;
    // bit 0: an op code 9..15 was seen, bit 1: a reference position reached 2^31
    uint32_t lane_err = ((m.pos + 1u) >> 31) << 1;
    const uint64_t row_heads = 0x0001000100010001ull;  // lane 0 of each row
    // out-of-range offsets (past num_records) load 0 = `0M`: lanes past a read's end and idle rows
    const __amdgpu_buffer_rsrc_t rsrc =
        __builtin_amdgcn_make_buffer_rsrc((void *)b.cigar4, (short)0, (int)(uint32_t)(b.n_cigar4 * 16u), 0x00020000);

    // read k's row word in lane k; an empty read where none is owned
    const uint32_t d_w = rw_pack(cigar_groups(m.nc & 0x0fffffffu), m.nc >> 31, ((m.misc >> 24) & RP_CHECKED) != 0u);

    const int rl = lane & (kRowLanes - 1);
    // the head phase's row: 8 lanes, one line; the upper half of a DPP row is a row of its own
    const int hl = lane & (kHeadLanes - 1);
    const int hrow = lane >> 3;
    const bool upper = (lane & kHeadLanes) != 0;

    // a piece on the line grid: the lanes from cur4 to the second line boundary behind it that the read still has groups for
    auto issue = [&](const RowStream &S) -> u32x4 {
        const uint32_t g = (S.cur4 & ~kLineMask) + (uint32_t)rl;
        const bool on = g - S.cur4 < (S.st >> RS_LEFT);
        return __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(on ? g * 16u : 0xfffffff0u), 0, AUX);
    };
    // The head's rows count a read's groups from the start of the line it starts in, so every line is 8 groups to them, and
    // hold in cur4 not a group but the byte offset of the lane's own group of the next line.
    auto head_issue = [&](const RowStream &S) -> u32x4 {
        return __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)((uint32_t)hl < (S.st >> RS_LEFT) ? S.cur4 : 0xfffffff0u), 0, AUX);
    };
    // One piece of every row of a slot: LANES = 8 in the head, 16 behind it.  `last` (wave-uniform, head only): the row gives
    // its read up whether it has stopped or not; the read's owner finds the position reached in L.endc either way.
    auto step = [&](const u32x4 w, RowStream &S, auto lanes, bool last) {
        constexpr uint32_t LANES = decltype(lanes)::value;
        const bool live = S.st != 0u;
        uint32_t e1, e2, e3, tot, incl, rtot;
        advance4(w, e1, e2, e3, tot);
        if (LANES == (uint32_t)kHeadLanes) {
            head_row_scan_u32(tot, upper, incl, rtot);
        } else {
            incl = row_inclusive_scan_u32(tot);
            rtot = row_last(incl);
        }
        if (checks) {
            if (live) {
                lane_err |= bad_ops(w) & 1u;
                lane_err |= ((S.carry + incl) >> 31) << 1;
            }
        }
        // the window-lane test of walk_pairs_whole, per row
        const uint32_t x = (S.carry - W.se1) + incl;
        if (push_window_lanes(L, qcount, live && x < W.width + tot, w, x, tot, S.st, 127u)) drain_queue(L, qcount, W, lane);
        S.carry += rtot;
        if (LANES == (uint32_t)kHeadLanes) {
            S.cur4 += 16u * LANES;
            // (an idle row has no groups left: it is `done` and stays idle)
            const bool done = last || (S.st >> RS_LEFT) <= LANES || ((S.st & RS_STOP) && S.carry > W.ee);
            if (live && done && hl == 0) L.endc[S.st & 63u] = S.carry;
            S.st = done ? 0u : S.st - (LANES << RS_LEFT);
        } else {
            // the piece ran from cur4 to a line boundary: lim groups
            const uint32_t end4 = (S.cur4 & ~kLineMask) + LANES;
            const uint32_t lim = end4 - S.cur4;
            S.cur4 = end4;
            if (live) {
                if ((S.st >> RS_LEFT) <= lim || ((S.st & RS_STOP) && S.carry > W.ee)) {
                    if (rl == 0) L.endc[S.st & 63u] = S.carry;
                    S.st = 0u;
                } else {
                    S.st -= lim << RS_LEFT;
                }
            }
        }
    };
    using Head = std::integral_constant<uint32_t, (uint32_t)kHeadLanes>;
    using Later = std::integral_constant<uint32_t, (uint32_t)kRowLanes>;

    // ---- head: read k of the pass is slot k / 8's row k % 8, for up to kHeadLines lines ----
    // The descriptors wait for their rows in LDS, not in registers: read k's first group and row word in the words the
    // continuation list takes over behind the head (q[k].pad), its start position in L.endc[k].
    L.q[lane].pad = make_uint2(m.off4, d_w);
    __builtin_amdgcn_wave_barrier();
    // ... and loads the first line: the lanes from the read's start on
    auto assign = [&](RowStream &S, int k0) -> u32x4 {
        S.st = 0u;
        uint32_t voff = 0xfffffff0u;
        if (k0 < cnt) {  // wave-uniform; k0 + hrow <= 63
            const uint2 d = L.q[k0 + hrow].pad;
            const uint32_t r_w = d.y, skip = d.x & kLineMask;
            S.cur4 = ((d.x & ~kLineMask) + (uint32_t)hl) * 16u;
            S.carry = L.endc[k0 + hrow];
            // an empty CIGAR, or a promised read that starts past the window: nothing to load
            if (rw_groups_slot0(r_w) != 0u && !(rw_promised(r_w) && S.carry > W.ee)) {
                // (the head asks of the groups left only whether they end in the line at hand)
                const uint32_t left = min(rw_groups_slot0(r_w) + skip, (uint32_t)((kHeadLines + 1) * kHeadLanes));
                S.st = row_state(left, (uint32_t)(k0 + hrow), rw_2d(r_w), rw_promised(r_w));
                if ((uint32_t)hl - skip < left - skip) voff = S.cur4;
            }
        }
        return __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)voff, 0, AUX);
    };
    RowStream sa{0u, 0u, 0u}, sb = sa, sc = sa, sd = sa;
    u32x4 qa, qb, qc, qd;
    // four named buffers, one load per slot and round whether its rows are live or not: each step waits only
    // for its own load (vmcnt(3)); an idle slot's load is out of range everywhere and moves no bytes
    for (int k0 = 0; k0 < cnt; k0 += 4 * kHeadLanes) {
        qa = assign(sa, k0);
        qb = assign(sb, k0 + kHeadLanes);
        qc = assign(sc, k0 + 2 * kHeadLanes);
        qd = assign(sd, k0 + 3 * kHeadLanes);
        if (ballot64((sa.st | sb.st | sc.st | sd.st) != 0u)) {
            int line = 0;
            do {
                const bool last = ++line == kHeadLines;
                if (ballot64(sa.st != 0u)) step(qa, sa, Head{}, last);
                qa = head_issue(sa);
                if (ballot64(sb.st != 0u)) step(qb, sb, Head{}, last);
                qb = head_issue(sb);
                if (ballot64(sc.st != 0u)) step(qc, sc, Head{}, last);
                qc = head_issue(sc);
                if (ballot64(sd.st != 0u)) step(qd, sd, Head{}, last);
                qd = head_issue(sd);
            } while (ballot64((sa.st | sb.st | sc.st | sd.st) != 0u));
        }
    }

    // ---- later pieces: the reads the head has not settled, as a list of ncont entries in LDS ----
    __builtin_amdgcn_wave_barrier();
    const uint32_t endc0 = L.endc[lane];
    const uint2 own = L.q[lane].pad;  // this lane's read again: first group, row word (read before any cont_put)
    const uint32_t groups = rw_groups_slot0(own.y) & (kRowMaxGroups - 1u);
    const bool promised = rw_promised(own.y);
    // what the head took of read k: kHeadLines lines from the start of the line the read starts in
    const uint32_t head_groups = (uint32_t)(kHeadLines * kHeadLanes) - (own.x & kLineMask);
    const bool cont = groups > head_groups && !(promised && endc0 > W.ee);
    const uint64_t cmask = ballot64(cont);
    if (cmask) {
        const int ncont = (int)__popcll(cmask);
        // the i-th read to go on: on the line boundary behind the head's lines, for the row that claims it
        if (cont) {
            const uint32_t i = __builtin_amdgcn_mbcnt_hi((uint32_t)(cmask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)cmask, 0u));
            cont_put(L, i, own.x + head_groups, (own.y - head_groups) | ((uint32_t)lane << RW_SLOT), endc0);
        }
        __builtin_amdgcn_wave_barrier();

        int next = 0;  // wave-uniform: the first read of the list no row has taken yet
        // rows whose stream is idle take the next reads of the list, in row order; every one of them has a piece to load
        auto claim = [&](RowStream &S) {
            if (next >= ncont) return;
            const bool idle = S.st == 0u;
            const uint64_t need = ballot64(idle) & row_heads;
            if (need == 0ull) return;
            // idle rows below this one: the set bits of `need` in lower lanes, less this row's own head
            const int below = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
            const int k = next + below - ((idle && rl != 0) ? 1 : 0);
            next += (int)__popcll(need);
            if (idle && k < ncont) {
                uint32_t r_w;
                cont_get(L, k, S.cur4, r_w, S.carry);
                S.st = row_state(rw_groups(r_w), rw_slot(r_w), rw_2d(r_w), rw_promised(r_w));
            }
        };
        sa.st = sb.st = sc.st = sd.st = 0u;
        claim(sa);
        qa = issue(sa);
        claim(sb);
        qb = issue(sb);
        claim(sc);
        qc = issue(sc);
        claim(sd);
        qd = issue(sd);
        while (ballot64((sa.st | sb.st | sc.st | sd.st) != 0u)) {
            if (ballot64(sa.st != 0u)) {
                step(qa, sa, Later{}, false);
                claim(sa);
            }
            qa = issue(sa);
            if (ballot64(sb.st != 0u)) {
                step(qb, sb, Later{}, false);
                claim(sb);
            }
            qb = issue(sb);
            if (ballot64(sc.st != 0u)) {
                step(qc, sc, Later{}, false);
                claim(sc);
            }
            qc = issue(sc);
            if (ballot64(sd.st != 0u)) {
                step(qd, sd, Later{}, false);
                claim(sd);
            }
            qd = issue(sd);
        }
    }
    if (qcount) drain_queue(L, qcount, W, lane);
    if (ballot64((lane_err & 1u) != 0u)) status |= ST_CIGAR_OP;  // rust-htslib cigar() would panic
    if (ballot64((lane_err & 2u) != 0u)) status |= ST_RANGE;
    __builtin_amdgcn_wave_barrier();
    read_epilogue<UNPHASED>(m, valid, cnt, W, lane, L.endc[lane], status, L, val, meta);
}

// The walk of pairs [0, cnt): window-bounded when some read of the block carries the producer's promise,
// the window does not wrap and the batch's CIGAR fits one buffer descriptor; the whole walk otherwise.
template <bool UNPHASED, int AUX>
__device__ __forceinline__ void walk_pairs(const BatchView &b, const PairMeta &m, bool valid, int cnt,
                                           const Window &W, int lane, uint32_t &status, WaveLds &L, int64_t &val,
                                           uint32_t &meta) {
    const bool checked = lane < cnt && valid && ((m.misc >> 24) & RP_CHECKED) != 0u;
    const bool too_long = lane < cnt && valid && cigar_groups(m.nc & 0x0fffffffu) >= kRowMaxGroups;
    if (ballot64(checked) != 0ull && ballot64(too_long) == 0ull && W.ee >= W.se1 && b.n_cigar4 < (1ull << 28)) {
        const bool checks = ballot64(lane < cnt && valid && !checked) != 0ull;
        walk_pairs_rows<UNPHASED, AUX>(b, m, valid, cnt, W, lane, checks, status, L, val, meta);
    } else {
        walk_pairs_whole<UNPHASED, AUX>(b, m, valid, cnt, W, lane, status, L, val, meta);
    }
}

}  // namespace inq
