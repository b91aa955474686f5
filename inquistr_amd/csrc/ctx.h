// ctx.h — the library context behind inq_ctx_t, shared by the translation units that implement the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <array>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <mutex>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/inquistr_hip.h"
#include "kernels.h"

namespace inq {

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

// e0 in front of a launch sequence, e1 behind its first kernel, e2 behind its last.  one_kernel: nothing was launched behind e1, so
// e2 was not recorded and e1 ends the sequence too (an event record with nothing in front of it still costs the stream ~5 us)
struct EvTriple {
    hipEvent_t e0, e1, e2;
    bool one_kernel = false;
};

// The byte runs behind the kept records of a flush, one kind each (the names: read_names.hip; the packed bases: read_seqs.hip): one
// 8-byte record per kept record, the exclusive scan of the records' byte lengths with its tile totals behind it, the runs back to back
// in the records' order.  They stay until the context's next call (inq_read_origins_fetch, inq_read_seqs_fetch).  Allocated by flushes
// that ask for the kind only
struct KeptRuns {
    DevBuf recs, off, bytes;
    uint64_t n_recs = 0, n_bytes = 0;  // records and bytes the last flush offers (0: it had none of this kind)
    auto bufs() { return std::array{&recs, &off, &bytes}; }
};

struct SpanState;  // device front end (span.hip)

}  // namespace inq

struct inq_ctx {
    int device = -1;
    hipStream_t stream = nullptr;
    std::string backend, last_err;
    inq::DevStatus *d_status = nullptr;
    inq::DevStatus *h_status = nullptr;  // pinned mirror for the host-buffer entry
    inq::DevBuf worklist, sval, smeta, deep;
    // staging for the host-buffer entry
    inq::DevBuf cigar, reads, pair_read, off, lstart, lend, p1, p2, pcall, pbits, lflags;
    // per-locus evidence (evidence.hip): the records of a host-buffer call or a flush, the slice list of the deep loci; pcall / pbits
    // also hold the per-pair outputs of a call with evidence whose caller did not ask for them.  Allocated by calls with evidence only
    inq::DevBuf levidence, evwork;
    // the per-read Calls (read_calls.hip): the tile arrays of the compaction; kept_off and the records of a host-buffer call or a flush,
    // which stay until the context's next call (inq_read_calls_fetch).  Allocated by calls with the lists only
    inq::DevBuf rctiles, rcoff, rckept;
    uint64_t read_calls_total = 0;  // records of the last host-buffer call or flush (0: it had no lists)
    // who those records are and the bases behind them (inq_call_flush_origins, inq_call_flush_seqs): the records of rnames are
    // inq_read_origin_t, those of rseqs inq_read_seq_t; rkeptpair: the pair each record came from, which only the bases are indexed by
    inq::KeptRuns rnames, rseqs;
    inq::DevBuf rkeptpair;
    // the motif runs of those bases (inq_call_flush_motifs, read_motifs.hip): one inq_read_motif_t per kept record, which stay until the
    // context's next call (inq_read_motifs_fetch), and the loci's motif words.  Allocated by flushes with motifs only
    inq::DevBuf rmotifs, rmotifword;
    uint64_t read_motifs_total = 0;  // records of the last flush with motifs (0: it had none)
    // the motif each locus's reads repeat (inq_call_flush_locus_motifs, locus_motifs.hip): one inq_locus_motif_t per locus, and the word
    // the motif kernel measures each locus with (the given one, else the found one).  Allocated by flushes that look for motifs only
    inq::DevBuf rlocusmotif, rmotifuse;
    inq::DevBuf ovalues, olen, oflags, okeep, otrans;  // inq_outlier_rows
    inq::DevBuf avalues, ay, acov, atcoef, arows;      // inq_assoc_rows: one tile of the matrix and of its rows, the shared columns
    inq::DevBuf aminmu, afirth;                        // inq_assoc_rows_firth: a tile's smallest min(mu, 1 - mu) per row, its Firth rows
    // every DevBuf above, for inq_ctx_destroy (DevBuf frees nothing itself): a member missing here leaks
    auto bufs() {
        std::vector<inq::DevBuf *> all{&worklist, &sval, &smeta, &deep, &cigar, &reads, &pair_read, &off, &lstart, &lend, &p1, &p2, &pcall, &pbits,
                                       &lflags, &levidence, &evwork, &rctiles, &rcoff, &rckept, &rkeptpair, &rmotifs, &rmotifword, &rlocusmotif, &rmotifuse, &ovalues, &olen, &oflags, &okeep, &otrans,
                                       &avalues, &ay, &acov, &atcoef, &arows, &aminmu, &afirth};
        for (inq::KeptRuns *k : {&rnames, &rseqs})
            for (inq::DevBuf *b : k->bufs()) all.push_back(b);
        return all;
    }
    uint32_t n_cus = 0;        // compute units of the device
    uint32_t grid_tail = 256;  // workgroups of the persistent locus_call_tail: they meet at grid barriers, so never more than n_cus
    uint32_t grid_medium = 4096;  // (8 192: + 3 us for the launch that finds the lists empty, 0 - 4 % quicker where they are full)
    uint32_t grid_side = 0;       // workgroups at most of a side kernel's launch (side_grid); 0: each launcher's own cap
    uint32_t max_reads_hint = 0;  // 0 = unknown; else the caller's bound on reads per locus
    uint32_t call_hint = 0;       // set by the host-buffer entry, which sees the offsets, for its own launch
    int nt_loads = -1;  // -1 auto: non-temporal when no read is shared between loci
    bool timing = false;
    bool verify_crc = true;  // device front end: check inflated blocks against their CRC32
    // workgroup inflate: the counting passes leave the symbols behind for the commit (option "inflate_tokens").  Round 3 switched it on
    // for match-heavy spans (+3 ... 4 % on CIGAR-only records); the counters then showed what it moves: 32 KB of scratch per block
    // written in EVERY counting pass, 7.5 GB of HBM traffic for 1.79 GB of algorithmic bytes on the 501 MB file (profiles/r03_front/).
    // With the inflate of span k + 1 now running beside the scan / gather / locus kernels of span k that traffic is no longer free:
    // off unless asked for (1 = on, -1 = on where the sampled block headers say match-heavy, 0 = off)
    int inflate_tokens = 0;
    int inflate_lit_pairs = -1;  // workgroup inflate's symbol loop: 1 = a second literal from the same peek, 0 = not, -1 = by the data (deflate_probe.h)
    // a staged span (inq_span_stage_begin) is inflated right behind its upload, on a stream of its own: the inflate of span k + 1 runs
    // beside span k's record scan, gather and join.  A staging slot then holds an inflated buffer of its own.  Round 3 left this off
    // for "+0.3 s for a one-file process"; round 4 found that figure to be the driver's teardown of the PREVIOUS process in the
    // timing loop, not the allocations (hipMalloc: 10 - 200 us whatever the size): on
    int inflate_ahead = 1;
    int outlier_tile = 1;   // z-score of rows of <= 256 values through an LDS tile (0: the transposed-copy kernel for every width)
    uint64_t assoc_tile_rows = 0;  // rows inq_assoc_rows uploads and fits per launch (0: as many as fill 256 MB)
    uint64_t assoc_firth_mu_ppb = 1000;  // inq_assoc_rows_firth, FALLBACK: min(mu, 1 - mu) below this many 1e-9 selects a row
    int blocking_sync = 0;  // waits give the core back (hipDeviceScheduleBlockingSync, blocking events): for a caller short of cores
    // the gather's stores bypass the caches (bam_scan.hip): the batch it builds is read by a later launch, not by this one; the locus
    // kernels behind it run at 5.4 - 6.2 instead of 4.9 - 5.3 TB/s of algorithmic bytes (profiles/r04_results/locus_kernels_in_the_cli.txt)
    bool gather_nt = true;
    uint64_t batch_loci_hint = 0;  // inq_call_span_deferred: loci the caller lets a batch collect before it flushes (0 = no word)
    // Buffers that were outgrown.  Growing one used to mean hipDeviceSynchronize + hipFree + hipMalloc on the spot; both calls wait for
    // EVERY stream of the device - in the span loop that is the 5 ms upload of the next span on the copy stream, ten times per file
    // (profiles/r04_results/span_loop_growth_stalls.txt).  hipMalloc alone costs 10 - 200 us whatever the size (tools/alloc_probe.hip),
    // so the old buffer is parked here - earlier launches may still read it - and given back at a point where the device is idle
    // anyway (the end of a flush / of a host-buffer call, the destruction of the ctx) or when more than 16 GB wait.
    std::mutex retired_mu;  // the uploader thread (inq_span_stage) grows its slots while the caller grows the scan buffers
    std::vector<std::pair<void *, size_t>> retired;
    size_t retired_bytes = 0;
    size_t retired_limit = 16ull << 30;  // option "retired_limit_mb"
    // an allocation that fails for lack of memory gives the parked buffers back and tries again (capi.hip device_alloc)
    uint32_t test_fail_allocs = 0;  // option "test_fail_allocs": the next N allocations fail at their first attempt
    uint64_t alloc_retries = 0;     // how often that second attempt was needed (inq_ctx_alloc_retries)
    std::vector<inq::EvTriple> ev_pool;
    size_t ev_used = 0;
    inq::SpanState *span = nullptr;  // created on first use by the device front end
};

#define HIP_TRY(ctx, expr)                                                                     \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) {                                                                \
            (ctx)->last_err = std::string(#expr) + ": " + hipGetErrorString(_e);               \
            return _e == hipErrorOutOfMemory ? INQ_ERR_NOMEM : INQ_ERR_HIP;                    \
        }                                                                                      \
    } while (0)

namespace inq {
// The one place the library could read an experiment's switch from the environment - and it does only when built with
// -DINQ_DEBUG_ENV (make DEBUG_ENV=1).  What a host can set is inq_ctx_set_option / inq_default_option, nothing else; INQ_TIMING
// (stage clocks on stderr) is the only variable the shipped library looks at.
#ifdef INQ_DEBUG_ENV
inline const char *debug_env(const char *name) { return std::getenv(name); }
#else
inline const char *debug_env(const char *) { return nullptr; }
#endif
// every ABI entry that can throw runs its body through this: nothing may unwind across the C ABI
template <class F> int guarded(F &&body) {
    try {
        return body();
    } catch (const std::bad_alloc &) {
        return INQ_ERR_NOMEM;
    } catch (...) {
        return INQ_ERR_HIP;
    }
}
// INQ_TIMING=2: host clocks on stderr, each line behind `prefix` ("[inq ctx]", "[inq span host]", "[inq stage host] slot N")
struct HostClock {
    using clk = std::chrono::steady_clock;
    const char *prefix;
    bool on;
    clk::time_point t0 = clk::now(), last = t0;
    explicit HostClock(const char *prefix_) : prefix(prefix_) {
        const char *e = std::getenv("INQ_TIMING");
        on = e && e[0] == '2';
    }
    static double ms(clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }
    void lap(const char *what) {  // since the last lap
        if (!on) return;
        const auto now = clk::now();
        std::fprintf(stderr, "%s %-34s %7.2f ms\n", prefix, what, ms(last, now));
        last = now;
    }
    void at(const char *what) const {  // since the start
        if (on) std::fprintf(stderr, "%s %-28s at %.2f ms\n", prefix, what, ms(t0, clk::now()));
    }
};
inline bool locus_ok(uint32_t start, uint32_t end) { return start >= 10 && end >= start; }  // else INQ_ERR_LOCUS
// grows b to at least `bytes` (with headroom); the old buffer is retired, not freed: no synchronisation, contents NOT kept
int ensure(inq_ctx *c, DevBuf &b, size_t bytes);
int device_alloc(inq_ctx *c, void **out, size_t want, size_t exact, size_t *got);
void retire(inq_ctx *c, void *p, size_t bytes);
void purge_retired(inq_ctx *c);  // hipFree of everything retired (waits for the device: call where it is idle)
// host arrays on their way into context buffers: each buffer is grown to its array (ensure), then the copy is enqueued on s (none for
// 0 bytes).  The arrays live until the caller has waited for s
struct Upload {
    DevBuf *d;
    const void *h;
    size_t bytes;
};
int upload(inq_ctx *c, hipStream_t s, std::initializer_list<Upload> ups);
// off[0 .. n] ascend and end at or in front of total (else INQ_ERR_ARG: the kernels' searches and grids assume it)
inline bool offsets_ok(const uint64_t *off, uint64_t n, uint64_t total) {
    for (uint64_t j = 0; j < n; ++j)
        if (off[j] > off[j + 1]) return false;
    return off[n] <= total;
}
// The per-locus side outputs of a call, as the launch sequence takes them: all DEVICE pointers.  Null = not asked for: nothing is added
// to the launch sequence and nothing is allocated.  A further per-locus output is one more member here and in HostExtras.
struct LocusExtras {
    uint8_t *flags = nullptr;                  // [n_loci] INQ_LOCUS_TIE
    inq_locus_evidence_t *evidence = nullptr;  // [n_loci]
    uint64_t *kept_off = nullptr;              // [n_loci + 1] the per-read Calls: offsets ...
    inq_read_call_t *kept = nullptr;           // [n_pairs] ... and records; both or neither
    // the byte runs behind those records (need kept), per kind: one record per kept record, and off[n_pairs + 1 + scan_tmp_words(n_pairs)],
    // the exclusive scan of the records' run_bytes() (off[n_pairs] = the total) with the scan's tile totals behind it
    template <class Rec> struct Runs {
        Rec *recs = nullptr;
        uint64_t *off = nullptr;
    };
    Runs<inq_read_origin_t> names;       // who the records are; name_off: the batch's names
    const uint64_t *name_off = nullptr;  // [n_reads + 1]
    // the bases behind them; kept_pair[n_pairs]: the pair each record came from, written by the compaction's scatter; seq_qbeg / seq_len:
    // the batch's slices, per pair
    Runs<inq_read_seq_t> seqs;
    uint64_t *kept_pair = nullptr;
    const uint32_t *seq_qbeg = nullptr, *seq_len = nullptr;  // [n_pairs]
    // the motif runs of those bases (needs seqs): a record per kept record out of motif_word[n_loci] and the batch's own per-pair
    // slices, seq_len[p] bases packed from byte seq_off[p] of seq_bytes on.  The launch sequence hands kept_pair, kept_off and these
    // slices to both motif kernels as one KeptSlices (kept_view.h); kept_pair and kept_off are written through here first, so the
    // members stay what the compaction takes
    inq_read_motif_t *motifs = nullptr;
    const uint64_t *motif_word = nullptr;
    const uint8_t *seq_bytes = nullptr;
    uint64_t seq_n_bytes = 0;
    const uint64_t *seq_off = nullptr;  // [n_pairs]
    // the motif each locus's reads repeat (needs motifs): a record per locus out of the same slices, in front of the motif kernel, which
    // then reads motif_word = what this wrote: motif_given[j] where that names a motif (null: none does), else the found word
    inq_locus_motif_t *locus_found = nullptr;
    const uint64_t *motif_given = nullptr;
    uint64_t *motif_use = nullptr;
};
// Where a flush takes the runs of one kind from, the deferred batch's (SpanState::Acc hands them over): n runs back to back in `bytes`,
// run i at off[i].  by_pair: a kept record's run is that of the pair it came from (the bases), else that of its read (the names)
struct RunSource {
    const uint8_t *bytes;
    uint64_t n_bytes;
    const uint64_t *off;  // [n + 1]
    uint64_t n;
    bool by_pair;
};
// ... and as a host-buffer call or a flush takes them: HOST pointers, [n_loci] / [n_loci] / [n_loci + 1] in the call's locus order, each
// may be null.  The records behind kept_off stay in context scratch (inq_read_calls_fetch).
struct HostExtras {
    uint8_t *flags = nullptr;
    inq_locus_evidence_t *evidence = nullptr;
    uint64_t *kept_off = nullptr;
    uint64_t *name_bytes = nullptr;  // a flush with origins (needs kept_off): receives the bytes of the kept records' names
    uint64_t *seq_bytes = nullptr;   // a flush with sequences (needs kept_off): receives the bytes of the kept records' packed slices
    const uint64_t *motif = nullptr;  // a flush with motifs (needs seq_bytes): the loci's motif words, read, not written
    inq_locus_motif_t *found = nullptr;  // a flush that looks for the loci's motifs (needs seq_bytes; motif may be null): a record per locus
    bool motif_runs() const { return motif || found; }  // the flush produces a read-motif record per kept record
    // the evidence is counted and the lists are compacted from the per-pair outputs: the call keeps those (pcall / pbits) also when
    // its caller did not ask for them
    bool per_pair() const { return evidence || kept_off; }
};
// The three steps of a host-buffer call or a flush around its launch sequence.  First of all extras_reset: the records of the call
// before are no longer offered, however this one ends.
inline void extras_reset(inq_ctx *c) {
    c->read_calls_total = c->read_motifs_total = 0;
    for (KeptRuns *k : {&c->rnames, &c->rseqs}) k->n_recs = k->n_bytes = 0;
}
// the context buffers behind what h asks for (and pcall / pbits where h.per_pair()), as device pointers
int extras_prepare(inq_ctx *c, uint64_t n_loci, uint64_t n_pairs, const HostExtras &h, LocusExtras *d);
// enqueues the copies down on s; the flags go to flags_dst (the caller's array, or page-locked staging on their way there)
int extras_download(inq_ctx *c, uint64_t n_loci, const HostExtras &h, const LocusExtras &d, uint8_t *flags_dst, hipStream_t s);
// a flush with origins, after its synchronisation (n_kept = kept_off[n_loci] is known then): the byte totals of the kinds asked for
// come down with one wait (*h.name_bytes, *h.seq_bytes), the context's byte buffers are sized from them, one copy launch per kind runs
// out of the batch's runs (names, seqs) and they are waited for once.  Without origins, pairs or records: nothing
int extras_names(inq_ctx *c, uint64_t n_pairs, uint64_t n_kept, const HostExtras &h, const LocusExtras &d, const RunSource &names,
                 const RunSource &seqs, hipStream_t s);
// after the call's synchronisation, or at once for a call without loci: how many records inq_read_calls_fetch offers.  err: the
// kernels' status word - after a domain error the lists are unspecified and none is offered, whatever the offsets say
void extras_finish(inq_ctx *c, uint64_t n_loci, uint64_t n_pairs, const HostExtras &h, uint32_t err);
// enqueue-only launch sequence of the locus kernels over a device-resident batch
int call_batch_device_impl(inq_ctx *c, const inq_batch_t *b, inq_result_t *r, void *hip_stream, const LocusExtras &x = LocusExtras());
int status_to_code(uint32_t st);
// The kernels' status travels with the results: enqueues DevStatus -> dst (page-locked), then clears err and ties on the same stream,
// i.e. before the next call's kernels (the work-list counters stay).  No synchronisation: dst is valid once the caller has waited for s.
int status_readback(inq_ctx *c, DevStatus *dst, hipStream_t s);
// a batch whose arrays are on the device, with the rows (and the optional per-pair outputs) it is called into
struct DevBatch {
    inq_batch_t b;
    inq_result_t r;
};
DevBatch device_batch(const void *cigar, const void *reads, const void *pair_read, const void *off, const void *lstart, const void *lend,
                      uint64_t n_reads, uint64_t n_cigar_words, uint64_t n_pairs, uint64_t n_loci, uint32_t minlen, uint32_t support,
                      uint32_t unphased, void *p1, void *p2, void *pair_call = nullptr, void *pair_bits = nullptr);
void span_state_destroy(SpanState *s);
int span_state_init(inq_ctx *c);       // device front end state, the part staging needs (streams, slots); called by inq_ctx_create
int span_state_init_rest(inq_ctx *c);  // ... and the part the calls need
void preload_locus(hipStream_t s);
void preload_inflate(hipStream_t s);
void preload_scan(hipStream_t s);
double span_last_inflate_ms(SpanState *s);  // kernel time of the last inflate launch, < 0 if none
}  // namespace inq
