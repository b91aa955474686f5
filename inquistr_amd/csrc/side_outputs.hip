// side_outputs.hip — the side-output half of the C ABI in include/inquistr_hip.h: the context buffers behind what a call or a flush is
// asked for besides its rows (extras_*, ctx.h), the fetches of what they left in the context, and the side kernels' stand-alone entries.
// The launch sequence itself is capi.hip's enqueue_batch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/inquistr_hip.h"
#include "ctx.h"
#include "front_kernels.h"
#include "locus_motifs.h"
#include "read_calls.h"
#include "read_motifs.h"
#include "read_seqs.h"
#include "run_bytes.h"

using namespace inq;

namespace {

// the first n of the `offered` records (rec_size bytes each) that the last flush left in buf
int records_fetch(inq_ctx *c, const DevBuf &buf, uint64_t offered, void *out, uint64_t n, size_t rec_size) {
    if (n > offered || (n && !out)) return INQ_ERR_ARG;
    if (!n) return INQ_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(out, buf.p, (size_t)n * rec_size, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return INQ_OK;
}

// the first n records (rec_size bytes each) and the first n_bytes bytes of the runs of one kind that the last flush left in c
int kept_runs_fetch(inq_ctx *c, KeptRuns inq_ctx::*kind, void *recs, uint64_t n, size_t rec_size, uint8_t *bytes, uint64_t n_bytes) {
    if (!c) return INQ_ERR_ARG;
    const KeptRuns *const k = &(c->*kind);
    if (n > k->n_recs || n_bytes > k->n_bytes || (n && !recs) || (n_bytes && !bytes)) return INQ_ERR_ARG;
    if (!n && !n_bytes) return INQ_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (n) HIP_TRY(c, hipMemcpyAsync(recs, k->recs.p, (size_t)n * rec_size, hipMemcpyDeviceToHost, c->stream));
    if (n_bytes) HIP_TRY(c, hipMemcpyAsync(bytes, k->bytes.p, (size_t)n_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return INQ_OK;
}

// What both stand-alone motif entries take: records and packed slices as inq_read_seqs_fetch returns them, the loci's offsets into them
struct HostSlices {
    const inq_read_seq_t *recs;  // [n]
    uint64_t n;
    const uint8_t *packed;
    uint64_t seq_bytes;
    const uint64_t *kept_off;  // [n_loci + 1]
    uint64_t n_loci;
};
// ... and what goes up of them: the kernels' per-segment arrays (where each record's slice begins, and its length), which live until
// the caller has waited for the stream, and the view of the uploads
struct SlicesUp {
    std::vector<uint64_t> seg_off;
    std::vector<uint32_t> seg_len;
    KeptSlices view;
};
// An entry's first step: the last call's records are no longer offered, whatever comes of this one; false: INQ_ERR_ARG
bool slices_ok(inq_ctx *c, const HostSlices &h) {
    if (!c) return false;
    extras_reset(c);
    if ((h.n && !h.recs) || (h.seq_bytes && !h.packed) || !h.kept_off) return false;
    return h.n < (1ull << 40) && h.n_loci < 0xfffffff0ull && offsets_ok(h.kept_off, h.n_loci, h.n);
}
// the slices and `words` (n_loci motif words, or null) go up into the scratch of the flushes' sequences and motifs, which is free
// between calls
int slices_up(inq_ctx *c, const HostSlices &h, const uint64_t *words, SlicesUp *up) {
    up->seg_off.resize(h.n);
    up->seg_len.resize(h.n);
    uint64_t at = 0;
    for (uint64_t k = 0; k < h.n; ++k) up->seg_off[k] = at, up->seg_len[k] = h.recs[k].n_bases, at += run_bytes(h.recs[k]);
    HIP_TRY(c, hipSetDevice(c->device));
    const int rc = upload(c, c->stream, {{&c->rseqs.bytes, h.packed, (size_t)h.seq_bytes},
                                         {&c->rseqs.off, up->seg_off.data(), (size_t)h.n * 8},
                                         {&c->rseqs.recs, up->seg_len.data(), (size_t)h.n * 4},
                                         {&c->rcoff, h.kept_off, (size_t)(h.n_loci + 1) * 8},
                                         {&c->rmotifword, words, words ? (size_t)h.n_loci * 8 : 0}});
    if (rc != INQ_OK) return rc;
    up->view = KeptSlices{nullptr, nullptr, (const uint64_t *)c->rcoff.p, h.n_loci, (const uint8_t *)c->rseqs.bytes.p, h.seq_bytes,
                          (const uint64_t *)c->rseqs.off.p, (const uint32_t *)c->rseqs.recs.p, h.n, h.n};
    return INQ_OK;
}

// the motif kernel alone: the slices go up, a record each comes down
int motif_runs_impl(inq_ctx_t *c, const HostSlices &h, const uint64_t *motif, inq_read_motif_t *out) {
    if (!slices_ok(c, h) || (h.n && !out) || (h.n_loci && !motif)) return INQ_ERR_ARG;
    if (!h.n) return INQ_OK;
    if (!h.n_loci) {  // no record has a locus
        std::memset(out, 0, (size_t)h.n * sizeof *out);
        return INQ_OK;
    }
    SlicesUp up;
    int rc = slices_up(c, h, motif, &up);
    if (rc != INQ_OK) return rc;
    hipStream_t s = c->stream;
    if ((rc = ensure(c, c->rmotifs, (size_t)h.n * sizeof(inq_read_motif_t))) != INQ_OK) return rc;
    launch_read_motifs(ReadMotifArgs{up.view, (const uint64_t *)c->rmotifword.p, (inq_read_motif_t *)c->rmotifs.p}, c->grid_side, s);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out, c->rmotifs.p, (size_t)h.n * sizeof(inq_read_motif_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));  // (the uploads' sources live until here)
    purge_retired(c);
    return INQ_OK;
}

// the locus motif kernel alone: the same slices go up, a record per locus and the words come down
int locus_motifs_find_impl(inq_ctx_t *c, const HostSlices &h, const uint64_t *given, inq_locus_motif_t *found, uint64_t *use) {
    if (!slices_ok(c, h) || (h.n_loci && !found)) return INQ_ERR_ARG;
    if (!h.n_loci) return INQ_OK;
    SlicesUp up;
    int rc = slices_up(c, h, given, &up);
    if (rc != INQ_OK) return rc;
    hipStream_t s = c->stream;
    if ((rc = ensure(c, c->rlocusmotif, (size_t)h.n_loci * sizeof(inq_locus_motif_t))) != INQ_OK) return rc;
    if (use && (rc = ensure(c, c->rmotifuse, (size_t)h.n_loci * 8)) != INQ_OK) return rc;
    launch_locus_motifs(LocusMotifArgs{up.view, given ? (const uint64_t *)c->rmotifword.p : nullptr, (inq_locus_motif_t *)c->rlocusmotif.p,
                                       use ? (uint64_t *)c->rmotifuse.p : nullptr}, c->grid_side, s);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(found, c->rlocusmotif.p, (size_t)h.n_loci * sizeof(inq_locus_motif_t), hipMemcpyDeviceToHost, s));
    if (use) HIP_TRY(c, hipMemcpyAsync(use, c->rmotifuse.p, (size_t)h.n_loci * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));  // (the uploads' sources live until here)
    purge_retired(c);
    return INQ_OK;
}

// the window walk alone: the batch goes up as a call's does, two arrays come down
int seq_windows_impl(inq_ctx_t *c, const inq_batch_t *b, const uint32_t *l_seq, uint32_t *q_beg, uint32_t *n_bases) {
    if (!c || !b) return INQ_ERR_ARG;
    extras_reset(c);
    if (b->n_loci && (!b->locus_pair_off || !b->locus_start || !b->locus_end)) return INQ_ERR_ARG;
    if (b->n_pairs && (!b->pair_read || !b->reads || !b->n_reads || !q_beg || !n_bases)) return INQ_ERR_ARG;
    if ((b->n_cigar_words && !b->cigar) || b->n_cigar_words % 4 != 0 || b->reserved != 0) return INQ_ERR_ARG;
    if ((!b->n_loci && b->n_pairs) || b->n_loci >= 0xfffffff0ull || b->n_pairs >= (1ull << 40)) return INQ_ERR_ARG;
    if (b->n_loci && (b->locus_pair_off[0] != 0 || b->locus_pair_off[b->n_loci] != b->n_pairs || !offsets_ok(b->locus_pair_off, b->n_loci, b->n_pairs)))
        return INQ_ERR_ARG;
    if (!b->n_pairs) return INQ_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    int rc = upload(c, s, {{&c->cigar, b->cigar, (size_t)b->n_cigar_words * 4},
                           {&c->reads, b->reads, (size_t)b->n_reads * sizeof(inq_read_t)},
                           {&c->pair_read, b->pair_read, (size_t)b->n_pairs * 4},
                           {&c->off, b->locus_pair_off, (size_t)(b->n_loci + 1) * 8},
                           {&c->lstart, b->locus_start, (size_t)b->n_loci * 4},
                           {&c->lend, b->locus_end, (size_t)b->n_loci * 4},
                           {&c->rseqs.off, l_seq, l_seq ? (size_t)b->n_reads * 4 : 0}});  // (scratch of the flushes' sequences, free between calls)
    if (rc != INQ_OK) return rc;
    if ((rc = ensure(c, c->rseqs.recs, (size_t)b->n_pairs * 8)) != INQ_OK) return rc;  // q_beg[n_pairs], n_bases[n_pairs]
    uint32_t *const d_qbeg = (uint32_t *)c->rseqs.recs.p, *const d_len = d_qbeg + b->n_pairs;
    SeqWindowArgs a{(const uint4 *)c->cigar.p, b->n_cigar_words / 4, (const uint4 *)c->reads.p, b->n_reads, (const uint32_t *)c->pair_read.p,
                    (const uint64_t *)c->off.p, (const uint32_t *)c->lstart.p, (const uint32_t *)c->lend.p, b->n_loci, b->n_pairs, SeqLenSource{},
                    d_qbeg, d_len};
    if (l_seq) a.len.l_seq = (const uint32_t *)c->rseqs.off.p;
    launch_seq_window(a, c->grid_side, s);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(q_beg, d_qbeg, (size_t)b->n_pairs * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(n_bases, d_len, (size_t)b->n_pairs * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    purge_retired(c);
    return INQ_OK;
}

}  // namespace

extern "C" {

uint32_t inq_read_call_tile(void) { return kReadCallTile; }
uint32_t inq_read_name_tile(void) { return kReadNameTile; }
uint32_t inq_seq_window_tile(void) { return kSeqWindowTile; }
uint32_t inq_read_motif_tile(void) { return kReadMotifTile; }

int inq_read_calls_fetch(inq_ctx_t *c, inq_read_call_t *out, uint64_t n) {
    return guarded([&] { return c ? records_fetch(c, c->rckept, c->read_calls_total, out, n, sizeof *out) : INQ_ERR_ARG; });
}
int inq_read_motifs_fetch(inq_ctx_t *c, inq_read_motif_t *recs, uint64_t n) {
    return guarded([&] { return c ? records_fetch(c, c->rmotifs, c->read_motifs_total, recs, n, sizeof *recs) : INQ_ERR_ARG; });
}
int inq_read_origins_fetch(inq_ctx_t *c, inq_read_origin_t *origins, uint64_t n, uint8_t *names, uint64_t name_bytes) {
    return guarded([&] { return kept_runs_fetch(c, &inq_ctx::rnames, origins, n, sizeof *origins, names, name_bytes); });
}
int inq_read_seqs_fetch(inq_ctx_t *c, inq_read_seq_t *seqs, uint64_t n, uint8_t *packed, uint64_t seq_bytes) {
    return guarded([&] { return kept_runs_fetch(c, &inq_ctx::rseqs, seqs, n, sizeof *seqs, packed, seq_bytes); });
}

int inq_motif_runs(inq_ctx_t *c, const inq_read_seq_t *recs, uint64_t n, const uint8_t *packed, uint64_t seq_bytes, const uint64_t *kept_off,
                   const uint64_t *motif, uint64_t n_loci, inq_read_motif_t *out) {
    return guarded([&] { return motif_runs_impl(c, HostSlices{recs, n, packed, seq_bytes, kept_off, n_loci}, motif, out); });
}
int inq_locus_motifs_find(inq_ctx_t *c, const inq_read_seq_t *recs, uint64_t n, const uint8_t *packed, uint64_t seq_bytes, const uint64_t *kept_off,
                          uint64_t n_loci, const uint64_t *given, inq_locus_motif_t *found, uint64_t *use) {
    return guarded([&] { return locus_motifs_find_impl(c, HostSlices{recs, n, packed, seq_bytes, kept_off, n_loci}, given, found, use); });
}
int inq_seq_windows(inq_ctx_t *c, const inq_batch_t *b, const uint32_t *l_seq, uint32_t *q_beg, uint32_t *n_bases) {
    return guarded([&] { return seq_windows_impl(c, b, l_seq, q_beg, n_bases); });
}

}  // extern "C"

int inq::extras_prepare(inq_ctx *c, uint64_t n_loci, uint64_t n_pairs, const HostExtras &h, LocusExtras *d) {
    int rc;
    if (h.flags && (rc = ensure(c, c->lflags, (size_t)n_loci)) != INQ_OK) return rc;
    if (h.per_pair() && (rc = ensure(c, c->pcall, (size_t)n_pairs * 8)) != INQ_OK) return rc;
    if (h.per_pair() && (rc = ensure(c, c->pbits, (size_t)n_pairs)) != INQ_OK) return rc;
    if (h.evidence && (rc = ensure(c, c->levidence, (size_t)n_loci * sizeof(inq_locus_evidence_t))) != INQ_OK) return rc;
    if (h.kept_off && (rc = ensure(c, c->rcoff, (size_t)(n_loci + 1) * 8)) != INQ_OK) return rc;
    if (h.kept_off && (rc = ensure(c, c->rckept, (size_t)n_pairs * sizeof(inq_read_call_t))) != INQ_OK) return rc;
    d->flags = h.flags ? (uint8_t *)c->lflags.p : nullptr;
    d->evidence = h.evidence ? (inq_locus_evidence_t *)c->levidence.p : nullptr;
    d->kept_off = h.kept_off ? (uint64_t *)c->rcoff.p : nullptr;
    d->kept = h.kept_off ? (inq_read_call_t *)c->rckept.p : nullptr;
    // a kind's records and the scan of their byte lengths (the batch's own names and slices, LocusExtras::name_off, seq_qbeg / seq_len,
    // are the caller's to set: only a deferred batch has them)
    auto runs = [&](KeptRuns &k, auto &out) -> int {
        if ((rc = ensure(c, k.recs, (size_t)n_pairs * sizeof *out.recs)) != INQ_OK) return rc;
        if ((rc = ensure(c, k.off, (size_t)(n_pairs + 1 + scan_tmp_words(std::max<uint64_t>(n_pairs, 1))) * 8)) != INQ_OK) return rc;
        out.recs = (decltype(out.recs))k.recs.p;
        out.off = (uint64_t *)k.off.p;
        return INQ_OK;
    };
    if (h.name_bytes) {
        if (!h.kept_off) return INQ_ERR_ARG;
        if ((rc = runs(c->rnames, d->names)) != INQ_OK) return rc;
    }
    if (h.seq_bytes) {
        if (!h.kept_off || !h.name_bytes) return INQ_ERR_ARG;
        if ((rc = ensure(c, c->rkeptpair, (size_t)n_pairs * 8)) != INQ_OK) return rc;
        if ((rc = runs(c->rseqs, d->seqs)) != INQ_OK) return rc;
        d->kept_pair = (uint64_t *)c->rkeptpair.p;
    }
    if (h.motif_runs()) {
        if (!h.seq_bytes) return INQ_ERR_ARG;
        if ((rc = ensure(c, c->rmotifs, (size_t)n_pairs * sizeof(inq_read_motif_t))) != INQ_OK) return rc;
        if ((rc = ensure(c, c->rmotifword, (size_t)n_loci * 8)) != INQ_OK) return rc;
        d->motifs = (inq_read_motif_t *)c->rmotifs.p;
        d->motif_word = (const uint64_t *)c->rmotifword.p;
    }
    if (h.found) {  // the motif kernel reads the words the search wrote, the given ones among them
        if ((rc = ensure(c, c->rlocusmotif, (size_t)n_loci * sizeof(inq_locus_motif_t))) != INQ_OK) return rc;
        if ((rc = ensure(c, c->rmotifuse, (size_t)n_loci * 8)) != INQ_OK) return rc;
        d->locus_found = (inq_locus_motif_t *)c->rlocusmotif.p;
        d->motif_given = h.motif ? (const uint64_t *)c->rmotifword.p : nullptr;
        d->motif_use = (uint64_t *)c->rmotifuse.p;
        d->motif_word = d->motif_use;
    }
    return INQ_OK;
}

int inq::extras_download(inq_ctx *c, uint64_t n_loci, const HostExtras &h, const LocusExtras &d, uint8_t *flags_dst, hipStream_t s) {
    if (h.flags) HIP_TRY(c, hipMemcpyAsync(flags_dst, d.flags, (size_t)n_loci, hipMemcpyDeviceToHost, s));
    if (h.evidence) HIP_TRY(c, hipMemcpyAsync(h.evidence, d.evidence, (size_t)n_loci * sizeof(inq_locus_evidence_t), hipMemcpyDeviceToHost, s));
    if (h.kept_off) HIP_TRY(c, hipMemcpyAsync(h.kept_off, d.kept_off, (size_t)(n_loci + 1) * 8, hipMemcpyDeviceToHost, s));
    if (h.found) HIP_TRY(c, hipMemcpyAsync(h.found, d.locus_found, (size_t)n_loci * sizeof(inq_locus_motif_t), hipMemcpyDeviceToHost, s));
    return INQ_OK;
}

int inq::extras_names(inq_ctx *c, uint64_t n_pairs, uint64_t n_kept, const HostExtras &h, const LocusExtras &d, const RunSource &names,
                      const RunSource &seqs, hipStream_t s) {
    // per kind: where its byte total goes (null: not asked for), the scan it sits behind, where the runs come from and where they go
    const struct {
        uint64_t *total;
        const uint64_t *off;
        const RunSource &src;
        DevBuf &dst;
    } kinds[] = {{h.name_bytes, d.names.off, names, c->rnames.bytes}, {h.seq_bytes, d.seqs.off, seqs, c->rseqs.bytes}};
    for (auto &k : kinds)
        if (k.total) *k.total = 0;
    if (!h.name_bytes || !n_pairs || !n_kept) return INQ_OK;
    // (each scan's total sits behind its last element; nothing else is in flight on s: plain 8-byte copies, one wait for all)
    for (auto &k : kinds)
        if (k.total) HIP_TRY(c, hipMemcpyAsync(k.total, k.off + n_pairs, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    bool any = false;
    for (auto &k : kinds) {
        if (!k.total || !*k.total) continue;
        const int rc = ensure(c, k.dst, (size_t)*k.total);
        if (rc != INQ_OK) return rc;
        launch_name_copy(NameCopyArgs{k.src.bytes, k.src.n_bytes, k.src.off, k.src.n, 0, k.src.by_pair ? nullptr : d.kept, (uint8_t *)k.dst.p,
                                      *k.total, k.off, std::min(n_kept, n_pairs), k.src.by_pair ? d.kept_pair : nullptr}, c->grid_side, s);
        any = true;
    }
    if (!any) return INQ_OK;
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(s));
    return INQ_OK;
}

void inq::extras_finish(inq_ctx *c, uint64_t n_loci, uint64_t n_pairs, const HostExtras &h, uint32_t err) {
    if (!h.kept_off) return;
    if (!n_loci) h.kept_off[0] = 0;  // (nothing was launched: no list, no record)
    if (err == 0) c->read_calls_total = std::min<uint64_t>(h.kept_off[n_loci], n_pairs);
    if (h.name_bytes && err == 0) c->rnames.n_recs = c->read_calls_total, c->rnames.n_bytes = *h.name_bytes;
    if (h.seq_bytes && err == 0) c->rseqs.n_recs = c->read_calls_total, c->rseqs.n_bytes = *h.seq_bytes;
    if (h.motif_runs() && err == 0) c->read_motifs_total = c->read_calls_total;
}
