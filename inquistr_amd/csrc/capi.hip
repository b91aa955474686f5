// capi.hip — implementation of the C ABI in include/inquistr_hip.h on top of kernels.hip: the context's life cycle and options, the
// launch sequence of a call and the host-buffer call.  The side outputs' buffers, fetches and stand-alone entries: side_outputs.hip.
// HIP only: there is no CPU fallback; without a gfx950 device every entry fails loudly.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/inquistr_hip.h"
#include "cigar_walk.h"
#include "ctx.h"
#include "evidence.h"
#include "front_kernels.h"
#include "kernels.h"
#include "locus_motifs.h"
#include "read_calls.h"
#include "read_motifs.h"
#include "read_seqs.h"

using namespace inq;

namespace inq {

void retire(inq_ctx *c, void *p, size_t bytes) {
    if (!p) return;
    std::lock_guard<std::mutex> g(c->retired_mu);
    c->retired.emplace_back(p, bytes);
    c->retired_bytes += bytes;
}

void purge_retired(inq_ctx *c) {
    std::vector<std::pair<void *, size_t>> gone;
    {
        std::lock_guard<std::mutex> g(c->retired_mu);
        gone.swap(c->retired);
        c->retired_bytes = 0;
    }
    for (auto &e : gone) (void)hipFree(e.first);  // hipFree waits for the device: work that still reads the buffer ends first
}

// hipMalloc that gives the parked buffers back before it gives up: retired buffers (ctx.h) are memory the context could free at any
// moment, so "out of memory" with some of them waiting is not yet out of memory.  `exact` (< want, or 0): what the caller really
// needs, tried last without the headroom.  ("test_fail_allocs" = N makes the next N first attempts fail: the retry's test seam.)
int device_alloc(inq_ctx *c, void **out, size_t want, size_t exact, size_t *got) {
    *out = nullptr;
    *got = want;
    hipError_t e = hipSuccess;
    if (c->test_fail_allocs > 0) {
        --c->test_fail_allocs;
        ++c->alloc_retries;
        e = hipErrorOutOfMemory;
    } else {
        e = hipMalloc(out, want);
    }
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();  // clear the sticky error
        purge_retired(c);         // waits for the device: whatever still read those buffers is through
        ++c->alloc_retries;
        e = hipMalloc(out, want);
        if (e == hipErrorOutOfMemory && exact && exact < want) {
            (void)hipGetLastError();
            e = hipMalloc(out, exact);
            *got = exact;
        }
    }
    if (e != hipSuccess) {
        *out = nullptr;
        c->last_err = std::string("hipMalloc: ") + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? INQ_ERR_NOMEM : INQ_ERR_HIP;
    }
    return INQ_OK;
}

int ensure(inq_ctx *c, DevBuf &b, size_t bytes) {
    if (bytes <= b.cap && b.p) return INQ_OK;
    if (b.p) {
        // earlier launches (possibly on the caller's stream) may still use the old buffer: it is parked, not freed (ctx.h)
        retire(c, b.p, b.cap);
        b.p = nullptr;
        b.cap = 0;
        bool too_much;
        {
            std::lock_guard<std::mutex> g(c->retired_mu);
            too_much = c->retired_bytes > c->retired_limit;
        }
        if (too_much) purge_retired(c);
    }
    // grow with headroom: batches of a sweep vary in size, reallocating for each new maximum would put a malloc in front of most
    // calls.  Large buffers get little of it: device memory a process holds is wiped by the driver when the process leaves, at
    // ~20 GB/s, and while that goes on the NEXT process's hipInit and hipMalloc wait (0.1 -> 0.3 s of start-up, 50 ms per GB
    // allocated: profiles/r04_results/back_to_back_vs_paused_processes.txt) - spans of a file are the same size to a percent
    const size_t floor_bytes = bytes < 256 ? 256 : bytes;
    size_t want = bytes < 256 ? 256 : bytes < (32u << 20) ? bytes + bytes / 2 + (1u << 16) : bytes + bytes / 16 + (1u << 20);
    size_t got = 0;
    const int rc = device_alloc(c, &b.p, want, floor_bytes, &got);
    if (rc != INQ_OK) return rc;
    b.cap = got;
    return INQ_OK;
}

int upload(inq_ctx *c, hipStream_t s, std::initializer_list<Upload> ups) {
    for (const Upload &u : ups) {
        const int rc = ensure(c, *u.d, u.bytes);
        if (rc != INQ_OK) return rc;
        if (u.bytes) HIP_TRY(c, hipMemcpyAsync(u.d->p, u.h, u.bytes, hipMemcpyHostToDevice, s));
    }
    return INQ_OK;
}

int status_to_code(uint32_t st) {
    if (st & ST_HINT) return INQ_ERR_ARG;
    if (st & ST_LOCUS) return INQ_ERR_LOCUS;
    if (st & ST_INDEX) return INQ_ERR_INDEX;
    if (st & ST_CIGAR_OP) return INQ_ERR_CIGAR_OP;
    if (st & ST_RANGE) return INQ_ERR_RANGE;
    if (st & ST_PHASE) return INQ_ERR_PHASE;
    if (st & ST_AUX) return INQ_ERR_AUX;
    if (st & ST_INTERNAL) return INQ_ERR_HIP;  // a grid barrier gave up waiting (the grid drained; the rows of very deep loci are not there)
    return INQ_OK;
}

int status_readback(inq_ctx *c, DevStatus *dst, hipStream_t s) {
    HIP_TRY(c, hipMemcpyAsync(dst, c->d_status, sizeof(DevStatus), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemsetAsync(&c->d_status->err, 0, sizeof(unsigned int), s));
    HIP_TRY(c, hipMemsetAsync(&c->d_status->ties, 0, sizeof(unsigned long long), s));
    return INQ_OK;
}

DevBatch device_batch(const void *cigar, const void *reads, const void *pair_read, const void *off, const void *lstart, const void *lend,
                      uint64_t n_reads, uint64_t n_cigar_words, uint64_t n_pairs, uint64_t n_loci, uint32_t minlen, uint32_t support,
                      uint32_t unphased, void *p1, void *p2, void *pair_call, void *pair_bits) {
    DevBatch d;
    d.b = {n_reads, n_cigar_words, n_pairs, n_loci, (const uint32_t *)cigar, (const inq_read_t *)reads, (const uint32_t *)pair_read,
           (const uint64_t *)off, (const uint32_t *)lstart, (const uint32_t *)lend, minlen, support, unphased, 0u};
    d.r = {(double *)p1, (double *)p2, (int64_t *)pair_call, (uint8_t *)pair_bits, 0};
    return d;
}

// with timing on: an event triple from the pool (grown as needed), its e0 recorded on s; *ev stays null with timing off
static int timing_begin(inq_ctx *c, hipStream_t s, EvTriple **ev) {
    *ev = nullptr;
    if (!c->timing) return INQ_OK;
    if (c->ev_used == c->ev_pool.size()) {
        EvTriple t;
        HIP_TRY(c, hipEventCreate(&t.e0));
        HIP_TRY(c, hipEventCreate(&t.e1));
        HIP_TRY(c, hipEventCreate(&t.e2));
        c->ev_pool.push_back(t);
    }
    *ev = &c->ev_pool[c->ev_used++];
    (*ev)->one_kernel = false;
    HIP_TRY(c, hipEventRecord((*ev)->e0, s));
    return INQ_OK;
}

}  // namespace inq

extern "C" {

int inq_abi_version(void) { return INQ_ABI_VERSION; }

const char *inq_strerror(int code) {
    switch (code) {
    case INQ_OK: return "ok";
    case INQ_ERR_ARG: return "invalid argument (null pointer, inconsistent sizes or non-monotone offsets)";
    case INQ_ERR_SUPPORT_ZERO: return "support must be >= 1";
    case INQ_ERR_PHASE: return "a read passing the phased filter has HP outside {0,1,2}";
    case INQ_ERR_CIGAR_OP: return "CIGAR op code above 8";
    case INQ_ERR_LOCUS: return "locus start < 10 or end < start";
    case INQ_ERR_RANGE: return "read position plus reference span does not fit 31 bits";
    case INQ_ERR_INDEX: return "pair or CIGAR index outside the batch buffers";
    case INQ_ERR_HIP: return "HIP runtime error";
    case INQ_ERR_NOMEM: return "out of device memory";
    case INQ_ERR_INFLATE: return "a BGZF block does not inflate to its recorded size (corrupt or truncated BAM)";
    case INQ_ERR_BAM: return "corrupt BAM record chain, or records not coordinate-sorted";
    case INQ_ERR_AUX: return "HP aux of a fetched read is neither C nor i, or the SA aux of a kept read with a soft clip cannot be parsed (the reference panics)";
    case INQ_ERR_NO_DEVICE: return "no gfx950 (MI355X) device available; this library has no CPU fallback";
    default: return "unknown error";
    }
}

static void apply_default_options(inq_ctx *c);
static bool default_option(const char *key, int64_t *value);

// The context in two steps for a caller that is in a hurry: *out is set and *stage_ready raised as soon as the staging entry points
// (inq_span_stage_begin / _wait / inq_span_stage) may be used - the runtime is up, the copy and inflate streams and the staging
// slots exist - while the rest (status buffers, code objects: ~30 ms) is still being made; a process whose spans are already in
// memory starts uploading that much earlier.  Everything else may be called once the function has returned INQ_OK.  Whatever it
// returns, a context it has published stays valid until inq_ctx_destroy (the caller destroys it, also after a failure).
int inq_ctx_create_early(int device_id, inq_ctx_t **out, volatile int *stage_ready) {
    if (!out) return INQ_ERR_ARG;
    *out = nullptr;
    if (stage_ready) *stage_ready = 0;
    int n = 0;
    // INQ_TIMING=2: where the start-up goes (the runtime's own initialisation is most of a short run)
    HostClock clock("[inq ctx]");
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return INQ_ERR_NO_DEVICE;
    clock.lap("hipGetDeviceCount (runtime init)");
    if (device_id < 0 || device_id >= n) return INQ_ERR_ARG;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) return INQ_ERR_HIP;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return INQ_ERR_NO_DEVICE;
    inq_ctx *c = new (std::nothrow) inq_ctx();
    if (!c) return INQ_ERR_NOMEM;
    c->device = device_id;
    c->n_cus = (uint32_t)std::max(prop.multiProcessorCount, 1);
    c->grid_tail = std::min<uint32_t>(c->grid_tail, c->n_cus);  // a partitioned device (CPX: 32 CUs) takes a smaller grid
    c->backend = std::string("hip:") + prop.gcnArchName + ":" + prop.name;
    bool published = false;
    auto fail = [&](int code) {
        if (!published) inq_ctx_destroy(c);  // (a published context is the caller's to destroy: another thread may be using it)
        return code;
    };
    clock.lap("device properties");
    {   // "blocking_sync" has to be known before the first stream and event are made
        int64_t v = 0;
        if (default_option("blocking_sync", &v) && v) {
            c->blocking_sync = 1;
            (void)hipSetDeviceFlags(hipDeviceScheduleBlockingSync);  // (an error here - flags fixed by an earlier user of the device - is not ours to report)
            (void)hipGetLastError();
        }
    }
    if (hipSetDevice(device_id) != hipSuccess) return fail(INQ_ERR_HIP);
    // the streams of the staging path first (the process's first stream costs 18 - 170 ms, every further one 8): uploads and the
    // inflates behind them start while the rest of the context is still being made
    if (span_state_init(c) != INQ_OK) return fail(INQ_ERR_HIP);
    apply_default_options(c);
    clock.lap("hipSetDevice + copy / inflate streams, slots");
    *out = c;
    if (stage_ready) {
        published = true;
        __atomic_store_n(stage_ready, 1, __ATOMIC_RELEASE);
    }
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return fail(INQ_ERR_HIP);
    if (span_state_init_rest(c) != INQ_OK) return fail(INQ_ERR_HIP);
    clock.lap("main stream, span state");
    if (hipMalloc((void **)&c->d_status, sizeof(DevStatus)) != hipSuccess) return fail(INQ_ERR_NOMEM);
    if (hipMemset(c->d_status, 0, sizeof(DevStatus)) != hipSuccess) return fail(INQ_ERR_HIP);
    if (hipHostMalloc((void **)&c->h_status, sizeof(DevStatus), hipHostMallocDefault) != hipSuccess) return fail(INQ_ERR_NOMEM);
    clock.lap("status buffers");
    // load the code objects while the caller is still busy opening its input
    preload_locus(c->stream);
    preload_inflate(c->stream);
    preload_scan(c->stream);
    if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(INQ_ERR_HIP);
    clock.lap("code objects (3 empty launches)");
    return INQ_OK;
}

int inq_ctx_create(int device_id, inq_ctx_t **out) {
    const int rc = inq_ctx_create_early(device_id, out, nullptr);
    if (rc != INQ_OK && out) *out = nullptr;  // (nothing was published: the context is gone already)
    return rc;
}

int inq_ctx_create_multi(const int *device_ids, int n, inq_ctx_t **ctxs) {
    if (!device_ids || !ctxs || n <= 0 || n > 64) return INQ_ERR_ARG;
    for (int i = 0; i < n; ++i) ctxs[i] = nullptr;
    try {
        std::vector<int> rc((size_t)n, INQ_OK);
        std::vector<std::thread> th;
        for (int i = 0; i < n; ++i) th.emplace_back([&, i] { rc[(size_t)i] = inq_ctx_create(device_ids[i], &ctxs[i]); });
        for (auto &t : th) t.join();
        for (int i = 0; i < n; ++i)
            if (rc[(size_t)i] != INQ_OK) {
                for (int k = 0; k < n; ++k) {
                    inq_ctx_destroy(ctxs[k]);
                    ctxs[k] = nullptr;
                }
                return rc[(size_t)i];
            }
        return INQ_OK;
    } catch (...) {
        for (int k = 0; k < n; ++k) {
            inq_ctx_destroy(ctxs[k]);
            ctxs[k] = nullptr;
        }
        return INQ_ERR_NOMEM;
    }
}

void inq_ctx_destroy(inq_ctx_t *c) {
    if (!c) return;
    if (c->device >= 0) (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->span) span_state_destroy(c->span);
    purge_retired(c);
    for (DevBuf *b : c->bufs())
        if (b->p) (void)hipFree(b->p);
    for (auto &e : c->ev_pool) {
        (void)hipEventDestroy(e.e0);
        (void)hipEventDestroy(e.e1);
        (void)hipEventDestroy(e.e2);
    }
    if (c->d_status) (void)hipFree(c->d_status);
    if (c->h_status) (void)hipHostFree(c->h_status);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int inq_ctx_numa_node(const inq_ctx_t *c) {
    if (!c) return -1;
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, c->device) != hipSuccess) return -1;
    for (char *q = bus; *q; ++q)
        if (*q >= 'A' && *q <= 'F') *q = (char)(*q - 'A' + 'a');  // sysfs spells the address in lower case
    char path[160];
    std::snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bus);
    FILE *f = std::fopen(path, "r");
    if (!f) return -1;
    int node = -1;
    if (std::fscanf(f, "%d", &node) != 1) node = -1;
    std::fclose(f);
    return node;
}

const char *inq_backend_name(const inq_ctx_t *c) { return c ? c->backend.c_str() : "none"; }
const char *inq_last_error(const inq_ctx_t *c) { return c ? c->last_err.c_str() : ""; }

static int check_scalars(const inq_batch_t *b, const inq_result_t *r) {
    if (!b || !r) return INQ_ERR_ARG;
    if (b->n_loci && (!r->phase1 || !r->phase2)) return INQ_ERR_ARG;
    if (b->n_loci && (!b->locus_pair_off || !b->locus_start || !b->locus_end)) return INQ_ERR_ARG;
    if (b->n_pairs && (!b->pair_read || !b->reads || !b->n_reads)) return INQ_ERR_ARG;
    if (b->n_cigar_words && !b->cigar) return INQ_ERR_ARG;
    if (b->n_cigar_words % 4 != 0 || b->reserved != 0 || b->unphased > 1) return INQ_ERR_ARG;
    if (!b->n_loci && b->n_pairs) return INQ_ERR_ARG;
    if (b->n_loci >= 0xfffffff0ull || b->n_pairs >= (1ull << 40)) return INQ_ERR_ARG;
    if (b->support == 0) return INQ_ERR_SUPPORT_ZERO;
    return INQ_OK;
}

static int enqueue_batch(inq_ctx_t *c, const inq_batch_t *b, inq_result_t *r, void *hip_stream, const LocusExtras &x = LocusExtras()) {
    if (!c) return INQ_ERR_ARG;
    int rc = check_scalars(b, r);
    if (rc != INQ_OK) return rc;
    if (x.evidence && b->n_pairs && (!r->pair_call || !r->pair_bits)) return INQ_ERR_ARG;  // the counting reads both
    if (!x.kept_off != !x.kept || ((uintptr_t)x.kept & 15u) || ((uintptr_t)x.kept_off & 7u)) return INQ_ERR_ARG;
    if (x.kept && b->n_pairs && (!r->pair_call || !r->pair_bits)) return INQ_ERR_ARG;  // ... and so does the compaction
    if (x.names.recs && (!x.kept || !x.names.off || !x.name_off || ((uintptr_t)x.names.recs & 7u))) return INQ_ERR_ARG;  // who the records are
    if (x.seqs.recs && (!x.kept || !x.kept_pair || !x.seqs.off || !x.seq_qbeg || !x.seq_len || ((uintptr_t)x.seqs.recs & 7u))) return INQ_ERR_ARG;
    if (((uintptr_t)b->cigar & 15u) || ((uintptr_t)b->reads & 15u)) return INQ_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    const uint64_t blocks = (b->n_loci + 3) / 4;
    const uint32_t per_xcd = (uint32_t)((blocks + 7) / 8);
    const uint32_t grid_small = per_xcd * 8u;
    const uint32_t shard_cap = (grid_small / kListShards + 1u) * 4u;
    if ((rc = ensure(c, c->worklist, (size_t)shard_cap * kListShards * kListKinds * 4)) != INQ_OK) return rc;
    if ((rc = ensure(c, c->sval, (size_t)b->n_pairs * 8)) != INQ_OK) return rc;
    if ((rc = ensure(c, c->smeta, (size_t)b->n_pairs)) != INQ_OK) return rc;
    // loci of more than kGridSelectMin reads are reduced over the whole grid (deep_select.hip): a state of 74 KB each, and there
    // cannot be more of them than n_pairs / kGridSelectMin; nothing is allocated or launched when the depth hint rules them out
    const uint32_t hint = c->call_hint ? c->call_hint : c->max_reads_hint;
    const bool deep_possible = b->n_pairs > kGridSelectMin && !(hint && hint <= kGridSelectMin);
    if (deep_possible && (rc = ensure(c, c->deep, deep_select_scratch_bytes(b->n_pairs))) != INQ_OK) return rc;
    // evidence: the slice list of the loci one wave does not count; no list and no second launch when the depth hint rules them out
    const uint64_t ev_list_cap = x.evidence && b->n_pairs > kEvidenceWaveMax && !(hint && hint <= kEvidenceWaveMax) ? evidence_list_cap(b->n_pairs) : 0;
    if (x.evidence && (rc = ensure(c, c->evwork, evidence_scratch_bytes(ev_list_cap))) != INQ_OK) return rc;
    if (x.kept && b->n_pairs && (rc = ensure(c, c->rctiles, read_call_scratch_bytes(b->n_pairs))) != INQ_OK) return rc;

    KArgs a;
    a.cigar4 = (const uint4 *)b->cigar;
    a.reads = (const uint4 *)b->reads;
    a.pair_read = b->pair_read;
    a.locus_pair_off = b->locus_pair_off;
    a.locus_start = b->locus_start;
    a.locus_end = b->locus_end;
    a.n_reads = b->n_reads;
    a.n_cigar4 = b->n_cigar_words / 4;
    a.n_pairs = b->n_pairs;
    a.n_loci = b->n_loci;
    a.minlen = b->minlen;
    a.support = b->support;
    a.phase1 = r->phase1;
    a.phase2 = r->phase2;
    a.pair_call = r->pair_call;
    a.pair_bits = r->pair_bits;
    a.status = c->d_status;
    a.worklist = (uint32_t *)c->worklist.p;
    a.sval = (int64_t *)c->sval.p;
    a.smeta = (uint8_t *)c->smeta.p;
    a.blocks_per_xcd = per_xcd;
    a.shard_cap = shard_cap;
    c->call_hint = 0;
    a.max_reads_hint = hint;
    a.locus_flags = x.flags;

    // CIGAR words of a read referenced by one locus only are read exactly once: stream them past the
    // caches (nt).  Reads shared by neighbouring loci keep the default policy so the second locus hits L2.
    const bool nt = c->nt_loads < 0 ? (b->n_pairs <= b->n_reads) : (c->nt_loads != 0);
    EvTriple *ev;
    if ((rc = timing_begin(c, s, &ev)) != INQ_OK) return rc;
    if (x.flags) HIP_TRY(c, hipMemsetAsync(x.flags, 0, (size_t)b->n_loci, s));  // the kernels store tie loci only
    if (x.evidence) HIP_TRY(c, hipMemsetAsync(c->evwork.p, 0, sizeof(EvidenceWork), s));  // the slice list starts empty
    const bool more_kernels = launch_locus_call(a, b->unphased != 0, nt, grid_small, c->grid_medium, c->grid_tail, s, ev ? ev->e1 : nullptr, deep_possible ? c->deep.p : nullptr);
    HIP_TRY(c, hipGetLastError());
    // what both kernels behind the locus kernels read: the batch's pairs, and what was just written for each
    const PairView view{b->locus_pair_off, r->pair_bits, r->pair_call, b->pair_read, (const uint32_t *)b->reads, b->n_reads, b->n_pairs, b->n_loci};
    if (x.evidence) {
        EvidenceWork *const work = (EvidenceWork *)c->evwork.p;
        launch_evidence(EvidenceArgs{view, x.evidence, work, (EvidenceSlice *)(work + 1), ev_list_cap}, b->unphased != 0, c->n_cus * 4u, s);
        HIP_TRY(c, hipGetLastError());
    }
    if (x.kept && !b->n_pairs) HIP_TRY(c, hipMemsetAsync(x.kept_off, 0, (size_t)(b->n_loci + 1) * 8, s));  // no pair: every list is empty
    if (x.kept && b->n_pairs) {
        uint64_t *const tile_base = (uint64_t *)c->rctiles.p;
        launch_read_calls(ReadCallArgs{view, x.kept_off, x.kept, (uint32_t *)(tile_base + read_call_tiles(b->n_pairs) + 1), tile_base, x.kept_pair},
                          b->unphased != 0, s);
        HIP_TRY(c, hipGetLastError());
    }
    // The byte runs of a kind, behind the scatter: a record per record it wrote (`records`: the kind's own kernel), then where each
    // record's bytes will go.  No pair: no record, no byte
    const uint64_t *const n_kept = x.kept_off ? x.kept_off + b->n_loci : nullptr;
    auto place_runs = [&](const auto &runs, auto &&records) {
        if (!runs.recs) return hipSuccess;
        if (!b->n_pairs) return hipMemsetAsync(runs.off, 0, 8, s);
        records();
        launch_scan_run_bytes(runs.recs, n_kept, runs.off, b->n_pairs, runs.off + b->n_pairs + 1, s);
        return hipGetLastError();
    };
    // an origin per record (its read's descriptor and name length); the slice of the pair each record came from
    const auto origins = [&] { launch_read_origins(ReadOriginArgs{x.kept, n_kept, view.read_words, b->n_reads, x.name_off, x.names.recs, b->n_pairs}, c->grid_side, s); };
    const auto slices = [&] { launch_read_seq_records(ReadSeqArgs{x.kept_pair, n_kept, x.seq_qbeg, x.seq_len, x.seqs.recs, b->n_pairs}, c->grid_side, s); };
    HIP_TRY(c, place_runs(x.names, origins));
    HIP_TRY(c, place_runs(x.seqs, slices));
    // what both motif kernels read: the records the scatter wrote, locus by locus, and the batch's own slices, a segment per pair
    const KeptSlices kept{x.kept_pair, n_kept, x.kept_off, b->n_loci, x.seq_bytes, x.seq_n_bytes, x.seq_off, x.seq_len, b->n_pairs, b->n_pairs};
    // the motif each locus's reads repeat: behind the slices' records (kept_pair, kept_off), in front of the motif kernel, which reads
    // the words this writes.  No pair: no record, every locus's answer is zeros
    if (x.locus_found && !b->n_pairs) HIP_TRY(c, hipMemsetAsync(x.locus_found, 0, (size_t)b->n_loci * sizeof(inq_locus_motif_t), s));
    if (x.locus_found && b->n_pairs) {
        launch_locus_motifs(LocusMotifArgs{kept, x.motif_given, x.locus_found, x.motif_use}, c->grid_side, s);
        HIP_TRY(c, hipGetLastError());
    }
    // the motif runs of each record's bases: in front of nothing
    if (x.motifs && b->n_pairs) {
        launch_read_motifs(ReadMotifArgs{kept, x.motif_word, x.motifs}, c->grid_side, s);
        HIP_TRY(c, hipGetLastError());
    }
    // e2 ends the sequence - unless the sequence was locus_call_small alone (a depth hint of at most 64 reads and no side output, which
    // are all launched behind it): e1 stands behind that already, and a second record right behind it would only hold the stream
    const bool side_outputs = x.evidence || x.kept || x.names.recs || x.seqs.recs || x.locus_found || x.motifs;
    if (ev) {
        ev->one_kernel = !more_kernels && !side_outputs;
        if (!ev->one_kernel) HIP_TRY(c, hipEventRecord(ev->e2, s));
    }
    return INQ_OK;
}

int inq_call_batch_device(inq_ctx_t *c, const inq_batch_t *b, inq_result_t *r, void *hip_stream) {
    return inq_call_batch_device_flags(c, b, r, nullptr, hip_stream);
}

int inq_call_batch_device_flags(inq_ctx_t *c, const inq_batch_t *b, inq_result_t *r, uint8_t *d_locus_flags, void *hip_stream) {
    return inq_call_batch_device_evidence(c, b, r, d_locus_flags, nullptr, hip_stream);
}

int inq_call_batch_device_evidence(inq_ctx_t *c, const inq_batch_t *b, inq_result_t *r, uint8_t *d_locus_flags, inq_locus_evidence_t *d_evidence,
                                   void *hip_stream) {
    return inq_call_batch_device_reads(c, b, r, d_locus_flags, d_evidence, nullptr, nullptr, hip_stream);
}

int inq_call_batch_device_reads(inq_ctx_t *c, const inq_batch_t *b, inq_result_t *r, uint8_t *d_locus_flags, inq_locus_evidence_t *d_evidence,
                                uint64_t *d_kept_off, inq_read_call_t *d_kept, void *hip_stream) {
    return guarded([&] { return enqueue_batch(c, b, r, hip_stream, LocusExtras{d_locus_flags, d_evidence, d_kept_off, d_kept}); });
}

int inq_ctx_status(inq_ctx_t *c, uint64_t *n_tie_loci) {
    if (!c) return INQ_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipDeviceSynchronize());
    const int rc = status_readback(c, c->h_status, c->stream);
    if (rc != INQ_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (n_tie_loci) *n_tie_loci = c->h_status->ties;
    return status_to_code(c->h_status->err);
}

static int call_batch_impl(inq_ctx_t *c, const inq_batch_t *b, inq_result_t *r, const HostExtras &h) {
    if (!c) return INQ_ERR_ARG;
    extras_reset(c);
    int rc = check_scalars(b, r);
    if (rc != INQ_OK) return rc;
    // host-side shape checks: everything the grid and the kernels' indexing assume
    uint64_t max_reads = 0;
    if (b->n_loci) {
        // (the offsets first, all of them: a locus's depth below is a difference of two that ascend)
        const uint64_t *const off = b->locus_pair_off;
        if (off[0] != 0 || off[b->n_loci] != b->n_pairs || !offsets_ok(off, b->n_loci, b->n_pairs)) return INQ_ERR_ARG;
        for (uint64_t j = 0; j < b->n_loci; ++j) {
            if (!locus_ok(b->locus_start[j], b->locus_end[j])) return INQ_ERR_LOCUS;
            max_reads = std::max<uint64_t>(max_reads, b->locus_pair_off[j + 1] - b->locus_pair_off[j]);
        }
    }
    r->n_tie_loci = 0;
    if (b->n_loci == 0) {
        extras_finish(c, 0, 0, h, 0);
        return INQ_OK;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    rc = upload(c, s, {{&c->cigar, b->cigar, (size_t)b->n_cigar_words * 4},
                       {&c->reads, b->reads, (size_t)b->n_reads * sizeof(inq_read_t)},
                       {&c->pair_read, b->pair_read, (size_t)b->n_pairs * 4},
                       {&c->off, b->locus_pair_off, (size_t)(b->n_loci + 1) * 8},
                       {&c->lstart, b->locus_start, (size_t)b->n_loci * 4},
                       {&c->lend, b->locus_end, (size_t)b->n_loci * 4}});
    if (rc != INQ_OK) return rc;
    if ((rc = ensure(c, c->p1, (size_t)b->n_loci * 8)) != INQ_OK) return rc;
    if ((rc = ensure(c, c->p2, (size_t)b->n_loci * 8)) != INQ_OK) return rc;
    const bool want_call = r->pair_call || h.per_pair(), want_bits = r->pair_bits || h.per_pair();
    if (r->pair_call && (rc = ensure(c, c->pcall, (size_t)b->n_pairs * 8)) != INQ_OK) return rc;
    if (r->pair_bits && (rc = ensure(c, c->pbits, (size_t)b->n_pairs)) != INQ_OK) return rc;
    LocusExtras x;
    if ((rc = extras_prepare(c, b->n_loci, b->n_pairs, h, &x)) != INQ_OK) return rc;

    DevBatch d = device_batch(c->cigar.p, c->reads.p, c->pair_read.p, c->off.p, c->lstart.p, c->lend.p, b->n_reads, b->n_cigar_words,
                              b->n_pairs, b->n_loci, b->minlen, b->support, b->unphased, c->p1.p, c->p2.p,
                              want_call ? c->pcall.p : nullptr, want_bits ? c->pbits.p : nullptr);
    const inq_result_t &dr = d.r;
    c->call_hint = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(max_reads, 1), 0xffffffffull);  // skips the deep-locus launches when no locus needs them
    if ((rc = enqueue_batch(c, &d.b, &d.r, s, x)) != INQ_OK) return rc;
    if ((rc = extras_download(c, b->n_loci, h, x, h.flags, s)) != INQ_OK) return rc;  // (the flags: straight to the caller's array)
    HIP_TRY(c, hipMemcpyAsync(r->phase1, dr.phase1, (size_t)b->n_loci * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(r->phase2, dr.phase2, (size_t)b->n_loci * 8, hipMemcpyDeviceToHost, s));
    if (r->pair_call && b->n_pairs)
        HIP_TRY(c, hipMemcpyAsync(r->pair_call, dr.pair_call, (size_t)b->n_pairs * 8, hipMemcpyDeviceToHost, s));
    if (r->pair_bits && b->n_pairs)
        HIP_TRY(c, hipMemcpyAsync(r->pair_bits, dr.pair_bits, (size_t)b->n_pairs, hipMemcpyDeviceToHost, s));
    if ((rc = status_readback(c, c->h_status, s)) != INQ_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(s));  // the one synchronisation of the call
    purge_retired(c);  // the stream is idle: buffers this call outgrew go back now
    r->n_tie_loci = c->h_status->ties;
    extras_finish(c, b->n_loci, b->n_pairs, h, c->h_status->err);
    return status_to_code(c->h_status->err);
}

int inq_call_batch(inq_ctx_t *c, const inq_batch_t *b, inq_result_t *r) { return inq_call_batch_flags(c, b, r, nullptr); }

int inq_call_batch_flags(inq_ctx_t *c, const inq_batch_t *b, inq_result_t *r, uint8_t *locus_flags) {
    return inq_call_batch_evidence(c, b, r, locus_flags, nullptr);
}

int inq_call_batch_evidence(inq_ctx_t *c, const inq_batch_t *b, inq_result_t *r, uint8_t *locus_flags, inq_locus_evidence_t *evidence) {
    return inq_call_batch_reads(c, b, r, locus_flags, evidence, nullptr);
}

int inq_call_batch_reads(inq_ctx_t *c, const inq_batch_t *b, inq_result_t *r, uint8_t *locus_flags, inq_locus_evidence_t *evidence,
                         uint64_t *kept_off) {
    return guarded([&] { return call_batch_impl(c, b, r, HostExtras{locus_flags, evidence, kept_off}); });
}

static int outlier_rows_impl(inq_ctx_t *c, const float *values, const uint32_t *row_len, uint64_t n_rows, uint32_t stride,
                             int method, uint32_t minsize, float cutoff, uint32_t mincluster, uint8_t *flags, uint8_t *keep) {
    if (!c || (method != INQ_OUTLIER_ZSCORE && method != INQ_OUTLIER_DBSCAN)) return INQ_ERR_ARG;
    if (n_rows && (!row_len || !keep || (stride && (!values || !flags)))) return INQ_ERR_ARG;
    if (n_rows >= 0x7fffffffull) return INQ_ERR_ARG;
    for (uint64_t i = 0; i < n_rows; ++i)
        if (row_len[i] > stride) return INQ_ERR_ARG;
    if (!n_rows) return INQ_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t cells = (size_t)n_rows * stride;
    int rc;
    if ((rc = ensure(c, c->ovalues, cells * 4)) != INQ_OK) return rc;
    if ((rc = ensure(c, c->olen, n_rows * 4)) != INQ_OK) return rc;
    if ((rc = ensure(c, c->oflags, cells)) != INQ_OK) return rc;
    if ((rc = ensure(c, c->okeep, n_rows)) != INQ_OK) return rc;
    const bool tile = c->outlier_tile && stride <= kOutlierTileMaxStride;
    if (method == INQ_OUTLIER_ZSCORE && !tile && (rc = ensure(c, c->otrans, outlier_rows_padded(n_rows) * stride * 4)) != INQ_OK) return rc;
    if (cells) HIP_TRY(c, hipMemcpyAsync(c->ovalues.p, values, cells * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->olen.p, row_len, n_rows * 4, hipMemcpyHostToDevice, s));
    if (cells) HIP_TRY(c, hipMemsetAsync(c->oflags.p, 0, cells, s));
    OutlierArgs a;
    a.values = (const float *)c->ovalues.p;
    a.row_len = (const uint32_t *)c->olen.p;
    a.n_rows = n_rows;
    a.stride = stride;
    a.minsize = minsize;
    a.zscore_cutoff = cutoff;
    a.mincluster = mincluster;
    a.flags = (uint8_t *)c->oflags.p;
    a.keep = (uint8_t *)c->okeep.p;
    EvTriple *ev;
    if ((rc = timing_begin(c, s, &ev)) != INQ_OK) return rc;
    launch_outlier(a, method, (float *)c->otrans.p, s, tile);
    HIP_TRY(c, hipGetLastError());
    if (ev) {
        HIP_TRY(c, hipEventRecord(ev->e1, s));
        HIP_TRY(c, hipEventRecord(ev->e2, s));
    }
    if (cells) HIP_TRY(c, hipMemcpyAsync(flags, c->oflags.p, cells, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(keep, c->okeep.p, n_rows, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return INQ_OK;
}

int inq_outlier_rows(inq_ctx_t *c, const float *values, const uint32_t *row_len, uint64_t n_rows, uint32_t stride, int method,
                     uint32_t minsize, float zscore_cutoff, uint32_t mincluster, uint8_t *flags, uint8_t *keep) {
    return guarded([&] { return outlier_rows_impl(c, values, row_len, n_rows, stride, method, minsize, zscore_cutoff, mincluster, flags, keep); });
}

// firth_when 0: inq_assoc_rows.  Else inq_assoc_rows_firth: the same launches, the ordinary kernel also leaving each row's smallest
// min(mu, 1 - mu), and behind each the Firth kernel, which picks its rows on the device
static int assoc_rows_impl(inq_ctx_t *c, const float *values, uint64_t n_rows, uint32_t n_samples, const double *y, const double *cov,
                           uint32_t k, int outcome, int str_mode, double missing_cutoff, inq_assoc_row_t *rows, int firth_when = 0,
                           inq_assoc_firth_row_t *firth = nullptr) {
    if (!c || (outcome != INQ_ASSOC_BINARY && outcome != INQ_ASSOC_CONTINUOUS)) return INQ_ERR_ARG;
    if (n_rows && firth_when && !firth) return INQ_ERR_ARG;
    if (str_mode != INQ_ASSOC_MAX && str_mode != INQ_ASSOC_MIN && str_mode != INQ_ASSOC_MEAN) return INQ_ERR_ARG;
    if (n_samples > kAssocMaxSamples || k > kAssocMaxCov || missing_cutoff != missing_cutoff) return INQ_ERR_ARG;
    if (n_rows && (!rows || (n_samples && (!values || !y || (k && !cov))))) return INQ_ERR_ARG;
    if (outcome == INQ_ASSOC_BINARY && n_rows)
        for (uint32_t i = 0; i < n_samples; ++i)
            if (y[i] != 0.0 && y[i] != 1.0) return INQ_ERR_ARG;
    if (!n_rows) return INQ_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    // 1 / B(df / 2, 1 / 2) of the Student-t p-value for every df a row can have: c[df + 2] = c[df] (df + 1) / df from c[1] = 1 / pi,
    // c[2] = 1 / 2 (no lgamma: a difference of two of its values near 600 loses three digits of the p-value)
    std::vector<double> tcoef;
    if (outcome == INQ_ASSOC_CONTINUOUS) {
        tcoef.assign((size_t)n_samples + 3, 0.0);
        tcoef[1] = 0.31830988618379067154, tcoef[2] = 0.5;
        for (uint32_t df = 1; df + 2 <= n_samples; ++df) tcoef[df + 2] = tcoef[df] * (double)(df + 1) / (double)df;
        tcoef.resize((size_t)n_samples + 1);
    }
    const size_t row_bytes = (size_t)n_samples * 8;
    uint64_t tile = c->assoc_tile_rows ? c->assoc_tile_rows : std::max<uint64_t>(1, (256ull << 20) / std::max<size_t>(row_bytes, 1));
    tile = std::min<uint64_t>({tile, n_rows, 1ull << 30});
    int rc;
    if ((rc = upload(c, s, {{&c->ay, y, (size_t)n_samples * 8}, {&c->acov, cov, (size_t)k * n_samples * 8},
                            {&c->atcoef, tcoef.data(), tcoef.size() * 8}})) != INQ_OK)
        return rc;
    if ((rc = ensure(c, c->avalues, tile * row_bytes)) != INQ_OK) return rc;
    if ((rc = ensure(c, c->arows, tile * sizeof(inq_assoc_row_t))) != INQ_OK) return rc;
    if (firth_when) {
        if ((rc = ensure(c, c->aminmu, tile * sizeof(double))) != INQ_OK) return rc;
        if ((rc = ensure(c, c->afirth, tile * sizeof(inq_assoc_firth_row_t))) != INQ_OK) return rc;
    }
    AssocArgs a;
    a.values = (const float *)c->avalues.p;
    a.n_samples = n_samples;
    a.k = k;
    a.y = (const double *)c->ay.p;
    a.cov = (const double *)c->acov.p;
    a.tcoef = (const double *)c->atcoef.p;
    a.outcome = outcome, a.str_mode = str_mode;
    a.missing_cutoff = missing_cutoff;
    a.rows = (inq_assoc_row_t *)c->arows.p;
    if (firth_when) {
        a.min_mu = (double *)c->aminmu.p;
        a.firth = (inq_assoc_firth_row_t *)c->afirth.p;
        a.firth_when = firth_when;
        a.firth_mu_bound = (double)c->assoc_firth_mu_ppb / 1e9;
    }
    // tile by tile on one stream: a tile's upload waits for the launch that read the buffer before it
    for (uint64_t r0 = 0; r0 < n_rows; r0 += tile) {
        a.n_rows = std::min<uint64_t>(tile, n_rows - r0);
        if (row_bytes) HIP_TRY(c, hipMemcpyAsync(c->avalues.p, values + r0 * 2 * n_samples, a.n_rows * row_bytes, hipMemcpyHostToDevice, s));
        EvTriple *ev;
        if ((rc = timing_begin(c, s, &ev)) != INQ_OK) return rc;
        launch_assoc(a, s);
        HIP_TRY(c, hipGetLastError());
        if (firth_when) {
            launch_assoc_firth(a, s);
            HIP_TRY(c, hipGetLastError());
        }
        if (ev) {
            HIP_TRY(c, hipEventRecord(ev->e1, s));
            HIP_TRY(c, hipEventRecord(ev->e2, s));
        }
        HIP_TRY(c, hipMemcpyAsync(rows + r0, c->arows.p, a.n_rows * sizeof(inq_assoc_row_t), hipMemcpyDeviceToHost, s));
        if (firth_when) HIP_TRY(c, hipMemcpyAsync(firth + r0, c->afirth.p, a.n_rows * sizeof(inq_assoc_firth_row_t), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    return INQ_OK;
}

int inq_assoc_rows(inq_ctx_t *c, const float *values, uint64_t n_rows, uint32_t n_samples, const double *y, const double *cov, uint32_t k,
                   int outcome, int str_mode, double missing_cutoff, inq_assoc_row_t *rows) {
    return guarded([&] { return assoc_rows_impl(c, values, n_rows, n_samples, y, cov, k, outcome, str_mode, missing_cutoff, rows); });
}

int inq_assoc_rows_firth(inq_ctx_t *c, const float *values, uint64_t n_rows, uint32_t n_samples, const double *y, const double *cov,
                         uint32_t k, int str_mode, double missing_cutoff, int when, inq_assoc_row_t *rows, inq_assoc_firth_row_t *firth) {
    if (when != INQ_ASSOC_FIRTH_FALLBACK && when != INQ_ASSOC_FIRTH_ALWAYS) return INQ_ERR_ARG;
    return guarded([&] { return assoc_rows_impl(c, values, n_rows, n_samples, y, cov, k, INQ_ASSOC_BINARY, str_mode, missing_cutoff, rows, when, firth); });
}

int inq_ctx_timing_enable(inq_ctx_t *c, int on) {
    if (!c) return INQ_ERR_ARG;
    c->timing = on != 0;
    return INQ_OK;
}

int inq_ctx_timing_reset(inq_ctx_t *c) {
    if (!c) return INQ_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipDeviceSynchronize());
    c->ev_used = 0;
    return INQ_OK;
}

int inq_ctx_timing_read(inq_ctx_t *c, int which, double *total_ms, uint64_t *launches) {
    if (!c || which < 0 || which > 2) return INQ_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    if (which == 2) {  // the last BGZF inflate launch (device front end)
        HIP_TRY(c, hipDeviceSynchronize());
        const double ms = span_last_inflate_ms(c->span);
        if (total_ms) *total_ms = ms < 0 ? 0.0 : ms;
        if (launches) *launches = ms < 0 ? 0u : 1u;
        return INQ_OK;
    }
    double tot = 0.0;
    for (size_t i = 0; i < c->ev_used; ++i) {
        EvTriple &e = c->ev_pool[i];
        const hipEvent_t last = e.one_kernel ? e.e1 : e.e2;
        HIP_TRY(c, hipEventSynchronize(last));
        float ms = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&ms, e.e0, which == 0 ? last : e.e1));
        tot += (double)ms;
    }
    if (total_ms) *total_ms = tot;
    if (launches) *launches = (uint64_t)c->ev_used;
    return INQ_OK;
}

// options every context made from now on starts with (inq_default_option): applied inside inq_ctx_create_early BEFORE the context is
// published for staging, so that an uploader thread never sees the built-in value of e.g. "inflate_ahead"
static std::mutex g_defaults_mu;
static std::vector<std::pair<std::string, int64_t>> g_defaults;

int inq_default_option(const char *key, int64_t value) {
    if (!key) return INQ_ERR_ARG;
    try {
        inq_ctx probe;  // the key and the value are checked on a context that is never opened
        probe.n_cus = 256;
        const int rc = inq_ctx_set_option(&probe, key, value);
        if (rc != INQ_OK) return rc;
        std::lock_guard<std::mutex> g(g_defaults_mu);
        for (auto &kv : g_defaults)
            if (kv.first == key) {
                kv.second = value;
                return INQ_OK;
            }
        g_defaults.emplace_back(key, value);
        return INQ_OK;
    } catch (...) {
        return INQ_ERR_NOMEM;
    }
}

static bool default_option(const char *key, int64_t *value) {
    std::lock_guard<std::mutex> g(g_defaults_mu);
    for (auto &kv : g_defaults)
        if (kv.first == key) {
            if (value) *value = kv.second;
            return true;
        }
    return false;
}
int inq_default_option_get(const char *key, int64_t *value) {
    if (!key) return INQ_ERR_ARG;
    try {
        return default_option(key, value) ? INQ_OK : INQ_ERR_ARG;
    } catch (...) {
        return INQ_ERR_NOMEM;
    }
}

static void apply_default_options(inq_ctx *c) {
    std::vector<std::pair<std::string, int64_t>> d;
    {
        std::lock_guard<std::mutex> g(g_defaults_mu);
        d = g_defaults;
    }
    for (auto &kv : d) (void)inq_ctx_set_option(c, kv.first.c_str(), kv.second);
}

int inq_ctx_set_option(inq_ctx_t *c, const char *key, int64_t value) {
    if (!c || !key) return INQ_ERR_ARG;
    if (std::strcmp(key, "grid_tail") == 0 || std::strcmp(key, "grid_big") == 0) {  // ("grid_big": the name up to ABI v4)
        if (value < 1 || value > 65535) return INQ_ERR_ARG;
        c->grid_tail = std::min<uint32_t>((uint32_t)value, c->n_cus ? c->n_cus : 1u);  // all of them must be resident at once
        return INQ_OK;
    }
    if (std::strcmp(key, "grid_medium") == 0) {
        if (value < 1 || value > 65535) return INQ_ERR_ARG;
        c->grid_medium = (uint32_t)value;
        return INQ_OK;
    }
    if (std::strcmp(key, "grid_side") == 0) {  // 0: every side kernel's launcher keeps its own cap
        if (value < 0 || value > 65535) return INQ_ERR_ARG;
        c->grid_side = (uint32_t)value;
        return INQ_OK;
    }
    if (std::strcmp(key, "max_reads_hint") == 0) {
        if (value < 0 || value > 0xffffffffll) return INQ_ERR_ARG;
        c->max_reads_hint = (uint32_t)value;
        return INQ_OK;
    }
    if (std::strcmp(key, "verify_crc") == 0) {
        c->verify_crc = value != 0;
        return INQ_OK;
    }
    if (std::strcmp(key, "inflate_algo") == 0) {
        // one kernel is left (a workgroup per BGZF block): 0 names it, 2 used to mean "the quicker one", 1 was the removed one
        return value == 0 || value == 2 ? INQ_OK : INQ_ERR_ARG;
    }
    if (std::strcmp(key, "inflate_lit_pairs") == 0) {
        c->inflate_lit_pairs = value < 0 ? -1 : (value != 0);
        return INQ_OK;
    }
    if (std::strcmp(key, "outlier_tile") == 0) {
        c->outlier_tile = value != 0;
        return INQ_OK;
    }
    if (std::strcmp(key, "assoc_tile_rows") == 0) {
        if (value < 0) return INQ_ERR_ARG;
        c->assoc_tile_rows = (uint64_t)value;
        return INQ_OK;
    }
    if (std::strcmp(key, "assoc_firth_mu_ppb") == 0) {
        if (value < 0) return INQ_ERR_ARG;
        c->assoc_firth_mu_ppb = (uint64_t)value;
        return INQ_OK;
    }
    if (std::strcmp(key, "blocking_sync") == 0) {
        // as a default option (set BEFORE the context is made) it also makes the context's events blocking ones; on a live context it
        // switches the device's wait mode only
        c->blocking_sync = value != 0;
        if (c->device >= 0 && c->stream) {
            (void)hipSetDevice(c->device);
            (void)hipSetDeviceFlags(value ? hipDeviceScheduleBlockingSync : hipDeviceScheduleSpin);
            (void)hipGetLastError();
        }
        return INQ_OK;
    }
    if (std::strcmp(key, "inflate_ahead") == 0) {
        c->inflate_ahead = value != 0;
        return INQ_OK;
    }
    if (std::strcmp(key, "batch_loci_hint") == 0) {
        c->batch_loci_hint = value < 0 ? 0u : (uint64_t)value;
        return INQ_OK;
    }
    if (std::strcmp(key, "gather_nt") == 0) {
        c->gather_nt = value != 0;
        return INQ_OK;
    }
    if (std::strcmp(key, "inflate_tokens") == 0) {
        c->inflate_tokens = value < 0 ? -1 : (value != 0);
        return INQ_OK;
    }
    if (std::strcmp(key, "retired_limit_mb") == 0) {  // outgrown buffers parked before they are given back (default 16384)
        if (value < 0 || value > (1ll << 20)) return INQ_ERR_ARG;
        c->retired_limit = (size_t)value << 20;
        return INQ_OK;
    }
    if (std::strcmp(key, "test_fail_allocs") == 0) {  // test seam: the next N device allocations see "out of memory" at their first attempt
        if (value < 0 || value > 1000000) return INQ_ERR_ARG;
        c->test_fail_allocs = (uint32_t)value;
        return INQ_OK;
    }
    if (std::strcmp(key, "nt_loads") == 0) {
        c->nt_loads = value < 0 ? -1 : (value != 0);
        return INQ_OK;
    }
    return INQ_ERR_ARG;
}

uint64_t inq_ctx_alloc_retries(const inq_ctx_t *c) { return c ? c->alloc_retries : 0; }

int inq_pin_host(void *p, size_t bytes) {
    if (!p || !bytes) return INQ_ERR_ARG;
    return hipHostRegister(p, bytes, hipHostRegisterDefault) == hipSuccess ? INQ_OK : INQ_ERR_HIP;
}

void inq_unpin_host(void *p) {
    if (p) (void)hipHostUnregister(p);
}

int inq_alloc_pinned(size_t bytes, void **out) {
    if (!out) return INQ_ERR_ARG;
    *out = nullptr;
    hipError_t e = hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault);
    if (e == hipErrorOutOfMemory) return INQ_ERR_NOMEM;
    if (e != hipSuccess) return INQ_ERR_NO_DEVICE;
    return INQ_OK;
}

void inq_free_pinned(void *p) {
    if (p) (void)hipHostFree(p);
}

}  // extern "C"

int inq::call_batch_device_impl(inq_ctx *c, const inq_batch_t *b, inq_result_t *r, void *hip_stream, const LocusExtras &x) {
    return enqueue_batch(c, b, r, hip_stream, x);
}
