// driver_internal.h - what the pieces of the host driver share (run.cc, span_pipeline.cc, session.cc, combine.cc,
// hostapi_probes.cc): the prepared call, the asynchronously created device context, the hooks a session adds to a call.
#pragma once
#include <sys/mman.h>
#include <fcntl.h>
#include <sched.h>
#include <sys/stat.h>
#include <sys/syscall.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <future>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/inquistr_host.h"
#include "../csrc/run_bytes.h"
#include "front_end.h"
#include "front_pool.h"
#include "host_common.h"
#include "inq_text.h"
#include "sa2d.h"
#include "span_pipeline.h"
#include "span_planner.h"
#include "targets.h"

namespace inqhost {

// Experiments' switches (INQ_SPAN_REGISTER, INQ_SPAN_BUFFERS, INQ_IO_PIN, INQ_EXIT_PROBE, INQ_GATE_READS, INQ_SPAN_PINNED) are read from
// the environment only by a build with -DINQ_DEBUG_ENV (make DEBUG_ENV=1).  What the shipped host library reads is listed in
// INQ_TIMING, INQ_FRONTEND, INQ_SPAN_MB, INQ_SPAN_GAP_BYTES, INQ_SPAN_JOB_BYTES, INQ_FLUSH_LOCI, INQ_NUMA_NODE, INQ_NUMA_CPUS,
// INQ_CTX_TIMEOUT_S, INQ_FAST_EXIT, INQ_SERVER, INQ_SERVER_IDLE, INQ_HOST_LIB, and torch.distributed.run's LOCAL_WORLD_SIZE / LOCAL_RANK.
#ifdef INQ_DEBUG_ENV
inline const char *debug_env(const char *name) { return std::getenv(name); }
#else
inline const char *debug_env(const char *) { return nullptr; }
#endif

// fast_exit(), timing_level(), Clock / secs / ms, set_err, write_all, Failure and INQ_GUARD: host_common.h, which the text commands
// (outlier.cc, assoc.cc) include without the rest of this header
inline bool starts_with(const std::string &s, const char *p) { return s.compare(0, std::strlen(p), p) == 0; }
inline bool ends_with(const std::string &s, const char *p) {
    size_t n = std::strlen(p);
    return s.size() >= n && s.compare(s.size() - n, n, p) == 0;
}
inline bool is_file(const std::string &p) {
    struct stat st;
    return ::stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode);
}

struct Prepared {
    std::unique_ptr<BamFile> bam;
    std::vector<RepeatInterval> targets;
    std::vector<std::string> target_name;  // column 4 of the BED, [k] of targets[k]; empty where there is none (TargetsResult::name)
    std::string sample;
};

// src/call.rs:87-102 + get_targets :182-202.  Returns an exit status.
// A cohort is called with ONE BED: inside a session (inquistr cohort / serve) the parsed and validated target list of the last BED is
// kept and taken again when the file is the same (device, inode, size, modification time) and the BAM's contigs are (names and lengths
// decide every check of from_bed, src/repeats.rs:96-115).  100 000 targets: 12 - 25 ms of a 70 ms call.
struct BedKey {
    std::string path;
    uint64_t dev = 0, ino = 0, size = 0;
    int64_t mtime_ns = 0;
    std::map<std::string, uint64_t> lengths;
    bool operator==(const BedKey &o) const {
        return path == o.path && dev == o.dev && ino == o.ino && size == o.size && mtime_ns == o.mtime_ns && lengths == o.lengths;
    }
};
struct BedCache {
    std::mutex mu;
    BedKey key;
    TargetsResult tr;
    bool valid = false;
};

int prepare(const inq_call_args_t *a, Prepared &P, std::string &msg, BedCache *bed_cache = nullptr);
// The motif words of P's targets for the read-motifs file: `motif` for every target, or (null) column 4 of the BED, each through
// motif_encode; a target whose text does not encode gets word 0 and their number goes to stderr once.  INQ_EXIT_ERROR and a message
// when `motif` does not encode, or when there is neither it nor a fourth column
// (need_given false - `--motif auto`, or the locus-motifs file alone: the words are the catalogue's to compare with, a target without
// one gets 0, a list without a fourth column is no error and nothing goes to stderr; `auto` itself stands for no `motif`)
int target_motif_words(const Prepared &P, const char *motif, bool need_given, std::vector<uint64_t> &words, std::string &msg);
inline bool motif_is_auto(const char *motif) { return motif && std::strcmp(motif, "auto") == 0; }
// ... for an entry of the C ABI: the message goes to the caller's buffer
inline int prepare(const inq_call_args_t *a, Prepared &P, char *errbuf, size_t errcap, BedCache *bed_cache = nullptr) {
    std::string msg;
    const int rc = prepare(a, P, msg, bed_cache);
    if (rc != INQ_EXIT_OK) set_err(errbuf, errcap, msg);
    return rc;
}


// The device context is created on its own thread from the first instruction of the command: HIP start-up
// (0.1 - 0.3 s) is the longest fixed cost of a run and overlaps opening the BAM, the BED, the .bai and the
// first reads of the file.
//
// Every wait for that thread is BOUNDED (ctx_timeout_s(): 60 s, INQ_CTX_TIMEOUT_S overrides).  Round 4 lost a GPU box to the case it
// was not: a profiler's tool library aborted (glog FATAL -> SIGABRT) inside the runtime's first call, ON the context thread
// (gpurun_out/prof_cli_locus/p2.log: inq_ctx_create_early <- AsyncCtx::start), its signal handler then "finalized" there for ever, and
// the process stayed: the uploader polled `stage_ready` without end, the caller sat in SpanPipeline::next() behind it, and a join of the
// context thread would have sat there too.  Now the thread's state lives in a block it shares with its owner; whoever waits gives up
// after the time-out, the context counts as failed (INQ_ERR_HIP, "did not come up"), the thread is left behind (detached: it may
// be stuck inside a signal handler or the driver) and the call ends with INQ_EXIT_ERROR.
double ctx_timeout_s();
// A caller short of cores (its share of the granted cores below 8: eight ranks on a 16-core grant have 2 each) cannot afford the two
// cores that SPIN while a span inflates (the caller's thread in hipStreamSynchronize) and crosses the link (the uploader's in
// hipEventSynchronize): they are the readers' (measured with the process confined to 4 CPUs: tools/few_cores.sh).  The context is then
// made with blocking waits ("blocking_sync"), unless the user has set the option either way (--ctx-option, inq_default_option).
// sharers: 0 = local_share().
void choose_wait_mode(int sharers);
typedef int (*CtxCreateFn)(int device, inq_ctx_t **ctx, volatile int *stage_ready);
CtxCreateFn ctx_create_fn();  // inq_ctx_create_early, or what inq_host_test_ctx_creator put in its place (tests)
struct AsyncCtx {
    struct State {
        inq_ctx_t *ctx = nullptr;
        int hrc = INQ_OK;
        int numa_node = -1;
        std::atomic<bool> ready{false};  // ctx / hrc / numa_node are final
        // raised by inq_ctx_create_early as soon as spans may be STAGED on ctx (uploads, inflates), ~30 ms before the context is
        // complete: the uploader thread starts on the spans the loader has read by then
        volatile int stage_ready = 0;
        std::atomic<bool> gave_up{false};  // a waiter ran into the time-out: hrc is the waiter's verdict, the thread's result is ignored
        std::mutex mu;
        std::condition_variable cv;
    };
    std::shared_ptr<State> st = std::make_shared<State>();
    inq_ctx_t *&ctx = st->ctx;
    int &hrc = st->hrc;
    int &numa_node = st->numa_node;
    std::atomic<bool> &ready = st->ready;
    std::thread th;
    bool started = false;
    bool leak = false;  // set by the OWNER after a clean run when the process is about to end: the context is left to the operating system
    std::chrono::steady_clock::time_point t_start;
    AsyncCtx() = default;
    AsyncCtx(const AsyncCtx &) = delete;
    void start(int device, int sharers = 0) {
        t_start = std::chrono::steady_clock::now();
        started = true;
        choose_wait_mode(sharers);
        std::shared_ptr<State> s = st;  // the thread keeps the block alive, whatever becomes of this object
        CtxCreateFn create = ctx_create_fn();
        th = std::thread([s, device, create] {
            prefer_gpu_node_for_this_thread(device);  // what the runtime allocates while it starts
            const double a = stamp_ms();
            inq_ctx_t *c = nullptr;
            // (the early form publishes through these two words; they are read by wait_stage() only)
            const int rc = create(device, &s->ctx, &s->stage_ready);
            c = s->ctx;
            const int node = rc == INQ_OK ? inq_ctx_numa_node(c) : -1;
            {
                std::lock_guard<std::mutex> g(s->mu);
                if (!s->gave_up.load()) s->hrc = rc, s->numa_node = node;
                s->ready.store(true);
            }
            s->cv.notify_all();
            if (timing_level() == 2) std::fprintf(stderr, "[inq ctx] @%.1f device context ready (inq_ctx_create %.1f ms), GPU on NUMA node %d\n", stamp_ms(), stamp_ms() - a, node);
        });
    }
    // marks the context as failed because its thread did not finish in time; the thread is left to itself
    void give_up_locked() {
        if (st->gave_up.exchange(true)) return;
        st->hrc = INQ_ERR_HIP;
        st->numa_node = -1;
        if (th.joinable()) th.detach();
    }
    double seconds_left() const {
        return ctx_timeout_s() - std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    }
    // any thread: true once spans may be staged on ctx (false: the context could not be made, or not in time)
    bool wait_stage() {
        while (!__atomic_load_n(&st->stage_ready, __ATOMIC_ACQUIRE)) {
            if (ready.load()) return hrc == INQ_OK && !st->gave_up.load() && __atomic_load_n(&st->stage_ready, __ATOMIC_ACQUIRE) != 0;
            if (st->gave_up.load()) return false;
            if (seconds_left() <= 0) {
                std::lock_guard<std::mutex> g(st->mu);
                if (!ready.load()) give_up_locked();
                return false;
            }
            std::this_thread::sleep_for(std::chrono::microseconds(200));
        }
        return ctx != nullptr && !st->gave_up.load();
    }
    std::mutex join_mu;
    bool wait() {  // any thread: the context is complete (true) or there is none (false); never longer than the time-out
        if (!started) return false;
        {
            std::unique_lock<std::mutex> g(st->mu);
            while (!ready.load() && !st->gave_up.load()) {
                const double left = seconds_left();
                if (left <= 0) {
                    give_up_locked();
                    break;
                }
                st->cv.wait_for(g, std::chrono::duration<double>(std::min(left, 0.25)));
            }
        }
        std::lock_guard<std::mutex> g(join_mu);
        if (!st->gave_up.load() && th.joinable()) th.join();
        return hrc == INQ_OK && !st->gave_up.load();
    }
    bool timed_out() const { return st->gave_up.load(); }
    ~AsyncCtx() {
        if (started) (void)wait();
        // a context whose thread was given up on is never touched again (the thread may still be inside its constructor)
        if (!leak && !st->gave_up.load()) inq_ctx_destroy(ctx);
    }
};

}  // namespace inqhost

// a session: many BAMs on ONE device context (session.cc; a prepared run may be opened on one: run.cc inq_session_run_open)
struct inq_session {
    inqhost::AsyncCtx actx;
    inqhost::HostBufPool pool;
    inqhost::BedCache bed_cache;
    int32_t device = 0;
    uint64_t n_staged = 0;  // inq_session_stage: which of the two sets of device slots the next file takes
};

namespace inqhost {

// How many processes / device parts share this host's cores with the caller, and which of them it is: the reader pool of a span
// pipeline takes the granted cores (sched_getaffinity, cut by the cgroup's CPU quota) divided by that number, and binds its threads to
// L3 domains starting at a different one per sharer.  Default: LOCAL_WORLD_SIZE / LOCAL_RANK as torch.distributed.run exports them
// (one process per GPU), else 1 / 0; inq_host_set_local_share overrides; the one-process --devices entry passes its own per part.
int granted_cpus();
void local_share(int *sharers, int *index);
void set_local_share(int sharers, int index);
void set_ctx_creator_for_tests(CtxCreateFn f, long timeout_ms);  // f = nullptr: the real one; timeout_ms < 0: the default

// what a device part of a multi-device call reports (inq_part_stats_t of include/inquistr_host.h is filled from it)
struct PartStats {
    uint64_t spans = 0, comp_bytes = 0;
    double span_loop_s = 0, wait_loader_s = 0, device_calls_s = 0;
    int front = 0;  // 1 = host sweep, 2 = device spans
    int io_threads = 0;
};

void publish_last_stats(const PartStats &s);
PartStats last_stats();  // of the last call that ended in this process (any thread)

// the options of a call as the device takes them (an inq_batch_t through HostBatch::view, an inq_span_t through apply)
struct CallOptions {
    uint32_t minlen = 5, support = 3;
    bool unphased = false;
    CallOptions() = default;
    explicit CallOptions(const inq_call_args_t &a)
        : minlen(a.minlen), support((uint32_t)std::min<uint64_t>(a.support, 0xffffffffull)), unphased(a.unphased != 0) {}
    void apply(inq_span_t &sp) const { sp.minlen = minlen, sp.support = support, sp.unphased = unphased ? 1u : 0u; }
};

// what one call works on: the opened BAM (header + index), the targets it was asked for, the options
struct CallView {
    BamFile &bam;
    const std::vector<RepeatInterval> &targets;
    const std::string &sample;
    CallOptions opt;
};

// the per-read Calls of a call's targets: [k] = the records of target k's kept reads in file order (empty: no batch or span held it)
using ReadCallLists = std::vector<std::vector<inq_read_call_t>>;

// A byte run behind each of those records: one Rec per record, in the records' order, and the runs back to back, inq::run_bytes(rec)
// bytes each (csrc/run_bytes.h).  Who the reads are, for the read table: their origins and names; the bases behind them, for the read-seqs
// file: their slices (inq_read_seq_t) and packed bases.  Of one target ([k] of TargetReports), or of a whole device call (BatchRows)
template <class Rec> struct RecordRuns {
    std::vector<Rec> recs;
    std::vector<uint8_t> bytes;
    // this call's runs cut into the shares of its loci: locus j holds the records [kept_off[j], kept_off[j + 1])
    void cut(const std::vector<uint64_t> &kept_off, std::vector<RecordRuns> &loci) const {
        size_t at = 0;
        for (size_t j = 0; j + 1 < kept_off.size(); ++j) {
            RecordRuns &t = loci[j];
            t.recs.assign(recs.begin() + kept_off[j], recs.begin() + kept_off[j + 1]);
            size_t n = 0;
            for (const Rec &r : t.recs) n += inq::run_bytes(r);
            t.bytes.assign(bytes.begin() + at, bytes.begin() + at + n);
            at += n;
        }
    }
};
using ReadIdentities = RecordRuns<inq_read_origin_t>;
using ReadSlices = RecordRuns<inq_read_seq_t>;

// src[j] -> dst[index[j]]: rows and reports of a batch, a flush or a device part into their targets' places
template <class T>
inline void scatter(const T *src, const uint32_t *index, size_t n, T *dst) {
    for (size_t j = 0; j < n; ++j) dst[index[j]] = src[j];
}

// The per-target reports of a call, beside its rows: the tie report (inq_call_args_t::ties_path), the evidence file (::evidence_path), the
// read-calls file (inq_genotype_repeats_reads), the read table (inq_genotype_repeats_table; it needs the read-calls lists, which are
// then collected with it), the read-seqs file (inq_genotype_repeats_seqs; its lines name the reads: the table's lists are collected
// with it), the read-motifs file (inq_genotype_repeats_motifs; the runs are those of the bases: the slices are collected with it),
// the locus-motifs file (inq_genotype_repeats_locus_motifs; the motif each target's reads repeat, found in those same slices).  One value at every layer; a further report is one more member of each of the three
// structs, a line in begin / scatter_from, a row in write_rows' table and a pointer in BatchRows::call / flush.  A further per-read
// payload (a byte run behind each record, as the names and the bases are) is a record type with its inq::run_bytes(), one more
// RecordRuns in TargetReports and in BatchRows, and a ByteRuns in ReadStore (front_end.h) where the host sweep is to keep it.
struct ReportSet {  // which of them are collected: what is not adds nothing to the launch sequence
    bool ties = false, evidence = false, read_calls = false, read_table = false, read_seqs = false, read_motifs = false;
    bool locus_motifs = false;  // the motif each target's reads repeat is looked for
    bool motif_auto = false;    // ... and is what the read-motifs file measures with (`--motif auto`): no target has a given word
};
struct ReportFds {  // where a text call writes them, in the .inq's row order (-1: no file)
    int ties = -1, evidence = -1, read_calls = -1, read_table = -1, read_seqs = -1, read_motifs = -1, locus_motifs = -1;
    bool motif_auto = false;  // the read-motifs file measures with the motifs found in the reads (`--motif auto`)
    ReportSet wanted() const {  // (the motif runs are those of the bases, and so is the motif the reads repeat: the slices are collected with them)
        const bool found = locus_motifs >= 0 || (read_motifs >= 0 && motif_auto);
        const bool bases = read_seqs >= 0 || read_motifs >= 0 || found, who = read_table >= 0 || bases;
        return ReportSet{ties >= 0, evidence >= 0, read_calls >= 0 || who, who, bases, read_motifs >= 0, found, read_motifs >= 0 && motif_auto};
    }
};
// ... of a set of targets (a call's, a device part's, one device call's loci): [k] belongs to target k of the set.  A target no batch or
// span holds keeps what begin put there: no flag, zeros, an empty list.
struct TargetReports {
    ReportSet has;
    std::vector<uint8_t> ties;                   // INQ_LOCUS_TIE
    std::vector<inq_locus_evidence_t> evidence;
    ReadCallLists read_calls;                    // the records of the target's kept reads in file order
    std::vector<ReadIdentities> read_table;      // ... and who each of them is
    std::vector<ReadSlices> read_seqs;           // ... and the bases behind each Call
    std::vector<std::vector<inq_read_motif_t>> read_motifs;  // ... and the motif runs of those bases
    std::vector<inq_locus_motif_t> locus_motifs;             // the motif the target's kept reads repeat
    // what the runs are measured with and the found motifs are compared with, an INPUT: the targets' given motif words (inq_read_motif_t;
    // 0: none), set by whoever begins the reports
    std::vector<uint64_t> motif_word;
    // the word target k's read-motifs lines are printed under
    uint64_t printed_word(size_t k) const { return has.motif_auto ? locus_motifs[k].word : motif_word[k]; }
    void begin(size_t n, ReportSet which) {
        has = which;
        ties.assign(which.ties ? n : 0, 0);
        evidence.assign(which.evidence ? n : 0, inq_locus_evidence_t{});
        read_calls.assign(which.read_calls ? n : 0, std::vector<inq_read_call_t>());
        read_table.assign(which.read_table ? n : 0, ReadIdentities());
        read_seqs.assign(which.read_seqs ? n : 0, ReadSlices());
        read_motifs.assign(which.read_motifs ? n : 0, std::vector<inq_read_motif_t>());
        locus_motifs.assign(which.locus_motifs ? n : 0, inq_locus_motif_t{});
        motif_word.assign(which.read_motifs || which.locus_motifs ? n : 0, 0);
    }
    // what part collected (nothing this one does not), part's k-th -> target idx[k]; the lists are moved out of part
    void scatter_from(TargetReports &part, const uint32_t *idx, size_t n) {
        if (part.has.ties) scatter(part.ties.data(), idx, n, ties.data());
        if (part.has.evidence) scatter(part.evidence.data(), idx, n, evidence.data());
        if (part.has.read_calls)
            for (size_t k = 0; k < n; ++k) read_calls[idx[k]] = std::move(part.read_calls[k]);
        if (part.has.read_table)
            for (size_t k = 0; k < n; ++k) read_table[idx[k]] = std::move(part.read_table[k]);
        if (part.has.read_seqs)
            for (size_t k = 0; k < n; ++k) read_seqs[idx[k]] = std::move(part.read_seqs[k]);
        if (part.has.read_motifs)
            for (size_t k = 0; k < n; ++k) read_motifs[idx[k]] = std::move(part.read_motifs[k]);
        if (part.has.locus_motifs) scatter(part.locus_motifs.data(), idx, n, locus_motifs.data());
    }
};

// what a session adds to one call: a pipeline that was started ahead of it (its loader has been reading and uploading while the
// previous file was being called), the buffer pool, the set of device staging slots
struct SessionHooks {
    SpanPipeline *early_pipe = nullptr;
    HostBufPool *pool = nullptr;
    int slot_base = 0;
    int front = 0;  // 0 = decide here, 1 = host sweep, 2 = device spans (decided when the pipeline was started)
    int sharers = 0, share_index = 0;  // > 0: this call is one of `sharers` device parts of one process (else: local_share())
    PartStats *stats = nullptr;        // may be null
    // rows stay on the device (inq_run_rows_device): row of target k of the call -> dev_p1[k], dev_p2[k]
    double *dev_p1 = nullptr, *dev_p2 = nullptr;
    uint64_t dev_cap = 0;
    // the reports: of target k of the call -> (*reports)[k], begun by the caller with what it wants collected (null: the call collects
    // what report_fds asks for into one of its own); a text call writes each file whose fd is set
    TargetReports *reports = nullptr;
    ReportFds report_fds;
    // the motif words of the call's whole target list (the read-motifs file), [i] of target i of Prepared::targets; null: none has one
    const std::vector<uint64_t> *motif_words = nullptr;
    // the caller owns the context AND the process ends with this call (fast_exit()): a pipeline the call made itself is left to the
    // operating system after a clean run (unmapping a GB of touched pages takes ~0.1 s), as the caller then leaves its context
    bool process_is_leaving = false;
};

// a file a call writes beside its .inq (the tie report, the evidence file): opened (created / truncated) before any device work,
// closed with the call
struct ReportFile {
    int fd = -1;
    ReportFile() = default;
    ReportFile(const ReportFile &) = delete;
    ReportFile &operator=(const ReportFile &) = delete;
    ~ReportFile() {
        if (fd >= 0) ::close(fd);
    }
    // path may be null (no file): INQ_EXIT_OK; a path that cannot be opened: INQ_EXIT_ERROR and a message that names `what` and it
    int open(const char *path, const char *what, std::string &msg);
};
constexpr const char *kTiesWhat = "the tie report", *kEvidenceWhat = "the evidence file", *kReadCallsWhat = "the read-calls file",
                      *kReadTableWhat = "the read table", *kReadSeqsWhat = "the read-seqs file", *kReadMotifsWhat = "the read-motifs file",
                      *kLocusMotifsWhat = "the locus-motifs file";
// the paths of the files that are no field of inq_call_args_t (it does not grow): what the widest entry of the family takes
struct ReportPaths {
    const char *read_calls = nullptr, *read_table = nullptr, *read_seqs = nullptr, *read_motifs = nullptr;
    const char *motif = nullptr;  // one motif for every target of the read-motifs file (null: column 4 of the BED; `auto`: the found one)
    const char *locus_motifs = nullptr;
};
// the files of a text call (inq_call_args_t::ties_path, ::evidence_path; `more` of inq_genotype_repeats_motifs, else nulls)
struct CallReports {
    ReportFile ties, evidence, read_calls, read_table, read_seqs, read_motifs, locus_motifs;
    bool motif_auto = false;
    int open(const inq_call_args_t &a, const ReportPaths &more, std::string &msg) {
        int rc = ties.open(a.ties_path, kTiesWhat, msg);
        if (rc == INQ_EXIT_OK) rc = evidence.open(a.evidence_path, kEvidenceWhat, msg);
        if (rc == INQ_EXIT_OK) rc = read_calls.open(more.read_calls, kReadCallsWhat, msg);
        if (rc == INQ_EXIT_OK) rc = read_table.open(more.read_table, kReadTableWhat, msg);
        if (rc == INQ_EXIT_OK) rc = read_seqs.open(more.read_seqs, kReadSeqsWhat, msg);
        if (rc == INQ_EXIT_OK) rc = read_motifs.open(more.read_motifs, kReadMotifsWhat, msg);
        motif_auto = motif_is_auto(more.motif);
        return rc != INQ_EXIT_OK ? rc : locus_motifs.open(more.locus_motifs, kLocusMotifsWhat, msg);
    }
    ReportFds fds() const {
        return ReportFds{ties.fd, evidence.fd, read_calls.fd, read_table.fd, read_seqs.fd, read_motifs.fd, locus_motifs.fd, motif_auto};
    }
    void to(SessionHooks &hooks) const { hooks.report_fds = fds(); }
};
// an entry that returns rows or keeps its context for many files writes no evidence file and says so (INQ_EXIT_ERROR) instead of
// ignoring the request
inline int refuse_evidence(const inq_call_args_t *a, const char *who, std::string &msg) {
    if (!a || !a->evidence_path) return INQ_EXIT_OK;
    msg = std::string("--evidence (evidence_path) is not supported by ") + who + ": use inquistr call / inq_genotype_repeats";
    return INQ_EXIT_ERROR;
}

// rows instead of text: the targets named by idx[] (positions in the parsed target list) are called, their rows go to p1 / p2
struct RowsOut {
    const uint32_t *idx = nullptr;
    uint64_t n = 0;
    double *p1 = nullptr, *p2 = nullptr;  // host arrays (null when the rows stay on the device)
    bool active = false;
    double *d1 = nullptr, *d2 = nullptr;  // DEVICE arrays of dcap entries on the call's device: the rows are left there
    uint64_t dcap = 0;
};

// what write_rows writes beside the .inq, each where it was collected and its fd is set, for the same rows in the same order
struct RowReports {
    const TargetReports *reports = nullptr;
    ReportFds fds;
    bool unphased = false;  // how the read-calls file splits a target's Calls
};

// the result buffers of one device call over n loci (rows start as NaN), its reports, and their way into the call's arrays
struct BatchRows {
    std::vector<double> b1, b2;
    inq_result_t res;
    TargetReports rep;                // of the call's loci, in the call's order
    std::vector<uint64_t> bk;         // kept_off of the per-read Calls
    std::vector<inq_read_call_t> bc;  // ... and the records, fetched behind the call
    // the read table: the records' origins and names, fetched with them (a flush) or looked up in the batch the host owns (a call); the
    // read-seqs file: their slices and packed bases, fetched (a flush) or cut out of the batch's SEQ (a call)
    ReadIdentities who;
    ReadSlices bases;
    // the read-motifs file: the loci's given motif words (motifs_of; none where the found ones are measured with) and a record per
    // record, fetched (a flush) or walked here (a call); the locus-motifs file: a record per locus in rep, likewise
    std::vector<uint64_t> words;
    std::vector<inq_read_motif_t> runs;
    void begin(size_t n, ReportSet which) {
        b1.assign(n, NAN), b2.assign(n, NAN);
        std::memset(&res, 0, sizeof res);
        res.phase1 = b1.data(), res.phase2 = b2.data();
        rep.begin(n, which);
        if (which.read_calls) bk.assign(n + 1, 0);
    }
    // the motif words of the call's loci, locus j being target index[j] of `all`; behind begin
    void motifs_of(const uint32_t *index, const TargetReports &all) {
        words.clear();
        if (!rep.has.read_motifs || rep.has.motif_auto) return;
        words.resize(b1.size());
        for (size_t j = 0; j < words.size(); ++j) words[j] = index[j] < all.motif_word.size() ? all.motif_word[index[j]] : 0;
    }
    // the records' runs cut into the loci's lists
    void cut_runs() {
        for (size_t j = 0; j + 1 < bk.size(); ++j) rep.read_motifs[j].assign(runs.begin() + bk[j], runs.begin() + bk[j + 1]);
    }
    // what the device call takes (null: not collected)
    uint8_t *flags() { return rep.has.ties ? rep.ties.data() : nullptr; }
    inq_locus_evidence_t *evidence() { return rep.has.evidence ? rep.evidence.data() : nullptr; }
    uint64_t *kept_off() { return rep.has.read_calls ? bk.data() : nullptr; }
    const uint64_t *given() const { return words.empty() ? nullptr : words.data(); }
    inq_locus_motif_t *found() { return rep.has.locus_motifs ? rep.locus_motifs.data() : nullptr; }
    // the host-buffer call / the flush of the n deferred loci with what begin asked for, the lists fetched behind it.  The read table:
    // `read` indexes a batch the host owns (owner: the sweep's batch with its names), or one that exists on the device only, whose
    // flush gathers origins and names there (the spans were appended with names)
    int call(inq_ctx_t *ctx, const inq_batch_t &batch, const HostBatch *owner = nullptr) {
        int rc = inq_call_batch_reads(ctx, &batch, &res, flags(), evidence(), kept_off());
        if (rc == INQ_OK) rc = fetch_read_calls(ctx);
        if (rc != INQ_OK || !rep.has.read_table) return rc;
        if (!owner || owner->names.off.size() != owner->reads.size() + 1) return INQ_ERR_ARG;
        who.recs.resize(bc.size());
        who.bytes.clear();
        for (size_t k = 0; k < bc.size(); ++k) {
            const uint32_t r = bc[k].read;  // (the call succeeded: every index lies inside the batch)
            const inq_read_t &rd = owner->reads[r];
            const uint64_t at = owner->names.off[r], len = owner->names.off[r + 1] - at;
            who.recs[k] = inq_read_origin_t{rd.pos, rd.mapq, rd.bits, (uint16_t)len};
            who.bytes.insert(who.bytes.end(), owner->names.bytes.begin() + at, owner->names.bytes.begin() + at + len);
        }
        who.cut(bk, rep.read_table);
        if (!rep.has.read_seqs) return INQ_OK;
        // the slices: record k of locus j is read bc[k].read under j's window, cut out of the SEQ the sweep kept (inq_host_seq_window)
        if (owner->seqs.off.size() != owner->reads.size() + 1 || owner->l_seq.size() != owner->reads.size()) return INQ_ERR_ARG;
        bases.recs.resize(bc.size());
        bases.bytes.clear();
        for (size_t j = 0; j + 1 < bk.size(); ++j)
            for (uint64_t k = bk[j]; k < bk[j + 1]; ++k) {
                const uint32_t r = bc[k].read;
                const inq_read_t &rd = owner->reads[r];
                inq_read_seq_t &q = bases.recs[k];
                seq_window(owner->cigar.data() + (size_t)rd.cigar_off4 * 4, rd.n_cigar, rd.pos, owner->l_seq[r], batch.locus_start[j],
                           batch.locus_end[j], &q.q_beg, &q.n_bases);
                pack_seq_slice(owner->seqs.bytes.data() + owner->seqs.off[r], q.q_beg, q.n_bases, bases.bytes);
            }
        bases.cut(bk, rep.read_seqs);
        if (!rep.has.read_motifs && !rep.has.locus_motifs) return INQ_OK;
        // the motif each locus's slices repeat (inq_host_locus_motif_find), then the runs: a sequential walk of each slice under its
        // locus's word (inq_host_motif_runs), the given one or, where there is none, the found one
        if (!words.empty() && words.size() + 1 != bk.size()) return INQ_ERR_ARG;
        if (rep.has.read_motifs) runs.resize(bc.size());
        std::vector<uint32_t> lens;
        size_t at = 0;
        for (size_t j = 0; j + 1 < bk.size(); ++j) {
            uint64_t word = words.empty() ? 0 : words[j];
            if (rep.has.locus_motifs) {
                lens.clear();
                for (uint64_t k = bk[j]; k < bk[j + 1]; ++k) lens.push_back(bases.recs[k].n_bases);
                locus_motif_find(bases.bytes.data() + at, lens.data(), lens.size(), &rep.locus_motifs[j]);
                word = motif_word_in_use(word, rep.locus_motifs[j].word);
            }
            for (uint64_t k = bk[j]; k < bk[j + 1]; ++k) {
                if (rep.has.read_motifs) motif_runs(bases.bytes.data() + at, bases.recs[k].n_bases, word, &runs[k]);
                at += inq::run_bytes(bases.recs[k]);
            }
        }
        if (rep.has.read_motifs) cut_runs();
        return INQ_OK;
    }
    int flush(inq_ctx_t *ctx, uint64_t n, double *ms_call) {
        if (!rep.has.read_table) {
            const int rc = inq_call_flush_reads(ctx, &res, n, ms_call, flags(), evidence(), kept_off());
            return rc != INQ_OK ? rc : fetch_read_calls(ctx);
        }
        uint64_t name_bytes = 0, seq_bytes = 0;
        if (!words.empty() && words.size() != n) return INQ_ERR_ARG;
        int rc = inq_call_flush_locus_motifs(ctx, &res, n, ms_call, flags(), evidence(), kept_off(), &name_bytes,
                                             rep.has.read_seqs ? &seq_bytes : nullptr, given(), found());
        if (rc == INQ_OK) rc = fetch_read_calls(ctx);
        if (rc != INQ_OK) return rc;
        who.recs.resize(bc.size()), who.bytes.resize(name_bytes);
        if ((rc = inq_read_origins_fetch(ctx, who.recs.data(), who.recs.size(), who.bytes.data(), who.bytes.size())) != INQ_OK) return rc;
        who.cut(bk, rep.read_table);
        if (!rep.has.read_seqs) return INQ_OK;
        bases.recs.resize(bc.size()), bases.bytes.resize(seq_bytes);
        if ((rc = inq_read_seqs_fetch(ctx, bases.recs.data(), bases.recs.size(), bases.bytes.data(), bases.bytes.size())) != INQ_OK) return rc;
        bases.cut(bk, rep.read_seqs);
        if (!rep.has.read_motifs) return INQ_OK;
        runs.resize(bc.size());
        if ((rc = inq_read_motifs_fetch(ctx, runs.data(), runs.size())) != INQ_OK) return rc;
        cut_runs();
        return INQ_OK;
    }
    // the records behind a call that filled kept_off, out of the context's scratch, cut into the loci's lists
    int fetch_read_calls(inq_ctx_t *ctx) {
        if (!rep.has.read_calls) return INQ_OK;
        bc.resize(bk.back());
        const int rc = inq_read_calls_fetch(ctx, bc.data(), bc.size());
        for (size_t j = 0; rc == INQ_OK && j + 1 < bk.size(); ++j) rep.read_calls[j].assign(bc.begin() + bk[j], bc.begin() + bk[j + 1]);
        return rc;
    }
    // p1 null: the rows went elsewhere (device memory)
    void scatter_to(const uint32_t *index, double *p1, double *p2, TargetReports *out) {
        if (p1) scatter(b1.data(), index, b1.size(), p1), scatter(b2.data(), index, b2.size(), p2);
        out->scatter_from(rep, index, b1.size());
    }
};

// a device call that returned rc != INQ_OK: "device call failed: <inq_strerror>" (+ the runtime's own text for INQ_ERR_HIP, + suffix)
// goes to errbuf; returns the exit status - domain errors are the reference's panics (HP > 2, bad CIGAR op, ...)
int device_call_failed(int rc, inq_ctx_t *ctx, char *errbuf, size_t errcap, const std::string &suffix = std::string());

bool use_device_front(const inq_call_args_t *args, const BamFile &bam, const std::vector<RepeatInterval> &targets);
std::string ctx_failure_message(AsyncCtx &actx);
int span_io_threads(const inq_call_args_t *args, int sharers);
SpanPipeline *start_span_pipeline(const inq_call_args_t *args, const BamFile &bam, const std::vector<RepeatInterval> &targets, AsyncCtx &actx,
                                  int slot_base, HostBufPool *pool, int sharers = 0, int share_index = 0);
int run_device_front(const inq_call_args_t *args, const CallView &V, AsyncCtx &actx, std::vector<double> &p1, std::vector<double> &p2,
                     char *errbuf, size_t errcap, double *t_front, double *t_dev, const SessionHooks &hooks = SessionHooks());
int genotype_prepared(const inq_call_args_t *args, AsyncCtx &actx, Prepared &P, int out_fd, char *errbuf, size_t errcap, const RowsOut &rows,
                      std::chrono::steady_clock::time_point t_start, const SessionHooks &hooks = SessionHooks());
// reports: the tie report, the evidence file and the read-calls file of the same rows, in the same order
int write_rows(uint64_t threads, const std::vector<RepeatInterval> &targets, const std::string &sample, const double *p1, const double *p2,
               int out_fd, char *errbuf, size_t errcap, const RowReports &reports = RowReports());
// the order of the .inq's rows: BED order for -t 1, (human_compare(chrom), start) for -t >= 2 (src/call.rs:33-38,141)
std::vector<uint32_t> row_order(uint64_t threads, const std::vector<RepeatInterval> &targets);
// One file beside the .inq: `header` (may be empty), then what row(text, i) appends for every target i = order[k] - its line, or nothing -,
// written in pieces of 8 MB (deep loci make long lines).  what: the file's name in "Failed writing <what>."
using ReportRow = std::function<void(std::string &text, uint32_t i)>;
int write_report(const std::vector<uint32_t> &order, const std::string &header, const ReportRow &row, const char *what, int fd, char *errbuf,
                 size_t errcap);
// the tie report: `chrom\tbegin\tend\n` for every target order[k] with a flag set (no header)
int write_ties(const std::vector<uint32_t> &order, const std::vector<RepeatInterval> &targets, const uint8_t *ties, int fd, char *errbuf,
               size_t errcap);
// inq_genotype_repeats with the read-calls file, the read table, the read-seqs, the read-motifs and the locus-motifs file (null: none), for
// inq_genotype_repeats_locus_motifs
int genotype_single(const inq_call_args_t *args, int out_fd, const ReportPaths &more, char *errbuf, size_t errcap);
int partition_prepared(Prepared &P, uint64_t world, uint32_t *order, uint64_t *cuts);

struct OwnedArgs {
    inq_call_args_t a;
    std::string bam, region, region_file, sample_name, reference, ties_path, evidence_path;
    explicit OwnedArgs(const inq_call_args_t &src) : a(src) {
        auto own = [](const char *&p, std::string &keep) {
            if (p) keep = p, p = keep.c_str();
        };
        own(a.bam, bam), own(a.region, region), own(a.region_file, region_file), own(a.sample_name, sample_name), own(a.reference, reference);
        own(a.ties_path, ties_path), own(a.evidence_path, evidence_path);
    }
    OwnedArgs(const OwnedArgs &) = delete;
};

}  // namespace inqhost
