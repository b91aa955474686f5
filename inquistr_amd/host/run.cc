// run.cc - `call::genotype_repeats` (src/call.rs:76-159) on top of the front ends and the HIP library: the prepared call, the host-sweep
// loop, the output stage, and the entry points of include/inquistr_host.h that run one call (text or rows), split it, or hold it open.
#include "driver_internal.h"

using namespace inqhost;

namespace inqhost {


int prepare(const inq_call_args_t *a, Prepared &P, std::string &msg, BedCache *bed_cache) {
    if (!a || !a->bam) {
        msg = "no BAM given";
        return INQ_EXIT_ERROR;
    }
    const std::string bamp = a->bam;
    const bool remote = starts_with(bamp, "s3") || starts_with(bamp, "https://");
    if (!is_file(bamp) && !remote) {  // :87-90
        msg = "ERROR: path to bam file " + bamp + " is not valid!";
        return INQ_EXIT_ERROR;
    }
    if (remote) {  // :227-240 needs libcurl + htslib network code: not in this build
        msg = "remote inputs (s3://, https://) are not supported by this build";
        return INQ_EXIT_ERROR;
    }
    if (ends_with(bamp, ".cram")) {  // :245-259 needs htslib's CRAM codecs: not in this build
        msg = "CRAM input is not supported by this build (BAM + .bai only)";
        return INQ_EXIT_ERROR;
    }
    P.sample = a->sample_name ? std::string(a->sample_name) : sample_name_from_path(bamp);  // :91-100
    // get_chrom_lengths_from_bam_header opens the BAM before the target arguments are looked at (:187)
    const auto t_open = Clock::now();
    P.bam.reset(new BamFile(1));  // header + index; with -t > 1 every sweep worker opens its own reader
    std::string e;
    if (!P.bam->open(bamp, &e)) {
        msg = "Error opening local BAM: " + e;  // :242-243
        return INQ_EXIT_PANIC;
    }
    auto lengths = P.bam->sq_lengths(&e);
    if (!e.empty()) {
        msg = e;
        return INQ_EXIT_PANIC;
    }
    const auto t_targets = Clock::now();
    TargetsResult tr;
    if (a->region && !a->region_file)
        tr = targets_from_string(a->region, lengths);  // :190
    else if (!a->region && a->region_file) {
        struct stat sb;
        const bool have_stat = bed_cache && ::stat(a->region_file, &sb) == 0;
        BedKey key;
        if (have_stat)
            key = BedKey{a->region_file, (uint64_t)sb.st_dev, (uint64_t)sb.st_ino, (uint64_t)sb.st_size,
                         (int64_t)sb.st_mtim.tv_sec * 1000000000ll + sb.st_mtim.tv_nsec, lengths};
        bool hit = false;
        if (have_stat) {
            std::lock_guard<std::mutex> lk(bed_cache->mu);
            hit = bed_cache->valid && bed_cache->key == key;
            if (hit) tr = bed_cache->tr;
        }
        if (!hit) {
            tr = targets_from_bed(a->region_file, lengths);  // :192-195
            if (have_stat) {
                std::lock_guard<std::mutex> lk(bed_cache->mu);
                bed_cache->key = std::move(key), bed_cache->tr = tr, bed_cache->valid = true;
            }
        }
    } else {
        msg = "ERROR: Specify a region string (-r) or a region_file (-R)!";  // :197-200
        return INQ_EXIT_ERROR;
    }
    if (tr.panicked) {
        msg = tr.message;
        return INQ_EXIT_PANIC;
    }
    for (const auto &t : tr.data) {
        if (t.start < 10) {  // src/call.rs:285,335: `repeat.start - 10` underflows u32 -> fetch fails -> expect() panics
            msg = "Failed to fetch region (" + t.chrom + ":" + std::to_string(t.start) + "-" + std::to_string(t.end) +
                  ": start - 10 underflows)";
            return INQ_EXIT_PANIC;
        }
    }
    P.targets.swap(tr.data);
    P.target_name.swap(tr.name);
    if (timing_level() == 2)
        std::fprintf(stderr, "[inq prepare] header + index %.2f ms, targets (%zu) %.2f ms\n", ms(t_open, t_targets), P.targets.size(),
                     ms(t_targets, Clock::now()));
    return INQ_EXIT_OK;
}

int target_motif_words(const Prepared &P, const char *motif, bool need_given, std::vector<uint64_t> &words, std::string &msg) {
    const size_t n = P.targets.size();
    words.assign(n, 0);
    if (motif_is_auto(motif)) motif = nullptr;  // (the found motifs are measured with: what is left to tell is what the catalogue says)
    if (motif) {  // one motif for every target; it overrides column 4
        uint64_t w = 0;
        if (motif_encode(motif, &w) != kMotifOk) {
            msg = std::string("--motif ") + motif + ": not a motif of 1 to 15 bases of ACGT";
            return INQ_EXIT_ERROR;
        }
        words.assign(n, w);
        return INQ_EXIT_OK;
    }
    if (P.target_name.size() != n) {  // a BED of three columns, or a region string
        if (!need_given) return INQ_EXIT_OK;
        msg = "the read-motifs file needs a motif for every target: column 4 of the BED, or --motif <STR> (needed with -r)";
        return INQ_EXIT_ERROR;
    }
    size_t bad = 0;
    for (size_t i = 0; i < n; ++i) bad += motif_encode(P.target_name[i].c_str(), &words[i]) != kMotifOk;
    if (bad && need_given)
        std::fprintf(stderr, "%zu of %zu targets have no motif of 1 to 15 bases of ACGT in column 4: `.` in the read-motifs file\n", bad, n);
    return INQ_EXIT_OK;
}

int ReportFile::open(const char *path, const char *what, std::string &msg) {
    if (!path) return INQ_EXIT_OK;
    fd = ::open(path, O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
    if (fd >= 0) return INQ_EXIT_OK;
    msg = std::string("cannot write ") + what + " " + path + ": " + std::strerror(errno);
    return INQ_EXIT_ERROR;
}

int device_call_failed(int rc, inq_ctx_t *ctx, char *errbuf, size_t errcap, const std::string &suffix) {
    std::string m = std::string("device call failed: ") + inq_strerror(rc);
    if (rc == INQ_ERR_HIP) m += std::string(" [") + inq_last_error(ctx) + "]";
    set_err(errbuf, errcap, m + suffix);
    return (rc == INQ_ERR_HIP || rc == INQ_ERR_NOMEM || rc == INQ_ERR_NO_DEVICE) ? INQ_EXIT_ERROR : INQ_EXIT_PANIC;
}

// the call on an opened BAM + parsed targets, on a device context that may outlive it (a session calls many BAMs on one)
int genotype_prepared(const inq_call_args_t *args, AsyncCtx &actx, Prepared &P, int out_fd, char *errbuf, size_t errcap,
                             const RowsOut &rows, Clock::time_point t_start, const SessionHooks &hooks) {
    const int timing = timing_level();
    double t_front = 0, t_dev = 0;
    std::vector<RepeatInterval> sub;
    if (rows.active) {  // this caller's share of the targets (one process per GPU: inquistr_amd/call_dist.py)
        sub.reserve(rows.n);
        for (uint64_t k = 0; k < rows.n; ++k) {
            if (rows.idx[k] >= P.targets.size()) {
                set_err(errbuf, errcap, "target index outside the target list");
                return INQ_EXIT_ERROR;
            }
            sub.push_back(P.targets[rows.idx[k]]);
        }
    }
    const CallView V{*P.bam, rows.active ? sub : P.targets, P.sample, CallOptions(*args)};
    const size_t n = V.targets.size();
    std::vector<double> p1(n, NAN), p2(n, NAN);
    // the reports, collected only where someone asked for them (the locus kernels run without flags otherwise, and so on)
    TargetReports own_reports;
    if (!hooks.reports) own_reports.begin(n, hooks.report_fds.wanted());
    TargetReports *const reports = hooks.reports ? hooks.reports : &own_reports;
    if ((reports->has.read_motifs || reports->has.locus_motifs) && hooks.motif_words)  // the words of this call's targets, as p1 / p2 are indexed
        for (size_t k = 0; k < n; ++k) {
            const size_t i = rows.active ? rows.idx[k] : k;
            reports->motif_word[k] = i < hooks.motif_words->size() ? (*hooks.motif_words)[i] : 0;
        }
    const bool rows_on_device = rows.active && rows.d1 && rows.d2;
    if (rows_on_device && rows.dcap < n) {
        set_err(errbuf, errcap, "device row arrays smaller than the target list");
        return INQ_EXIT_ERROR;
    }
    auto emit = [&]() -> int {
        if (!rows.active)
            return write_rows(args->threads, V.targets, V.sample, p1.data(), p2.data(), out_fd, errbuf, errcap,
                              RowReports{reports, hooks.report_fds, V.opt.unphased});
        if (rows_on_device) return INQ_EXIT_OK;  // (device front end: they are there; host sweep: written below)
        if (n) std::memcpy(rows.p1, p1.data(), n * sizeof(double)), std::memcpy(rows.p2, p2.data(), n * sizeof(double));
        return INQ_EXIT_OK;
    };

    const auto t_open = Clock::now();
    const bool device_front = hooks.front ? hooks.front == 2 : use_device_front(args, V.bam, V.targets);
    // what the call did, for whoever asks afterwards (a device part's inq_part_stats_t, inq_host_last_call_stats)
    PartStats local_stats;
    PartStats *ps = hooks.stats ? hooks.stats : &local_stats;
    struct Publish {
        PartStats *p;
        ~Publish() { publish_last_stats(*p); }
    } publish{ps};
    ps->front = device_front ? 2 : 1;
    if (device_front) {
        const auto t_choice = Clock::now();
        SessionHooks dh = hooks;
        dh.stats = ps;
        if (rows_on_device) dh.dev_p1 = rows.d1, dh.dev_p2 = rows.d2, dh.dev_cap = rows.dcap;
        dh.reports = reports;  // (indexed like p1 / p2)
        int drc = run_device_front(args, V, actx, p1, p2, errbuf, errcap, &t_front, &t_dev, dh);
        if (drc != INQ_EXIT_OK) return drc;
        const auto t_run = Clock::now();
        drc = emit();
        if (timing)
            std::fprintf(stderr,
                         "[inq timing] device front end: open+targets %.3fs  front-end choice %.3fs  spans %.3fs (waiting for the loader "
                         "%.3fs, device calls %.3fs)  output %.3fs  total %.3fs\n",
                         secs(t_start, t_open), secs(t_open, t_choice), secs(t_choice, t_run), t_front, t_dev, secs(t_run, Clock::now()),
                         secs(t_start, Clock::now()));
        return drc;
    }

    auto t_prep = Clock::now();
    inq_ctx_t *&ctx = actx.ctx;
    int &hrc = actx.hrc;
    bool ctx_ready = false;
    auto need_ctx = [&]() -> bool {
        if (!ctx_ready) {
            actx.wait();
            ctx_ready = true;
        }
        if (hrc != INQ_OK) {
            set_err(errbuf, errcap, ctx_failure_message(actx));
            return false;
        }
        return true;
    };

    // -t N: N-1 sweep workers + this thread (which feeds the GPU and spins in the HIP runtime while waiting)
    // pinned staging: the device copies come from page-locked memory this thread fills, never from the
    // workers' pageable vectors (on-the-fly pinning contends with their page faults: 25 ms stalls)
    struct Pinned {
        void *p = nullptr;
        size_t cap = 0;
        ~Pinned() { inq_free_pinned(p); }
        void *fit(size_t bytes) {
            if (bytes > cap) {
                inq_free_pinned(p);
                p = nullptr;
                cap = bytes + bytes / 2 + (1u << 20);
                if (inq_alloc_pinned(cap, &p) != INQ_OK) p = nullptr, cap = 0;
            }
            return p;
        }
    } pin;
    const int n_workers = (int)std::max<uint64_t>(1, std::min<uint64_t>(args->threads > 1 ? args->threads - 1 : 1, 64));
    ParallelFrontEnd pfe(args->bam, V.bam, V.targets, V.opt.unphased, n_workers, 0, reports->has.read_table, reports->has.read_seqs);
    auto t_ctx = Clock::now();
    BatchRows br;
    for (;;) {
        ParallelFrontEnd::Item item;
        std::string ferr;
        bool fpanic = false;
        auto ta = Clock::now();
        int nb = pfe.next(item, &ferr, &fpanic);
        auto tb = Clock::now();
        t_front += secs(ta, tb);
        if (nb < 0) {
            set_err(errbuf, errcap, ferr);
            return INQ_EXIT_PANIC;  // read errors are expect()/unwrap() panics in the reference (:294,346)
        }
        if (nb == 0) break;
        if (!need_ctx()) return INQ_EXIT_ERROR;
        inq_batch_t batch;
        item.batch.view(&batch, V.opt.minlen, V.opt.support, V.opt.unphased);
        {
            auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
            const size_t s0 = al(batch.n_cigar_words * 4), s1 = al(batch.n_reads * sizeof(inq_read_t)),
                         s2 = al(batch.n_pairs * 4), s3 = al((batch.n_loci + 1) * 8), s4 = al(batch.n_loci * 4);
            char *base = (char *)pin.fit(s0 + s1 + s2 + s3 + 2 * s4);
            if (!base) {
                set_err(errbuf, errcap, "cannot allocate pinned host memory");
                return INQ_EXIT_ERROR;
            }
            auto put = [&](const void *src, size_t bytes, size_t &off, size_t slot) {
                void *dst = base + off;
                if (bytes) std::memcpy(dst, src, bytes);
                off += slot;
                return dst;
            };
            size_t off = 0;
            batch.cigar = (const uint32_t *)put(batch.cigar, batch.n_cigar_words * 4, off, s0);
            batch.reads = (const inq_read_t *)put(batch.reads, batch.n_reads * sizeof(inq_read_t), off, s1);
            batch.pair_read = (const uint32_t *)put(batch.pair_read, batch.n_pairs * 4, off, s2);
            batch.locus_pair_off = (const uint64_t *)put(batch.locus_pair_off, (batch.n_loci + 1) * 8, off, s3);
            batch.locus_start = (const uint32_t *)put(batch.locus_start, batch.n_loci * 4, off, s4);
            batch.locus_end = (const uint32_t *)put(batch.locus_end, batch.n_loci * 4, off, s4);
        }
        br.begin(batch.n_loci, reports->has);
        br.motifs_of(item.index.data(), *reports);
        auto tc = Clock::now();
        const int rc2 = br.call(ctx, batch, &item.batch);
        t_dev += secs(tb, Clock::now());
        if (timing == 2)
            std::fprintf(stderr, "[inq batch] loci %llu pairs %llu cigar %.1f MB  wait-ctx %.2f ms  call %.2f ms\n",
                         (unsigned long long)batch.n_loci, (unsigned long long)batch.n_pairs, batch.n_cigar_words * 4 / 1e6,
                         secs(tb, tc) * 1e3, secs(tc, Clock::now()) * 1e3);
        if (rc2 != INQ_OK) return device_call_failed(rc2, ctx, errbuf, errcap);
        br.scatter_to(item.index.data(), p1.data(), p2.data(), reports);
        pfe.recycle(std::move(item));
    }
    if (!need_ctx()) return INQ_EXIT_ERROR;  // no GPU is an error even for an empty target list
    if (rows_on_device && n) {  // the sweep's rows came back batch by batch (small inputs): one copy up
        if (inq_dev_write_rows(ctx, rows.d1, p1.data(), n) != INQ_OK || inq_dev_write_rows(ctx, rows.d2, p2.data(), n) != INQ_OK) {
            set_err(errbuf, errcap, std::string("device call failed: ") + inq_last_error(ctx));
            return INQ_EXIT_ERROR;
        }
    }

    {
        int wrc = emit();
        if (wrc != INQ_EXIT_OK) return wrc;
    }
    if (timing)
        std::fprintf(stderr, "[inq timing] open+targets %.3fs  hip ctx %.3fs  front end %.3fs  device calls %.3fs  total %.3fs\n",
                     secs(t_start, t_prep), secs(t_prep, t_ctx), t_front, t_dev, secs(t_start, Clock::now()));
    return INQ_EXIT_OK;
}


static std::mutex g_last_mu;
static PartStats g_last_stats;
void publish_last_stats(const PartStats &s) {
    std::lock_guard<std::mutex> g(g_last_mu);
    g_last_stats = s;
}
PartStats last_stats() {
    std::lock_guard<std::mutex> g(g_last_mu);
    return g_last_stats;
}

std::vector<uint32_t> row_order(uint64_t threads, const std::vector<RepeatInterval> &targets) {
    const size_t n = targets.size();
    std::vector<uint32_t> order(n);
    for (size_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
    if (threads > 1) {
        // genotypes_vec.sort_unstable() with Ord = (human_compare(chrom), start), :33-38,141.  Equal keys
        // are in completion order in the reference (nondeterministic); BED order is kept here.
        // The contig names are ranked once (a BED has few distinct ones), the rows sorted on integers.
        std::map<std::string, uint32_t> rank;
        for (size_t i = 0; i < n; ++i)
            if (i == 0 || targets[i].chrom != targets[i - 1].chrom) rank.emplace(targets[i].chrom, 0u);
        std::vector<const std::string *> names;
        for (auto &kv : rank) names.push_back(&kv.first);
        std::stable_sort(names.begin(), names.end(), [](const std::string *a, const std::string *b) { return human_compare(*a, *b) < 0; });
        for (size_t i = 0, r = 0; i < names.size(); ++i) {
            if (i && human_compare(*names[i - 1], *names[i]) != 0) ++r;  // names that compare equal share a rank
            rank[*names[i]] = (uint32_t)r;
        }
        std::vector<uint64_t> key(n);
        const std::string *last = nullptr;  // neighbouring targets mostly share the contig: one map lookup per run of them
        uint32_t last_rank = 0;
        for (size_t i = 0; i < n; ++i) {
            if (!last || *last != targets[i].chrom) last = &targets[i].chrom, last_rank = rank[*last];
            key[i] = ((uint64_t)last_rank << 32) | targets[i].start;
        }
        if (!std::is_sorted(key.begin(), key.end())) {
            // stable LSD radix sort of the row numbers on the 64-bit key, 16 bits a pass; digits all keys share are skipped
            // (a BED has few contigs and starts below 2^28: two or three passes instead of n log n compares)
            uint64_t all_or = 0, all_and = ~0ull;
            for (uint64_t k : key) all_or |= k, all_and &= k;
            std::vector<uint32_t> tmp(n);
            std::vector<uint32_t> cnt(65536);
            for (int shift = 0; shift < 64; shift += 16) {
                if ((((all_or ^ all_and) >> shift) & 0xffffu) == 0) continue;
                std::fill(cnt.begin(), cnt.end(), 0u);
                for (size_t i = 0; i < n; ++i) ++cnt[(key[order[i]] >> shift) & 0xffffu];
                uint32_t run = 0;
                for (auto &c : cnt) {
                    const uint32_t v = c;
                    c = run;
                    run += v;
                }
                for (size_t i = 0; i < n; ++i) tmp[cnt[(key[order[i]] >> shift) & 0xffffu]++] = order[i];
                order.swap(tmp);
            }
        }
    }
    return order;
}

int write_report(const std::vector<uint32_t> &order, const std::string &header, const ReportRow &row, const char *what, int fd, char *errbuf,
                 size_t errcap) {
    std::string text = header;
    bool ok = true;
    for (size_t k = 0; k < order.size() && ok; ++k) {
        row(text, order[k]);
        if (text.size() >= (8u << 20)) ok = write_all(fd, text), text.clear();
    }
    if (!ok || !write_all(fd, text)) {
        set_err(errbuf, errcap, std::string("Failed writing ") + what + ".");
        return INQ_EXIT_ERROR;
    }
    return INQ_EXIT_OK;
}

static ReportRow tie_row(const std::vector<RepeatInterval> &targets, const uint8_t *ties) {
    return [&targets, ties](std::string &text, uint32_t i) {
        const RepeatInterval &t = targets[i];
        if (ties[i] & INQ_LOCUS_TIE) text += t.chrom + '\t' + std::to_string(t.start) + '\t' + std::to_string(t.end) + '\n';
    };
}

int write_ties(const std::vector<uint32_t> &order, const std::vector<RepeatInterval> &targets, const uint8_t *ties, int fd, char *errbuf,
               size_t errcap) {
    return write_report(order, std::string(), tie_row(targets, ties), kTiesWhat, fd, errbuf, errcap);
}

int write_rows(uint64_t threads, const std::vector<RepeatInterval> &targets, const std::string &sample, const double *p1,
                      const double *p2, int out_fd, char *errbuf, size_t errcap, const RowReports &reports) {
    const size_t n = targets.size();
    const auto t_w0 = Clock::now();
    const std::vector<uint32_t> order = row_order(threads, targets);
    const auto t_w1 = Clock::now();
    // the text: rows formatted by a few threads into their own stretches of one buffer (sized from an upper bound per row,
    // written through a bare pointer: no per-character capacity checks), written in order.  Four threads at most: 500 000
    // rows are 17 MB of text, ~20 ms on one core, and starting a thread costs up to 2 ms on virtualised hosts.
    const size_t n_parts = n < 65536 ? 1 : std::min<size_t>(4, std::max(1u, std::thread::hardware_concurrency()));
    const std::string header = format_header(sample) + "\n";
    std::vector<size_t> part_off(n_parts + 1, 0), part_len(n_parts, 0);
    auto value_bound = [](double v) -> size_t { return std::fabs(v) < 9007199254740992.0 || std::isnan(v) ? 20 : 330; };
    for (size_t k = 0; k < n_parts; ++k) {
        const size_t lo = n * k / n_parts, hi = n * (k + 1) / n_parts;
        size_t cap = (k == 0 ? header.size() : 0) + (hi - lo) * (2 * 10 + 5) + 128;
        for (size_t j = lo; j < hi; ++j) {
            const uint32_t i = order[j];
            cap += targets[i].chrom.size() + value_bound(p1[i]) + value_bound(p2[i]);
        }
        part_off[k + 1] = part_off[k] + ((cap + 63) & ~(size_t)63);
    }
    const auto t_w1b = Clock::now();
    const size_t huge = 2u << 20, map_len = (part_off[n_parts] + huge - 1) / huge * huge;
    char *const base = (char *)::mmap(nullptr, map_len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (base == (char *)MAP_FAILED) {
        set_err(errbuf, errcap, "cannot allocate the output buffer");
        return INQ_EXIT_ERROR;
    }
    auto format_part = [&](size_t k) {
        const size_t lo = n * k / n_parts, hi = n * (k + 1) / n_parts;
        char *p = base + part_off[k];
        if (k == 0) std::memcpy(p, header.data(), header.size()), p += header.size();
        for (size_t j = lo; j < hi; ++j) {
            const uint32_t i = order[j];
            const RepeatInterval &t = targets[i];
            p = write_row(p, t.chrom, t.start, t.end, p1[i], p2[i]);
            *p++ = '\n';
        }
        part_len[k] = (size_t)(p - (base + part_off[k]));
    };
    {
        std::vector<std::thread> th;
        for (size_t k = 1; k < n_parts; ++k) th.emplace_back(format_part, k);
        format_part(0);
        for (auto &x : th) x.join();
    }
    const auto t_w2 = Clock::now();
    bool wrote = true;
    for (size_t k = 0; k < n_parts && wrote; ++k) wrote = write_all(out_fd, base + part_off[k], part_len[k]);
    ::munmap(base, map_len);
    if (!wrote) {
        set_err(errbuf, errcap, "Failed writing the result.");
        return INQ_EXIT_PANIC;
    }
    if (const TargetReports *const tr = reports.reports) {  // each file that was collected and has somewhere to go, in the rows' order
        const bool unphased = reports.unphased;
        size_t disagree = 0;  // the locus-motifs file: the targets whose catalogue motif is no rotation of the found one
        const struct {
            bool on;
            int fd;
            std::string header;
            const char *what;
            ReportRow row;  // one line per row; the tie report: per flagged row
        } files[] = {
            {tr->has.ties, reports.fds.ties, std::string(), kTiesWhat, tie_row(targets, tr->ties.data())},
            {tr->has.evidence, reports.fds.evidence, std::string(kEvidenceHeader) + '\n', kEvidenceWhat,
             [&targets, tr](std::string &text, uint32_t i) {
                 append_evidence_row(text, targets[i].chrom, targets[i].start, targets[i].end, tr->evidence[i]);
                 text += '\n';
             }},
            {tr->has.read_calls, reports.fds.read_calls, std::string(kReadCallsHeader) + '\n', kReadCallsWhat,
             [&targets, tr, unphased](std::string &text, uint32_t i) {
                 const std::vector<inq_read_call_t> &l = tr->read_calls[i];
                 append_read_calls_row(text, targets[i].chrom, targets[i].start, targets[i].end, l.data(), l.size(), unphased);
                 text += '\n';
             }},
            {tr->has.read_table, reports.fds.read_table, std::string(kReadTableHeader) + '\n', kReadTableWhat,
             [&targets, tr, unphased](std::string &text, uint32_t i) {  // one line per kept read: none for a target without one
                 const std::vector<inq_read_call_t> &l = tr->read_calls[i];
                 const ReadIdentities &w = tr->read_table[i];
                 if (w.recs.size() == l.size())
                     append_read_table_rows(text, targets[i].chrom, targets[i].start, targets[i].end, l.data(), w.recs.data(), w.bytes.data(),
                                            l.size(), unphased);
             }},
            {tr->has.read_seqs, reports.fds.read_seqs, std::string(kReadSeqsHeader) + '\n', kReadSeqsWhat,
             [&targets, tr, unphased](std::string &text, uint32_t i) {  // the table's lines, with the bases instead of the origin
                 const std::vector<inq_read_call_t> &l = tr->read_calls[i];
                 const ReadIdentities &w = tr->read_table[i];
                 const ReadSlices &q = tr->read_seqs[i];
                 if (w.recs.size() == l.size() && q.recs.size() == l.size())
                     append_read_seq_rows(text, targets[i].chrom, targets[i].start, targets[i].end, l.data(), w.recs.data(), w.bytes.data(),
                                          q.recs.data(), q.bytes.data(), l.size(), unphased);
             }},
            {tr->has.read_motifs, reports.fds.read_motifs, std::string(kReadMotifsHeader) + '\n', kReadMotifsWhat,
             [&targets, tr, unphased](std::string &text, uint32_t i) {  // the same lines again, with the motif runs instead of the bases
                 const std::vector<inq_read_call_t> &l = tr->read_calls[i];
                 const ReadIdentities &w = tr->read_table[i];
                 const ReadSlices &q = tr->read_seqs[i];
                 const std::vector<inq_read_motif_t> &m = tr->read_motifs[i];
                 if (w.recs.size() == l.size() && q.recs.size() == l.size() && m.size() == l.size())
                     append_read_motif_rows(text, targets[i].chrom, targets[i].start, targets[i].end, l.data(), w.recs.data(), w.bytes.data(),
                                            q.recs.data(), m.data(), tr->printed_word(i), l.size(), unphased);
             }},
            {tr->has.locus_motifs, reports.fds.locus_motifs, std::string(kLocusMotifsHeader) + '\n', kLocusMotifsWhat,
             [&targets, tr, &disagree](std::string &text, uint32_t i) {  // one line per target: the motif its kept reads repeat
                 disagree += append_locus_motif_row(text, targets[i].chrom, targets[i].start, targets[i].end, tr->read_calls[i].size(),
                                                    tr->locus_motifs[i], tr->motif_word[i]) == 0;
             }},
        };
        for (const auto &f : files) {
            if (!f.on || f.fd < 0) continue;
            const int frc = write_report(order, f.header, f.row, f.what, f.fd, errbuf, errcap);
            if (frc != INQ_EXIT_OK) return frc;
        }
        if (tr->has.locus_motifs && reports.fds.locus_motifs >= 0 && disagree)
            std::fprintf(stderr, "%zu of %zu targets have a catalogue motif that their reads do not repeat: `0` in the locus-motifs file\n", disagree, n);
    }
    if (timing_level())
        std::fprintf(stderr, "[inq output] %zu rows: order %.2f ms, bounds %.2f ms, text %.2f ms (%zu threads), write %.2f ms\n", n, ms(t_w0, t_w1), ms(t_w1, t_w1b), ms(t_w1b, t_w2),
                     n_parts, ms(t_w2, Clock::now()));
    return INQ_EXIT_OK;
}

}  // namespace inqhost

struct inq_frontend {
    Prepared P;
    std::unique_ptr<FrontEnd> fe;           // threads <= 1: one sweep on the caller's thread
    std::unique_ptr<ParallelFrontEnd> pfe;  // threads  > 1: the same worker pool the CLI driver uses
    ParallelFrontEnd::Item item;
    HostBatch batch;
    std::string bam_path;
    CallOptions opt;
    uint64_t threads = 1, max_words = 0;
    const HostBatch *current = nullptr;  // the batch the last inq_frontend_next handed out (inq_frontend_read_names, _read_seqs)
    bool keep_seqs = false;              // inq_frontend_set_keep_seqs
};

// target i of a prepared call, for the two handles that show their list (0, or -1 past its end)
static int target_at(const Prepared &P, uint64_t i, const char **chrom, uint32_t *start, uint32_t *end) {
    if (i >= P.targets.size()) return -1;
    if (chrom) *chrom = P.targets[i].chrom.c_str();
    if (start) *start = P.targets[i].start;
    if (end) *end = P.targets[i].end;
    return 0;
}

extern "C" {

static int inq_frontend_open_impl(const inq_call_args_t *args, inq_frontend_t **out, char *errbuf, size_t errcap) {
    if (!out) return INQ_EXIT_ERROR;
    *out = nullptr;
    std::unique_ptr<inq_frontend> F(new inq_frontend());
    const int rc = prepare(args, F->P, errbuf, errcap);
    if (rc != INQ_EXIT_OK) return rc;
    F->opt = CallOptions(*args);
    F->threads = args->threads;
    F->bam_path = args->bam;
    if (F->threads <= 1) F->fe.reset(new FrontEnd(*F->P.bam, F->P.targets, F->opt.unphased));
    if (F->fe) F->fe->set_keep_names(true);  // every batch this handle hands out names its reads (inq_frontend_read_names)
    *out = F.release();
    return INQ_EXIT_OK;
}

uint64_t inq_frontend_n_targets(const inq_frontend_t *fe) { return fe ? fe->P.targets.size() : 0; }

int inq_frontend_target(const inq_frontend_t *fe, uint64_t i, const char **chrom, uint32_t *start, uint32_t *end) {
    return fe ? target_at(fe->P, i, chrom, start, end) : -1;
}

const char *inq_frontend_target_name(const inq_frontend_t *fe, uint64_t i) {
    return fe && i < fe->P.target_name.size() ? fe->P.target_name[i].c_str() : nullptr;
}

const char *inq_frontend_sample(const inq_frontend_t *fe) { return fe ? fe->P.sample.c_str() : ""; }

void inq_frontend_set_batch_words(inq_frontend_t *fe, uint64_t w) {
    if (!fe) return;
    fe->max_words = w;
    if (fe->fe) fe->fe->set_max_batch_words(w);
}

void inq_frontend_set_keep_seqs(inq_frontend_t *fe, int on) {
    if (!fe) return;
    fe->keep_seqs = on != 0;
    if (fe->fe) fe->fe->set_keep_seqs(on != 0);
}

static int inq_frontend_next_impl(inq_frontend_t *fe, inq_batch_t *batch, const uint32_t **locus_index, char *errbuf,
                      size_t errcap) {
    if (!fe || !batch) return -INQ_EXIT_ERROR;
    std::string err;
    bool panic = false;
    fe->current = nullptr;
    if (fe->threads > 1) {  // batches arrive in completion order; locus_index says where each row belongs
        if (!fe->pfe)
            fe->pfe.reset(new ParallelFrontEnd(fe->bam_path, *fe->P.bam, fe->P.targets, fe->opt.unphased,
                                               (int)std::min<uint64_t>(fe->threads, 64), fe->max_words, true, fe->keep_seqs));
        fe->pfe->recycle(std::move(fe->item));
        fe->item = ParallelFrontEnd::Item();
        int rc = fe->pfe->next(fe->item, &err, &panic);
        if (rc < 0) {
            set_err(errbuf, errcap, err);
            return -INQ_EXIT_PANIC;
        }
        if (rc == 0) return 0;
        fe->item.batch.view(batch, fe->opt.minlen, fe->opt.support, fe->opt.unphased);
        if (locus_index) *locus_index = fe->item.index.data();
        fe->current = &fe->item.batch;
        return 1;
    }
    int rc = fe->fe->next(fe->batch, &err, &panic);
    if (rc < 0) {
        set_err(errbuf, errcap, err);
        return -INQ_EXIT_PANIC;  // read errors are expect()/unwrap() panics too (:294,346)
    }
    if (rc == 0) return 0;
    fe->batch.view(batch, fe->opt.minlen, fe->opt.support, fe->opt.unphased);
    if (locus_index) *locus_index = fe->batch.locus_index.data();
    fe->current = &fe->batch;
    return 1;
}

int inq_frontend_read_names(const inq_frontend_t *fe, const uint64_t **name_off, const uint8_t **names, uint64_t *n_reads) {
    if (!fe || !fe->current || fe->current->names.off.size() != fe->current->reads.size() + 1) return INQ_EXIT_ERROR;
    if (name_off) *name_off = fe->current->names.off.data();
    if (names) *names = fe->current->names.bytes.data();
    if (n_reads) *n_reads = fe->current->reads.size();
    return INQ_EXIT_OK;
}

int inq_frontend_read_seqs(const inq_frontend_t *fe, const uint32_t **l_seq, const uint64_t **seq_off, const uint8_t **seqs, uint64_t *n_reads) {
    if (!fe || !fe->current || fe->current->seqs.off.size() != fe->current->reads.size() + 1) return INQ_EXIT_ERROR;
    if (l_seq) *l_seq = fe->current->l_seq.data();
    if (seq_off) *seq_off = fe->current->seqs.off.data();
    if (seqs) *seqs = fe->current->seqs.bytes.data();
    if (n_reads) *n_reads = fe->current->reads.size();
    return INQ_EXIT_OK;
}

void inq_frontend_close(inq_frontend_t *fe) { delete fe; }


static int inq_genotype_repeats_impl(const inq_call_args_t *args, int out_fd, char *errbuf, size_t errcap, const RowsOut &rows = RowsOut(),
                                     const ReportPaths &more = ReportPaths()) {
    const auto t_start = Clock::now();
    std::string msg;
    CallReports files;  // (a call that returns rows writes no file: the tie report is left out, the evidence file refused)
    if (args && (rows.active ? refuse_evidence(args, "inq_genotype_repeats_rows", msg) : files.open(*args, more, msg)) != INQ_EXIT_OK) {
        set_err(errbuf, errcap, msg);
        return INQ_EXIT_ERROR;
    }
    AsyncCtx actx;
    if (args) actx.start(args->device);
    Prepared P;
    int rc = prepare(args, P, errbuf, errcap);
    if (rc != INQ_EXIT_OK) return rc;
    SessionHooks hooks;
    files.to(hooks);
    std::vector<uint64_t> words;
    if ((more.read_motifs || more.locus_motifs) && !rows.active) {
        if (target_motif_words(P, more.motif, more.read_motifs && !motif_is_auto(more.motif), words, msg) != INQ_EXIT_OK) {
            set_err(errbuf, errcap, msg);
            return INQ_EXIT_ERROR;
        }
        hooks.motif_words = &words;
    }
    hooks.process_is_leaving = fast_exit();  // the context is this call's own, and so is the process's end (the CLI's `call`)
    rc = genotype_prepared(args, actx, P, out_fd, errbuf, errcap, rows, t_start, hooks);
    actx.leak = rc == INQ_EXIT_OK && hooks.process_is_leaving;  // only after a clean run: error paths tear down normally
    return rc;
}

}  // extern "C"
int inqhost::genotype_single(const inq_call_args_t *args, int out_fd, const ReportPaths &more, char *errbuf, size_t errcap) {
    return inq_genotype_repeats_impl(args, out_fd, errbuf, errcap, RowsOut(), more);
}
extern "C" {

int inq_frontend_open(const inq_call_args_t *args, inq_frontend_t **out, char *errbuf, size_t errcap) {
    INQ_GUARD(inq_frontend_open_impl(args, out, errbuf, errcap), errbuf, errcap)
}
int inq_frontend_next(inq_frontend_t *fe, inq_batch_t *batch, const uint32_t **locus_index, char *errbuf, size_t errcap) {
    INQ_GUARD_AS(-INQ_EXIT_ERROR, inq_frontend_next_impl(fe, batch, locus_index, errbuf, errcap), errbuf, errcap)
}
int inq_genotype_repeats(const inq_call_args_t *args, int out_fd, char *errbuf, size_t errcap) {
    INQ_GUARD(inq_genotype_repeats_impl(args, out_fd, errbuf, errcap), errbuf, errcap)
}

// ---- one process per GPU: this process's share of the targets, rows as numbers ----
static int inq_genotype_repeats_rows_impl(const inq_call_args_t *args, const uint32_t *target_index, uint64_t n_index, double *phase1,
                                          double *phase2, char *errbuf, size_t errcap) {
    if (n_index && (!target_index || !phase1 || !phase2)) {
        set_err(errbuf, errcap, "null argument");
        return INQ_EXIT_ERROR;
    }
    RowsOut r;
    r.idx = target_index;
    r.n = n_index;
    r.p1 = phase1;
    r.p2 = phase2;
    r.active = true;
    return inq_genotype_repeats_impl(args, -1, errbuf, errcap, r);
}
int inq_genotype_repeats_rows(const inq_call_args_t *args, const uint32_t *target_index, uint64_t n_index, double *phase1, double *phase2,
                              char *errbuf, size_t errcap) {
    INQ_GUARD(inq_genotype_repeats_rows_impl(args, target_index, n_index, phase1, phase2, errbuf, errcap), errbuf, errcap)
}

}  // extern "C"

namespace inqhost {

// The targets in file order (contig of the BAM header, start, end, position in the list) and `world` + 1 cut points into
// that order, so that every part needs about the same number of compressed BAM bytes: cost of a target = bytes between its
// scan start in the .bai's linear index and the next target's, capped so that one far-away locus does not own a contig.
int partition_prepared(Prepared &P, uint64_t world, uint32_t *order, uint64_t *cuts) {
    const size_t n = P.targets.size();
    std::vector<int> tid(n);
    {
        std::map<std::string, int> memo;
        for (size_t i = 0; i < n; ++i) {
            auto it = memo.find(P.targets[i].chrom);
            if (it == memo.end()) it = memo.emplace(P.targets[i].chrom, P.bam->tid(P.targets[i].chrom)).first;
            tid[i] = it->second;
        }
    }
    for (size_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
    std::stable_sort(order, order + n, [&](uint32_t a, uint32_t b) {
        if (tid[a] != tid[b]) return tid[a] < tid[b];
        if (P.targets[a].start != P.targets[b].start) return P.targets[a].start < P.targets[b].start;
        return P.targets[a].end < P.targets[b].end;
    });
    std::vector<double> off(n), cost(n, 1.0);
    for (size_t k = 0; k < n; ++k) {
        const RepeatInterval &t = P.targets[order[k]];
        off[k] = (double)(P.bam->index().scan_start(tid[order[k]], t.start >= 10 ? (int64_t)t.start - 10 : 0) >> 16);
    }
    std::vector<double> d;
    for (size_t k = 0; k + 1 < n; ++k)
        if (tid[order[k]] == tid[order[k + 1]] && off[k + 1] > off[k]) d.push_back(off[k + 1] - off[k]);
    if (!d.empty()) {
        std::vector<double> ds = d;
        std::sort(ds.begin(), ds.end());
        const double cap = ds[std::min(ds.size() - 1, (size_t)(0.99 * (double)ds.size()))] * 4 + 1, med = ds[ds.size() / 2];
        for (size_t k = 0; k < n; ++k) {
            const bool same = k + 1 < n && tid[order[k]] == tid[order[k + 1]] && off[k + 1] > off[k];
            cost[k] += same ? std::min(off[k + 1] - off[k], cap) : med;  // last target of a contig: a typical gap
        }
    }
    std::vector<double> csum(n + 1, 0.0);
    for (size_t k = 0; k < n; ++k) csum[k + 1] = csum[k] + cost[k];
    cuts[0] = 0;
    for (uint64_t r = 1; r < world; ++r) {
        const double want = csum[n] * (double)r / (double)world;
        uint64_t k = (uint64_t)(std::lower_bound(csum.begin(), csum.end(), want) - csum.begin());
        cuts[r] = std::min<uint64_t>(std::max<uint64_t>(k, cuts[r - 1]), n);
    }
    cuts[world] = n;
    return INQ_EXIT_OK;
}

}  // namespace inqhost

extern "C" {

static int inq_host_partition_impl(const inq_call_args_t *args, uint64_t world, uint32_t *order, uint64_t order_cap, uint64_t *cuts,
                                   uint64_t *n_targets, char *errbuf, size_t errcap) {
    if (!world || !cuts || !n_targets) {
        set_err(errbuf, errcap, "null argument");
        return INQ_EXIT_ERROR;
    }
    Prepared P;
    const int rc = prepare(args, P, errbuf, errcap);
    if (rc != INQ_EXIT_OK) return rc;
    const size_t n = P.targets.size();
    *n_targets = n;
    if (n > order_cap || (n && !order)) {
        set_err(errbuf, errcap, "order[] too small for the target list");
        return INQ_EXIT_ERROR;
    }
    return partition_prepared(P, world, order, cuts);
}
int inq_host_partition(const inq_call_args_t *args, uint64_t world, uint32_t *order, uint64_t order_cap, uint64_t *cuts, uint64_t *n_targets,
                       char *errbuf, size_t errcap) {
    INQ_GUARD(inq_host_partition_impl(args, world, order, order_cap, cuts, n_targets, errbuf, errcap), errbuf, errcap)
}


struct inq_run {
    std::unique_ptr<OwnedArgs> args;
    Prepared P;
    // inq_run_rows_device: the context outlives the call (its rows are read from device memory afterwards)
    std::unique_ptr<AsyncCtx> actx;
    // inq_session_run_open: context, span buffers and BED cache are the session's (which outlives the run)
    inq_session *sess = nullptr;
    double *d1 = nullptr, *d2 = nullptr;
    uint64_t dcap = 0;
    // the reports of the last rows call: the tie flags, collected when the run was opened with ties_path set
    TargetReports reports;
    bool have_ties = false;
    AsyncCtx *ctx_of_rows() { return sess ? &sess->actx : actx.get(); }
    ~inq_run() {
        AsyncCtx *c = ctx_of_rows();
        if (d1 && c && c->wait()) inq_dev_free_rows(c->ctx, d1);  // (d2 points into the same allocation)
    }
};

static int inq_run_open_impl(const inq_call_args_t *args, inq_run_t **out, char *errbuf, size_t errcap, inq_session *sess = nullptr) {
    if (!out || !args) return INQ_EXIT_ERROR;
    *out = nullptr;
    std::string refused;
    if (refuse_evidence(args, "a prepared run (inq_run_*)", refused) != INQ_EXIT_OK) {
        set_err(errbuf, errcap, refused);
        return INQ_EXIT_ERROR;
    }
    std::unique_ptr<inq_run> R(new inq_run());
    R->args.reset(new OwnedArgs(*args));
    R->sess = sess;
    if (sess) R->args->a.device = sess->device;
    const int rc = prepare(&R->args->a, R->P, errbuf, errcap, sess ? &sess->bed_cache : nullptr);
    if (rc != INQ_EXIT_OK) return rc;
    *out = R.release();
    return INQ_EXIT_OK;
}
int inq_run_open(const inq_call_args_t *args, inq_run_t **out, char *errbuf, size_t errcap) {
    INQ_GUARD(inq_run_open_impl(args, out, errbuf, errcap), errbuf, errcap)
}
int inq_session_run_open(inq_session_t *s, const inq_call_args_t *args, inq_run_t **out, char *errbuf, size_t errcap) {
    if (!s) {
        set_err(errbuf, errcap, "null session");
        return INQ_EXIT_ERROR;
    }
    INQ_GUARD(inq_run_open_impl(args, out, errbuf, errcap, s), errbuf, errcap)
}
uint64_t inq_run_n_targets(const inq_run_t *r) { return r ? r->P.targets.size() : 0; }
const char *inq_run_sample(const inq_run_t *r) { return r ? r->P.sample.c_str() : ""; }
int inq_run_target(const inq_run_t *r, uint64_t i, const char **chrom, uint32_t *start, uint32_t *end) {
    return r ? target_at(r->P, i, chrom, start, end) : -1;
}
int inq_run_partition(inq_run_t *r, uint64_t world, uint32_t *order, uint64_t *cuts, char *errbuf, size_t errcap) {
    if (!r || !world || !cuts || (!order && !r->P.targets.empty())) {
        set_err(errbuf, errcap, "null argument");
        return INQ_EXIT_ERROR;
    }
    INQ_GUARD(partition_prepared(r->P, world, order, cuts), errbuf, errcap)
}
// The rows of the targets target_index[0 .. n_index) on actx, which outlives the call (the session's, or the run's own: nothing is made
// or torn down per call) or is the caller's to end; ro says where they go.  The tie flags are collected when the run was opened
// with ties_path set.
static int run_rows_on(inq_run_t *r, AsyncCtx &actx, RowsOut ro, const uint32_t *target_index, uint64_t n_index, Clock::time_point t_start,
                       char *errbuf, size_t errcap) {
    ro.idx = target_index, ro.n = n_index, ro.active = true;
    SessionHooks hooks;
    if (r->sess) hooks.pool = &r->sess->pool;  // the session's span buffers
    r->have_ties = false;
    ReportSet which;
    which.ties = r->args->a.ties_path != nullptr;
    r->reports.begin(n_index, which);
    hooks.reports = &r->reports;
    const int rc = genotype_prepared(&r->args->a, actx, r->P, -1, errbuf, errcap, ro, t_start, hooks);
    r->have_ties = rc == INQ_EXIT_OK && which.ties;
    return rc;
}
static int inq_run_rows_impl(inq_run_t *r, const uint32_t *target_index, uint64_t n_index, double *phase1, double *phase2, char *errbuf,
                             size_t errcap) {
    if (!r || (n_index && (!target_index || !phase1 || !phase2))) {
        set_err(errbuf, errcap, "null argument");
        return INQ_EXIT_ERROR;
    }
    const auto t_start = Clock::now();
    RowsOut ro;
    ro.p1 = phase1, ro.p2 = phase2;
    if (r->sess) return run_rows_on(r, r->sess->actx, ro, target_index, n_index, t_start, errbuf, errcap);
    AsyncCtx actx;  // this call's own, destroyed with it
    actx.start(r->args->a.device);
    return run_rows_on(r, actx, ro, target_index, n_index, t_start, errbuf, errcap);
}
int inq_run_rows(inq_run_t *r, const uint32_t *target_index, uint64_t n_index, double *phase1, double *phase2, char *errbuf, size_t errcap) {
    INQ_GUARD(inq_run_rows_impl(r, target_index, n_index, phase1, phase2, errbuf, errcap), errbuf, errcap)
}
static int inq_run_rows_device_impl(inq_run_t *r, const uint32_t *target_index, uint64_t n_index, uint64_t width, void **d_phase1, void **d_phase2,
                                    char *errbuf, size_t errcap) {
    if (!r || !d_phase1 || !d_phase2 || width < n_index || (n_index && !target_index)) {
        set_err(errbuf, errcap, "null argument, or width below the number of targets");
        return INQ_EXIT_ERROR;
    }
    *d_phase1 = *d_phase2 = nullptr;
    const auto t_start = Clock::now();
    if (!r->sess && !r->actx) {
        r->actx.reset(new AsyncCtx());
        r->actx->start(r->args->a.device);
    }
    AsyncCtx &actx = *r->ctx_of_rows();
    if (!actx.wait()) {
        set_err(errbuf, errcap, ctx_failure_message(actx));
        return INQ_EXIT_ERROR;
    }
    // one array of 2 x width: phase1 row, phase2 row (one collective's buffer); made afresh per call - every entry starts as NaN, a
    // device allocation costs microseconds (tools/alloc_probe.hip)
    const uint64_t w = std::max<uint64_t>(width, 1);
    inq_dev_free_rows(actx.ctx, r->d1);
    r->d1 = r->d2 = nullptr, r->dcap = 0;
    if (inq_dev_alloc_rows(actx.ctx, 2 * w, &r->d1) != INQ_OK) {
        set_err(errbuf, errcap, "cannot allocate the device row arrays");
        return INQ_EXIT_ERROR;
    }
    r->d2 = r->d1 + w, r->dcap = w;
    RowsOut ro;
    ro.d1 = r->d1, ro.d2 = r->d2, ro.dcap = r->dcap;
    const int rc = run_rows_on(r, actx, ro, target_index, n_index, t_start, errbuf, errcap);
    if (rc != INQ_EXIT_OK) return rc;
    *d_phase1 = r->d1, *d_phase2 = r->d2;
    return INQ_EXIT_OK;
}
int inq_run_rows_device(inq_run_t *r, const uint32_t *target_index, uint64_t n_index, uint64_t width, void **d_phase1, void **d_phase2, char *errbuf,
                        size_t errcap) {
    INQ_GUARD(inq_run_rows_device_impl(r, target_index, n_index, width, d_phase1, d_phase2, errbuf, errcap), errbuf, errcap)
}
int inq_run_write_inq(inq_run_t *r, const double *phase1, const double *phase2, uint64_t n_rows, int out_fd, char *errbuf, size_t errcap) {
    if (!r || n_rows != r->P.targets.size() || (n_rows && (!phase1 || !phase2))) {
        set_err(errbuf, errcap, "row count does not match the target list");
        return INQ_EXIT_ERROR;
    }
    INQ_GUARD(write_rows(r->args->a.threads, r->P.targets, r->P.sample, phase1, phase2, out_fd, errbuf, errcap), errbuf, errcap)
}
int inq_run_tie_flags(const inq_run_t *r, uint8_t *flags, uint64_t n) {
    if (!r || !r->have_ties || n != r->reports.ties.size() || (n && !flags)) return INQ_EXIT_ERROR;
    if (n) std::memcpy(flags, r->reports.ties.data(), n);
    return INQ_EXIT_OK;
}
int inq_run_write_ties(inq_run_t *r, const uint8_t *flags, uint64_t n_rows, int fd, char *errbuf, size_t errcap) {
    if (!r || n_rows != r->P.targets.size() || (n_rows && !flags)) {
        set_err(errbuf, errcap, "flag count does not match the target list");
        return INQ_EXIT_ERROR;
    }
    INQ_GUARD(write_ties(row_order(r->args->a.threads, r->P.targets), r->P.targets, flags, fd, errbuf, errcap), errbuf, errcap)
}
void inq_run_close(inq_run_t *r) { delete r; }

}  // extern "C"
