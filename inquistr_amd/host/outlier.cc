// outlier.cc — `inquiSTR outlier` (src/outlier.rs:33-73, src/main.rs:75-99,202-229): reads a combined .inq,
// hands the numbers of all loci to the GPU in one matrix (inq_outlier_rows) and prints the loci with
// outlying samples.  Text in, text out; the arithmetic is not here.
#include <zlib.h>
#include <sys/mman.h>
#include <fcntl.h>
#include <chrono>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <functional>
#include <string>
#include <limits>
#include <memory>
#include <thread>
#include <vector>

#include <sys/stat.h>
#include <unistd.h>

#include "../../include/inquistr_host.h"

#include "text_input.h"

namespace {

using namespace inq::textin;


int outlier_impl(const inq_outlier_args_t *a, int out_fd, char *errbuf, size_t errcap) {
    if (!a || !a->combined) {
        set_err(errbuf, errcap, "no combined file given");
        return INQ_EXIT_ERROR;
    }
    struct stat st;
    if (::stat(a->combined, &st) != 0) {  // src/main.rs:210-212
        set_err(errbuf, errcap, "Combined file does not exist!");
        return INQ_EXIT_PANIC;
    }
    if (a->sample && a->subset_file) {  // src/main.rs:214-216
        set_err(errbuf, errcap, "Cannot use both -s and -S arguments");
        return INQ_EXIT_PANIC;
    }
    if (a->method != INQ_OUTLIER_ZSCORE && a->method != INQ_OUTLIER_DBSCAN) {
        set_err(errbuf, errcap, "unknown method");
        return INQ_EXIT_ERROR;
    }
    bool have_subset = false;
    std::vector<std::string> subset;
    if (a->sample) have_subset = true, subset.emplace_back(a->sample);
    if (a->subset_file) {  // one name per line, src/main.rs:220-223
        Lines sf;
        if (!sf.open(a->subset_file)) {
            set_err(errbuf, errcap, "Problem opening file");
            return INQ_EXIT_PANIC;
        }
        have_subset = true;
        std::string l;
        while (sf.next(l)) subset.push_back(l);
    }
    // the HIP runtime starts (0.1 - 0.3 s) while the text is read and parsed
    inq_ctx_t *ctx = nullptr;
    int hrc = INQ_OK;
    std::thread ctx_thread([&] { hrc = inq_ctx_create(a->device, &ctx); });
    struct CtxGuard {
        inq_ctx_t *&c;
        std::thread &t;
        ~CtxGuard() {
            if (t.joinable()) t.join();
            const char *fast = std::getenv("INQ_FAST_EXIT");  // set by the CLI, which is about to leave the process
            if (!(fast && fast[0] == '1')) inq_ctx_destroy(c);
        }
    } ctx_guard{ctx, ctx_thread};
    // the whole text in memory, then lines parsed by several threads: the numbers are what the command spends its
    // time on (40 million of them in a 200 000 x 200 cohort), the GPU part is milliseconds.  A plain file is mapped (no copy:
    // the page cache is the buffer; round 2 pulled 139 MB through gzread, 0.1 s on one thread), a gzip file inflated.
    using clk = std::chrono::steady_clock;
    const bool timing = std::getenv("INQ_TIMING") != nullptr;
    const auto t_begin = clk::now();
    auto lap = [&](const char *what) {
        if (timing) std::fprintf(stderr, "[inq outlier] %-22s at %7.1f ms\n", what, std::chrono::duration<double, std::milli>(clk::now() - t_begin).count());
    };
    TextFile tf;
    {
        std::string lerr;
        if (!tf.load(a->combined, lerr)) {
            set_err(errbuf, errcap, lerr);
            return INQ_EXIT_PANIC;
        }
    }
    const char *const tdata = tf.data;
    const size_t tsize = tf.size;
    lap("text in memory");
    // BufRead::lines(): split on '\n' (a trailing '\r' goes too); no line after a final newline.  The newlines are found by
    // several threads, each over its own stretch of the text.
    std::vector<std::pair<size_t, size_t>> lines;  // (offset, length)
    find_lines(tdata, tsize, lines);
    lap("lines found");
    if (lines.empty()) {  // lines.next().unwrap(), src/outlier.rs:36
        set_err(errbuf, errcap, "called `Option::unwrap()` on a `None` value (empty combined file)");
        return INQ_EXIT_PANIC;
    }
    std::string line(tdata + lines[0].first, lines[0].second);
    std::vector<std::pair<size_t, size_t>> fld;
    split_tabs(line, fld);
    std::vector<std::string> samples;
    for (size_t k = 3; k < fld.size(); ++k) samples.push_back(line.substr(fld[k].first, fld[k].second));
    if (samples.empty()) {  // samples.len().ilog2(), :39; the header went out one line earlier (:37)
        write_all(out_fd, "chrom\tbegin\tend\toutliers\n");
        set_err(errbuf, errcap, "argument of integer logarithm must be positive (no sample columns)");
        return INQ_EXIT_PANIC;
    }
    uint32_t mincluster = 0;
    for (size_t n = samples.size(); n > 1; n >>= 1) ++mincluster;
    for (auto &s : samples) s = strip_hap(s);

    // The reference works line by line: what it printed before a panic stays printed.  The first line that makes
    // it panic (fewer than three fields, a number that does not parse) ends the input here; the lines in front
    // of it are still computed and printed.
    const size_t n_lines = lines.size() - 1;
    const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    const size_t n_thr = std::max<size_t>(1, std::min<size_t>(hw, n_lines / 2048 + 1));
    std::vector<uint32_t> row_len(n_lines, 0);
    std::vector<size_t> bad_a(n_thr, (size_t)-1);
    auto chunk = [&](size_t t) { return std::make_pair(n_lines * t / n_thr, n_lines * (t + 1) / n_thr); };
    auto parallel = [&](const std::function<void(size_t)> &fn) {
        std::vector<std::thread> th;
        for (size_t t = 1; t < n_thr; ++t) th.emplace_back(fn, t);
        fn(0);
        for (auto &x : th) x.join();
    };
    parallel([&](size_t t) {  // pass A: fields per line
        auto [lo, hi] = chunk(t);
        for (size_t i = lo; i < hi; ++i) {
            const char *p = tdata + lines[i + 1].first;
            size_t tabs = 0;
            for (size_t k = 0; k < lines[i + 1].second; ++k) tabs += p[k] == '\t';
            if (tabs < 2) {  // splitline[2], :43
                bad_a[t] = i;
                return;
            }
            row_len[i] = (uint32_t)(tabs - 2);
        }
    });
    size_t first_bad = n_lines;
    std::string late_panic;
    for (size_t t = 0; t < n_thr; ++t)
        if (bad_a[t] < first_bad) first_bad = bad_a[t], late_panic = "index out of bounds: a line with fewer than three fields";
    size_t stride = 0;
    for (size_t i = 0; i < first_bad; ++i) stride = std::max<size_t>(stride, row_len[i]);
    // not zero-filled: a row's values beyond row_len are never read (inq_outlier_rows), and 160 MB of zeros is time
    std::unique_ptr<float[]> mat_mem(new float[std::max<size_t>(first_bad * stride, 1)]);
    float *const mat = mat_mem.get();
    std::vector<size_t> bad_b(n_thr, (size_t)-1);
    parallel([&](size_t t) {  // pass B: the numbers
        auto [lo, hi] = chunk(t);
        hi = std::min(hi, first_bad);
        for (size_t i = lo; i < hi; ++i) {
            const char *p = tdata + lines[i + 1].first, *end = p + lines[i + 1].second;
            int field = 0;
            const char *f0 = p;
            for (const char *q = p;; ++q) {
                if (q == end || *q == '\t') {
                    if (field >= 3 && !parse_f32(f0, (size_t)(q - f0), &mat[i * stride + (size_t)(field - 3)])) {  // :78
                        bad_b[t] = i;
                        return;
                    }
                    ++field;
                    f0 = q + 1;
                    if (q == end) break;
                }
            }
        }
    });
    for (size_t t = 0; t < n_thr; ++t)
        if (bad_b[t] < first_bad) first_bad = bad_b[t], late_panic = "Failed to parse number";
    row_len.resize(first_bad);
    auto coords_of = [&](size_t i) {  // chrom, begin, end as they stand in the file
        const char *p = tdata + lines[i + 1].first;
        size_t k = 0, tabs = 0;
        for (; k < lines[i + 1].second; ++k)
            if (p[k] == '\t' && ++tabs == 3) break;
        return std::string(p, k);
    };
    const size_t n_rows = first_bad;
    std::vector<uint8_t> flags(n_rows * stride, 0), keep(n_rows, 0);

    lap("numbers parsed");
    ctx_thread.join();
    lap("device context there");
    if (hrc != INQ_OK) {
        set_err(errbuf, errcap, std::string("cannot open HIP device: ") + inq_strerror(hrc));
        return INQ_EXIT_ERROR;
    }
    hrc = inq_outlier_rows(ctx, mat, row_len.data(), n_rows, (uint32_t)stride, a->method, a->minsize, a->zscore,
                           mincluster, flags.data(), keep.data());
    std::string detail = hrc == INQ_ERR_HIP ? inq_last_error(ctx) : "";
    if (hrc != INQ_OK) {
        set_err(errbuf, errcap, std::string("device call failed: ") + inq_strerror(hrc) + (detail.empty() ? "" : " [" + detail + "]"));
        return INQ_EXIT_ERROR;
    }

    lap("kernels done");
    std::string out = "chrom\tbegin\tend\toutliers\n";  // :37
    for (size_t i = 0; i < n_rows; ++i) {
        switch (keep[i]) {
        case INQ_OUTLIER_ROW_SKIP: continue;
        case INQ_OUTLIER_ROW_EMPTY:
            write_all(out_fd, out);
            set_err(errbuf, errcap, "called `Option::unwrap()` on a `None` value (a locus without values)");
            return INQ_EXIT_PANIC;
        case INQ_OUTLIER_ROW_NO_MODE:
            write_all(out_fd, out);
            set_err(errbuf, errcap, "No mode found for repeat");
            return INQ_EXIT_PANIC;
        case INQ_OUTLIER_ROW_TOO_WIDE:
            set_err(errbuf, errcap, "DBSCAN on more than 8192 values per locus is not supported");
            return INQ_EXIT_ERROR;
        default: break;
        }
        std::string names;
        bool any = false, in_subset = !have_subset;
        for (uint32_t k = 0; k < row_len[i]; ++k) {
            if (!flags[i * stride + k]) continue;
            if (k >= samples.size()) {  // samples[index], :108
                write_all(out_fd, out);
                set_err(errbuf, errcap, "index out of bounds: more values than samples in the header");
                return INQ_EXIT_PANIC;
            }
            if (any) names += ',';
            names += samples[k];
            any = true;
            if (have_subset && !in_subset)
                for (const auto &s : subset)
                    if (s == samples[k]) in_subset = true;
        }
        if (any && in_subset) {  // :47-66
            out += coords_of(i);
            out += '\t';
            out += names;
            out += '\n';
        }
        if (out.size() > (1u << 20)) {
            if (!write_all(out_fd, out)) return INQ_EXIT_PANIC;
            out.clear();
        }
    }
    if (!write_all(out_fd, out)) return INQ_EXIT_PANIC;
    if (!late_panic.empty()) {
        set_err(errbuf, errcap, late_panic);
        return INQ_EXIT_PANIC;
    }
    return INQ_EXIT_OK;
}

}  // namespace

extern "C" int inq_outlier(const inq_outlier_args_t *args, int out_fd, char *errbuf, size_t errcap) {
    try {
        return outlier_impl(args, out_fd, errbuf, errcap);
    } catch (const std::exception &e) {
        set_err(errbuf, errcap, std::string("internal error: ") + e.what());
        return INQ_EXIT_ERROR;
    } catch (...) {
        set_err(errbuf, errcap, "internal error");
        return INQ_EXIT_ERROR;
    }
}
