// outlier.cc — `inquiSTR outlier` (src/outlier.rs:33-73, src/main.rs:75-99,202-229): reads a combined .inq,
// hands the numbers of all loci to the GPU in one matrix (inq_outlier_rows) and prints the loci with
// outlying samples.  Text in, text out; the arithmetic is not here.  The steps in the order they run: check_args, read_subset, the text
// and its lines, sample_names, parse_matrix, the device call, print_outliers; what `assoc` does the same way is in text_input.h.
#include <cstdint>
#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "../../include/inquistr_host.h"

#include "text_input.h"

namespace {

using namespace inq::textin;

void check_args(const inq_outlier_args_t *a) {
    if (!a || !a->combined) throw Failure{INQ_EXIT_ERROR, "no combined file given"};
    struct stat st;
    if (::stat(a->combined, &st) != 0) throw Failure{INQ_EXIT_PANIC, "Combined file does not exist!"};  // src/main.rs:210-212
    if (a->sample && a->subset_file) throw Failure{INQ_EXIT_PANIC, "Cannot use both -s and -S arguments"};  // src/main.rs:214-216
    if (a->method != INQ_OUTLIER_ZSCORE && a->method != INQ_OUTLIER_DBSCAN) throw Failure{INQ_EXIT_ERROR, "unknown method"};
}

// -s / -S: a locus is printed only when one of these samples is among its outliers
struct Subset {
    bool given = false;
    std::vector<std::string> names;
};
Subset read_subset(const inq_outlier_args_t *a) {
    Subset s;
    if (a->sample) s.given = true, s.names.emplace_back(a->sample);
    if (a->subset_file) {  // one name per line, src/main.rs:220-223
        Lines sf;
        if (!sf.open(a->subset_file)) throw Failure{INQ_EXIT_PANIC, "Problem opening file"};
        s.given = true;
        std::string l;
        while (sf.next(l)) s.names.push_back(l);
    }
    return s;
}

// the header's columns from the fourth on, as they stand
std::vector<std::string> sample_names(const std::string &header) {
    std::vector<std::pair<size_t, size_t>> fld;
    split_tabs(header, fld);
    std::vector<std::string> samples;
    for (size_t k = 3; k < fld.size(); ++k) samples.push_back(header.substr(fld[k].first, fld[k].second));
    return samples;
}

// The numbers of the loci in front of the first line that makes the reference panic.  The reference works line by line: what it
// printed before a panic stays printed.  The first such line (fewer than three fields, a number that does not parse) ends the input
// here; the lines in front of it are still computed and printed, and late_panic is said after them.
struct Matrix {
    std::unique_ptr<float[]> values;  // [row_len.size()][stride]; a row's values beyond its row_len are not set
    std::vector<uint32_t> row_len;
    size_t stride = 0;
    std::string late_panic;
};
// The numbers are what the command spends its time on (40 million of them in a 200 000 x 200 cohort), the GPU part is milliseconds:
// the lines are parsed by several threads.
Matrix parse_matrix(const CombinedText &txt) {
    Matrix m;
    const size_t n_lines = txt.loci();
    const size_t n_thr = thread_count(n_lines, kLinesPerThread);
    auto chunk = [&](size_t t) { return std::make_pair(n_lines * t / n_thr, n_lines * (t + 1) / n_thr); };
    m.row_len.assign(n_lines, 0);
    std::vector<size_t> bad_a(n_thr, (size_t)-1);
    on_threads(n_thr, [&](size_t t) {  // pass A: fields per line, a plain count of tabs
        auto [lo, hi] = chunk(t);
        for (size_t i = lo; i < hi; ++i) {
            size_t tabs = 0;
            for (const char *p = txt.begin(i), *end = txt.end(i); p < end; ++p) tabs += *p == '\t';
            if (tabs < 2) {  // splitline[2], :43
                bad_a[t] = i;
                return;
            }
            m.row_len[i] = (uint32_t)(tabs - 2);
        }
    });
    size_t first_bad = n_lines;
    for (size_t t = 0; t < n_thr; ++t)
        if (bad_a[t] < first_bad) first_bad = bad_a[t], m.late_panic = "index out of bounds: a line with fewer than three fields";
    for (size_t i = 0; i < first_bad; ++i) m.stride = std::max<size_t>(m.stride, m.row_len[i]);
    // not zero-filled: a row's values beyond row_len are never read (inq_outlier_rows), and 160 MB of zeros is time
    m.values.reset(new float[std::max<size_t>(first_bad * m.stride, 1)]);
    std::vector<size_t> bad_b(n_thr, (size_t)-1);
    on_threads(n_thr, [&](size_t t) {  // pass B: the numbers
        auto [lo, hi] = chunk(t);
        hi = std::min(hi, first_bad);
        for (size_t i = lo; i < hi; ++i) {
            float *row = m.values.get() + i * m.stride;
            if (walk_values(txt.begin(i), txt.end(i), [row](size_t k, const char *s, size_t n) { return parse_f32(s, n, &row[k]); }) == kWalkStopped) {  // :78
                bad_b[t] = i;
                return;
            }
        }
    });
    for (size_t t = 0; t < n_thr; ++t)
        if (bad_b[t] < first_bad) first_bad = bad_b[t], m.late_panic = "Failed to parse number";
    m.row_len.resize(first_bad);
    return m;
}

// one of the reference's panics in the middle of its output: what it had printed stays printed
[[noreturn]] void panic_after(const OutBuffer &out, const char *message) {
    write_all(out.fd, out.text);
    throw Failure{INQ_EXIT_PANIC, message};
}

// `chrom begin end outliers` of every kept locus with a flagged sample (one of the subset, where there is one), src/outlier.rs:47-66
void print_outliers(const CombinedText &txt, const std::vector<std::string> &samples, const Subset &subset, const Matrix &m,
                    const std::vector<uint8_t> &flags, const std::vector<uint8_t> &keep, OutBuffer &out) {
    for (size_t i = 0; i < m.row_len.size(); ++i) {
        switch (keep[i]) {
        case INQ_OUTLIER_ROW_SKIP: continue;
        case INQ_OUTLIER_ROW_EMPTY: panic_after(out, "called `Option::unwrap()` on a `None` value (a locus without values)");
        case INQ_OUTLIER_ROW_NO_MODE: panic_after(out, "No mode found for repeat");
        case INQ_OUTLIER_ROW_TOO_WIDE: throw Failure{INQ_EXIT_ERROR, "DBSCAN on more than 8192 values per locus is not supported"};
        default: break;
        }
        std::string names;
        bool any = false, in_subset = !subset.given;
        for (uint32_t k = 0; k < m.row_len[i]; ++k) {
            if (!flags[i * m.stride + k]) continue;
            if (k >= samples.size()) panic_after(out, "index out of bounds: more values than samples in the header");  // samples[index], :108
            if (any) names += ',';
            names += samples[k];
            any = true;
            if (subset.given && !in_subset)
                for (const auto &s : subset.names)
                    if (s == samples[k]) in_subset = true;
        }
        if (any && in_subset) {
            Span c[3] = {};
            first_three(txt.begin(i), txt.end(i), c);  // (three fields are there: pass A of parse_matrix)
            for (const Span &f : c) out.text.append(f.p, f.n), out.text += '\t';
            out.text += names;
            out.text += '\n';
        }
        out.line_done();
    }
}

int outlier_impl(const inq_outlier_args_t *a, int out_fd) {
    check_args(a);
    const Subset subset = read_subset(a);
    BackgroundCtx device(a->device);
    const Laps lap{"outlier"};
    CombinedText txt;
    txt.read(a->combined);
    lap("text in memory");
    txt.split();
    lap("lines found");
    std::vector<std::string> samples = sample_names(txt.header());
    if (samples.empty()) {  // samples.len().ilog2(), :39; the header went out one line earlier (:37)
        write_all(out_fd, "chrom\tbegin\tend\toutliers\n");
        throw Failure{INQ_EXIT_PANIC, "argument of integer logarithm must be positive (no sample columns)"};
    }
    uint32_t mincluster = 0;
    for (size_t n = samples.size(); n > 1; n >>= 1) ++mincluster;
    for (auto &s : samples) s = strip_hap(s);
    const Matrix m = parse_matrix(txt);
    const size_t n_rows = m.row_len.size();
    std::vector<uint8_t> flags(n_rows * m.stride, 0), keep(n_rows, 0);
    lap("numbers parsed");
    inq_ctx_t *ctx = device.wait(lap);
    const int rc = inq_outlier_rows(ctx, m.values.get(), m.row_len.data(), n_rows, (uint32_t)m.stride, a->method, a->minsize, a->zscore, mincluster,
                                    flags.data(), keep.data());
    if (rc != INQ_OK) device_call_failed(rc, ctx);
    lap("kernels done");
    OutBuffer out{out_fd, "chrom\tbegin\tend\toutliers\n"};  // :37
    print_outliers(txt, samples, subset, m, flags, keep, out);
    out.flush();
    if (!m.late_panic.empty()) throw Failure{INQ_EXIT_PANIC, m.late_panic};
    return INQ_EXIT_OK;
}

}  // namespace

extern "C" int inq_outlier(const inq_outlier_args_t *args, int out_fd, char *errbuf, size_t errcap) {
    INQ_GUARD(outlier_impl(args, out_fd), errbuf, errcap)
}
