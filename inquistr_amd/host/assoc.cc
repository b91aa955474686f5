// assoc.cc — `inquistr assoc` (the reference's scripts/STR_regression.R): reads a combined .inq and a phenotype
// file, hands the H1 / H2 pairs of the analysed samples of all loci to the GPU in one matrix (inq_assoc_rows) and prints the tested
// loci by ascending p-value.  With --firth the rows whose fit separation broke print Firth's fit (inq_assoc_rows_firth) in its place.
// Text in, text out; the regressions are not here.  The steps in the order they run: check_args, the text and its lines, make_design,
// pick_loci, fill_matrix, fit_rows, print_order, print_table, tally; what `outlier` does the same way is in text_input.h.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/inquistr_host.h"
#include "inq_text.h"
#include "text_input.h"

namespace {

using namespace inq::textin;

std::vector<std::string> split_on(const std::string &s, char sep) {
    std::vector<std::string> out;
    size_t p = 0;
    for (;;) {
        const size_t t = s.find(sep, p);
        out.push_back(s.substr(p, t == std::string::npos ? t : t - p));
        if (t == std::string::npos) return out;
        p = t + 1;
    }
}

// a finite number with nothing around it ("NA", "", "1.5x", "nan", "inf": no)
bool parse_finite(const std::string &s, double *out) {
    if (s.empty() || s[0] == ' ' || s[0] == '\t') return false;
    char *end = nullptr;
    const double v = std::strtod(s.c_str(), &end);
    if (end != s.c_str() + s.size() || !std::isfinite(v)) return false;
    *out = v;
    return true;
}

// The samples analysed: which value columns of the combined file they own, their outcome and covariates
struct Design {
    std::vector<std::string> names;
    std::vector<uint32_t> column;  // sample i owns value columns 2 * column[i], 2 * column[i] + 1 of the combined file
    std::vector<double> y;
    std::vector<double> cov;  // [k][n]
    std::vector<std::string> cov_names;
    std::string group1, group2;
    size_t file_columns = 0;  // value columns in the combined file's header
};

void check_args(const inq_assoc_args_t *a) {
    if (!a || !a->combined) throw Failure{INQ_EXIT_ERROR, "no combined file given"};
    if (!a->phenocovar || !a->phenotype) throw Failure{INQ_EXIT_ERROR, "no phenotype file or phenotype column given"};
    if (a->outcome != INQ_ASSOC_BINARY && a->outcome != INQ_ASSOC_CONTINUOUS) throw Failure{INQ_EXIT_ERROR, "unknown outcome"};
    if (a->str_mode != INQ_ASSOC_MAX && a->str_mode != INQ_ASSOC_MIN && a->str_mode != INQ_ASSOC_MEAN) throw Failure{INQ_EXIT_ERROR, "unknown STR mode"};
    struct stat st;
    if (::stat(a->combined, &st) != 0) throw Failure{INQ_EXIT_PANIC, "Combined file does not exist!"};  // src/assoc.rs:26-28
    if (::stat(a->phenocovar, &st) != 0) throw Failure{INQ_EXIT_PANIC, "Metadata file does not exist!"};  // :29-31
    if (a->outcome == INQ_ASSOC_BINARY && !(a->binary_order && *a->binary_order))
        throw Failure{INQ_EXIT_PANIC, "--binary-order is missing, please provide it with --outcome binary"};
    if (!(a->missing_cutoff == a->missing_cutoff)) throw Failure{INQ_EXIT_PANIC, "the missing cutoff is not a number"};
    if ((a->chr_begin >= 0) != (a->chr_end >= 0) || (a->chr_begin >= 0 && !a->chr))
        throw Failure{INQ_EXIT_PANIC, "--chr-begin and --chr-end go together, and with --chr"};
    if (a->firth != INQ_HOST_FIRTH_NO && a->firth != INQ_HOST_FIRTH_FALLBACK && a->firth != INQ_HOST_FIRTH_ALWAYS)
        throw Failure{INQ_EXIT_PANIC, "--firth takes no, fallback or always"};
    if (a->firth != INQ_HOST_FIRTH_NO && a->outcome != INQ_ASSOC_BINARY)
        throw Failure{INQ_EXIT_PANIC, "--firth is for --outcome binary: a continuous outcome has no separation"};
}

// header: the first line of the combined file
Design make_design(const inq_assoc_args_t *a, const std::string &header) {
    Design d;
    if (a->outcome == INQ_ASSOC_BINARY) {
        const auto ab = split_on(a->binary_order, ',');
        if (ab.size() != 2 || ab[0].empty() || ab[1].empty() || ab[0] == ab[1])
            throw Failure{INQ_EXIT_PANIC, "--binary-order takes two different values, as in Control,Patient"};
        d.group1 = ab[0], d.group2 = ab[1];
    }
    if (a->covariates && *a->covariates) d.cov_names = split_on(a->covariates, ',');
    if (d.cov_names.size() > 6) throw Failure{INQ_EXIT_PANIC, "at most 6 covariates"};
    Lines ph;
    if (!ph.open(a->phenocovar)) throw Failure{INQ_EXIT_PANIC, "Problem opening file"};
    std::string line;
    if (!ph.next(line)) throw Failure{INQ_EXIT_PANIC, "the phenotype file is empty"};
    const auto head = split_on(line, '\t');
    auto column_of = [&](const std::string &name, const char *what) {
        for (size_t c = 1; c < head.size(); ++c)
            if (head[c] == name) return c;
        throw Failure{INQ_EXIT_PANIC, std::string("The ") + what + " " + name + " is not a column in the phenotype file."};
    };
    const size_t pcol = column_of(a->phenotype, "phenotype variable");
    std::vector<size_t> ccol;
    for (const auto &c : d.cov_names) ccol.push_back(column_of(c, "covariate"));
    // per listed sample (the first line of a sample counts): usable, y, covariates
    struct Pheno {
        bool usable;
        double y;
        double cov[6];
    };
    std::unordered_map<std::string, Pheno> listed;
    while (ph.next(line)) {
        if (line.empty()) continue;
        const auto f = split_on(line, '\t');
        Pheno p{};
        p.usable = pcol < f.size();
        if (p.usable) {
            if (a->outcome == INQ_ASSOC_BINARY) {
                p.usable = f[pcol] == d.group1 || f[pcol] == d.group2;
                p.y = f[pcol] == d.group2 ? 1.0 : 0.0;
            } else {
                p.usable = parse_finite(f[pcol], &p.y);
            }
        }
        for (size_t j = 0; p.usable && j < ccol.size(); ++j) p.usable = ccol[j] < f.size() && parse_finite(f[ccol[j]], &p.cov[j]);
        listed.emplace(f[0], p);
    }
    std::vector<std::pair<size_t, size_t>> fld;
    split_tabs(header, fld);
    if (fld.size() < 3) throw Failure{INQ_EXIT_PANIC, "the combined file's header has fewer than three columns"};
    d.file_columns = fld.size() - 3;
    if (d.file_columns % 2) throw Failure{INQ_EXIT_PANIC, "the combined file's sample columns do not come in H1 / H2 pairs"};
    std::vector<const Pheno *> chosen;
    for (size_t s = 0; s < d.file_columns / 2; ++s) {
        const std::string h1 = strip_hap(header.substr(fld[3 + 2 * s].first, fld[3 + 2 * s].second));
        const std::string h2 = strip_hap(header.substr(fld[4 + 2 * s].first, fld[4 + 2 * s].second));
        if (h1 != h2) throw Failure{INQ_EXIT_PANIC, "the combined file's sample columns do not come in H1 / H2 pairs: " + h1 + ", " + h2};
        const auto it = listed.find(h1);
        if (it == listed.end() || !it->second.usable) continue;
        d.names.push_back(h1);
        d.column.push_back((uint32_t)s);
        chosen.push_back(&it->second);
    }
    const size_t n = d.names.size();
    if (n < 2)  // src/assoc.rs:35-45
        throw Failure{INQ_EXIT_PANIC, std::string("Not enough samples in ") + a->phenocovar + " matching " + a->phenotype};
    if (n > 65535) throw Failure{INQ_EXIT_ERROR, "more than 65535 samples are not supported"};
    d.y.resize(n);
    d.cov.resize(d.cov_names.size() * n);
    for (size_t i = 0; i < n; ++i) {
        d.y[i] = chosen[i]->y;
        for (size_t j = 0; j < d.cov_names.size(); ++j) d.cov[j * n + i] = chosen[i]->cov[j];
    }
    return d;
}

const char *const kStatusNames[] = {"OK", "LOW_CALL_RATE", "CONSTANT", "ONE_GROUP", "TOO_FEW", "SINGULAR", "NOT_CONVERGED"};
const char *status_name(uint32_t status) { return kStatusNames[status < 7 ? status : INQ_ASSOC_ROW_SINGULAR]; }
bool tested(const inq_assoc_row_t &w) { return w.status == INQ_ASSOC_ROW_OK || w.status == INQ_ASSOC_ROW_NOT_CONVERGED; }

// the loci asked for (--chr, --chr-begin / --chr-end), in file order
std::vector<size_t> pick_loci(const inq_assoc_args_t *a, const CombinedText &txt) {
    const std::string want_chr = a->chr ? a->chr : "";
    std::vector<size_t> picked;
    picked.reserve(txt.loci());
    for (size_t i = 0; i < txt.loci(); ++i) {
        if (txt.begin(i) == txt.end(i)) continue;  // an empty line
        Span c[3];
        if (!first_three(txt.begin(i), txt.end(i), c)) throw Failure{INQ_EXIT_PANIC, "index out of bounds: a line with fewer than three fields"};
        if (a->chr) {
            if (c[0].n != want_chr.size() || std::memcmp(c[0].p, want_chr.data(), want_chr.size()) != 0) continue;
            if (a->chr_begin >= 0) {
                double b = 0, e = 0;
                if (!parse_finite(std::string(c[1].p, c[1].n), &b) || !parse_finite(std::string(c[2].p, c[2].n), &e))
                    throw Failure{INQ_EXIT_PANIC, "Failed to parse number"};
                if (!(b >= (double)a->chr_begin && e <= (double)a->chr_end)) continue;
            }
        }
        picked.push_back(i);
    }
    return picked;
}

// [picked.size()][2 * samples]: the H1 / H2 pairs of the analysed samples, parsed by several threads.  Every value of a line is
// parsed, as the reference does (src/assoc.rs:82), also those of samples that are not analysed.
std::unique_ptr<float[]> fill_matrix(const CombinedText &txt, const std::vector<size_t> &picked, const Design &d) {
    const size_t ns = d.names.size(), n_rows = picked.size();
    // value column -> where it goes in a row of the matrix (-1: a sample that is not analysed)
    std::vector<int32_t> dest(d.file_columns, -1);
    for (size_t i = 0; i < ns; ++i) dest[2 * d.column[i]] = (int32_t)(2 * i), dest[2 * d.column[i] + 1] = (int32_t)(2 * i + 1);
    std::unique_ptr<float[]> mat(new float[std::max<size_t>(n_rows * 2 * ns, 1)]);
    const size_t n_thr = thread_count(n_rows, kLinesPerThread);
    std::vector<std::string> bad(n_thr);
    on_threads(n_thr, [&](size_t t) {
        const size_t lo = n_rows * t / n_thr, hi = n_rows * (t + 1) / n_thr;
        for (size_t r = lo; r < hi; ++r) {
            float *row = mat.get() + r * 2 * ns;
            const size_t fields = walk_values(txt.begin(picked[r]), txt.end(picked[r]), [row, to = dest.data(), n_dest = dest.size()](size_t k, const char *s, size_t n) {  // (captured by value: they stay in registers)
                if (k >= n_dest) return true;
                float v;
                if (!parse_f32(s, n, &v)) return false;
                if (to[k] >= 0) row[to[k]] = v;
                return true;
            });
            if (fields == kWalkStopped) bad[t] = "Failed to parse number";
            else if (fields < 3 + dest.size()) bad[t] = "a line with fewer values than the header has sample columns";
            if (!bad[t].empty()) return;
        }
    });
    for (const auto &b : bad)
        if (!b.empty()) throw Failure{INQ_EXIT_PANIC, b};
    return mat;
}

// The regressions.  --firth: the same rows, and beside them Firth's fit of the ones the device picks (firth stays empty without)
void fit_rows(inq_ctx_t *ctx, const inq_assoc_args_t *a, const Design &d, const float *mat, std::vector<inq_assoc_row_t> &rows,
              std::vector<inq_assoc_firth_row_t> &firth) {
    const uint32_t ns = (uint32_t)d.names.size(), k = (uint32_t)d.cov_names.size();
    int rc;
    if (a->firth != INQ_HOST_FIRTH_NO) {
        firth.resize(rows.size());
        rc = inq_assoc_rows_firth(ctx, mat, rows.size(), ns, d.y.data(), d.cov.data(), k, a->str_mode, a->missing_cutoff,
                                  a->firth == INQ_HOST_FIRTH_ALWAYS ? INQ_ASSOC_FIRTH_ALWAYS : INQ_ASSOC_FIRTH_FALLBACK, rows.data(), firth.data());
    } else {
        rc = inq_assoc_rows(ctx, mat, rows.size(), ns, d.y.data(), d.cov.data(), k, a->outcome, a->str_mode, a->missing_cutoff, rows.data());
    }
    if (rc != INQ_OK) device_call_failed(rc, ctx);
}

// what a row prints as beta, se and p: its Firth fit's where that is there and OK, else the ordinary fit's
struct Printed {
    double beta, se, p;
    bool firth;
};
Printed printed(const std::vector<inq_assoc_row_t> &rows, const std::vector<inq_assoc_firth_row_t> &firth, size_t r) {
    if (!firth.empty() && firth[r].status == INQ_ASSOC_FIRTH_ROW_OK) return Printed{firth[r].beta, firth[r].se, firth[r].p, true};
    return Printed{rows[r].beta, rows[r].se, rows[r].p, false};
}

// tested rows by ascending printed p (a NaN behind every number), ties in file order; then, with all_rows, the others in file order
std::vector<size_t> print_order(bool all_rows, const std::vector<inq_assoc_row_t> &rows, const std::vector<inq_assoc_firth_row_t> &firth) {
    std::vector<size_t> order;
    for (size_t r = 0; r < rows.size(); ++r)
        if (tested(rows[r])) order.push_back(r);
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) {
        const double px = printed(rows, firth, x).p, py = printed(rows, firth, y).p;
        if (std::isnan(px) || std::isnan(py)) return !std::isnan(px) && std::isnan(py);
        return px < py;
    });
    if (all_rows)
        for (size_t r = 0; r < rows.size(); ++r)
            if (!tested(rows[r])) order.push_back(r);
    return order;
}

// the header and one line per row of `order`
void print_table(const inq_assoc_args_t *a, const Design &d, const CombinedText &txt, const std::vector<size_t> &picked,
                 const std::vector<size_t> &order, const std::vector<inq_assoc_row_t> &rows, const std::vector<inq_assoc_firth_row_t> &firth,
                 OutBuffer &out) {
    const bool binary = a->outcome == INQ_ASSOC_BINARY, firth_on = a->firth != INQ_HOST_FIRTH_NO;
    std::string model = std::string(a->phenotype) + "~x";
    for (const auto &c : d.cov_names) model += "+" + c;
    if (binary) {
        const std::string &A = d.group1, &B = d.group2;
        out.text = "VariantID\tOR\tOR_L95\tOR_U95\tOR_stdErr\tPvalue\tN\t" + A + "_N\t" + B + "_N\tAvgSize\t" + A + "_AvgSize\t" + B + "_AvgSize\t" + B +
                   "_" + A + "_absAvgSizeDiff\t" + B + "_" + A + "_OR_for_absAvgSizeDiff\tmodel\tbinaryOrder";
    } else {
        out.text = "VariantID\tBeta\tBeta_L95\tBeta_U95\tBeta_stdErr\tPvalue\tN\tAvgSize\tMinSize\tMaxSize\tMax_Min_absSizeDiff\tMax_Min_Beta_for_absSizeDiff\tmodel";
    }
    if (a->all_rows) out.text += "\tstatus";
    out.text += firth_on ? "\tmethod\n" : "\n";
    auto num = [&](double v) {
        inqhost::append_f64(out.text, v);
        out.text += '\t';
    };
    auto count = [&](uint32_t v) {
        out.text += std::to_string(v);
        out.text += '\t';
    };
    constexpr double z95 = 1.959963984540054;
    for (size_t r : order) {
        const inq_assoc_row_t &w = rows[r];
        Span c[3];  // VariantID = chrom:begin_end, as the file spells them
        first_three(txt.begin(picked[r]), txt.end(picked[r]), c);
        out.text.append(c[0].p, c[0].n), out.text += ':';
        out.text.append(c[1].p, c[1].n), out.text += '_';
        out.text.append(c[2].p, c[2].n), out.text += '\t';
        const Printed f = printed(rows, firth, r);
        const double lo = f.beta - z95 * f.se, hi = f.beta + z95 * f.se;
        if (binary) {
            const double diff = std::fabs(w.mean_g2 - w.mean_g1);
            num(std::exp(f.beta)), num(std::exp(lo)), num(std::exp(hi)), num(f.se), num(f.p);
            count(w.n), count(w.n_g1), count(w.n_g2);
            num(w.mean_all), num(w.mean_g1), num(w.mean_g2), num(diff), num(std::exp(diff * f.beta));
            out.text += model + "\t" + d.group1 + "," + d.group2;
        } else {
            const double diff = std::fabs(w.max_x - w.min_x);
            num(w.beta), num(lo), num(hi), num(w.se), num(w.p);
            count(w.n);
            num(w.mean_all), num(w.min_x), num(w.max_x), num(diff), num(diff * w.beta);
            out.text += model;
        }
        if (a->all_rows) out.text += std::string("\t") + status_name(w.status);
        if (firth_on) out.text += f.firth ? "\tfirth" : "\tglm";
        out.text += '\n';
        out.line_done();
    }
}

// the line on stderr: how many loci ended in each status, and how many print Firth's fit
std::string tally(const Design &d, const std::vector<inq_assoc_row_t> &rows, const std::vector<inq_assoc_firth_row_t> &firth, bool firth_on) {
    size_t per_status[7] = {0, 0, 0, 0, 0, 0, 0}, n_firth = 0;
    for (size_t r = 0; r < rows.size(); ++r) {
        ++per_status[rows[r].status < 7 ? rows[r].status : INQ_ASSOC_ROW_SINGULAR];
        n_firth += printed(rows, firth, r).firth;
    }
    std::string line = "[inq assoc] " + std::to_string(rows.size()) + " loci, " + std::to_string(d.names.size()) + " samples:";
    for (int s = 0; s < 7; ++s) line += std::string(" ") + kStatusNames[s] + " " + std::to_string(per_status[s]);
    if (firth_on) line += "; fitted by Firth " + std::to_string(n_firth);
    return line;
}

int assoc_impl(const inq_assoc_args_t *a, int out_fd) {
    check_args(a);
    BackgroundCtx device(a->device);
    const Laps lap{"assoc"};
    CombinedText txt;
    txt.read(a->combined);
    lap("text in memory");
    txt.split();
    const Design d = make_design(a, txt.header());
    const std::vector<size_t> picked = pick_loci(a, txt);
    const std::unique_ptr<float[]> mat = fill_matrix(txt, picked, d);
    lap("numbers parsed");
    inq_ctx_t *ctx = device.wait(lap);
    std::vector<inq_assoc_row_t> rows(picked.size());
    std::vector<inq_assoc_firth_row_t> firth;
    fit_rows(ctx, a, d, mat.get(), rows, firth);
    lap("kernels done");
    OutBuffer out{out_fd, ""};
    print_table(a, d, txt, picked, print_order(a->all_rows != 0, rows, firth), rows, firth, out);
    out.flush();
    std::fprintf(stderr, "%s\n", tally(d, rows, firth, a->firth != INQ_HOST_FIRTH_NO).c_str());
    return INQ_EXIT_OK;
}

int assoc_samples_impl(const inq_assoc_args_t *args, char *names, size_t names_cap, double *y, double *cov, size_t cap, uint32_t *n_samples,
                       uint32_t *k) {
    check_args(args);
    Lines in;
    std::string header;
    if (!in.open(args->combined)) throw Failure{INQ_EXIT_PANIC, "Problem opening file"};
    if (!in.next(header)) throw Failure{INQ_EXIT_PANIC, "called `Option::unwrap()` on a `None` value (empty combined file)"};
    const Design d = make_design(args, header);
    std::string joined;
    for (size_t i = 0; i < d.names.size(); ++i) joined += (i ? "," : "") + d.names[i];
    if (names && names_cap) std::snprintf(names, names_cap, "%s", joined.c_str());
    if (n_samples) *n_samples = (uint32_t)d.names.size();
    if (k) *k = (uint32_t)d.cov_names.size();
    if (cap >= d.names.size()) {
        if (y) std::copy(d.y.begin(), d.y.end(), y);
        if (cov) std::copy(d.cov.begin(), d.cov.end(), cov);
    }
    return INQ_EXIT_OK;
}

}  // namespace

extern "C" int inq_assoc(const inq_assoc_args_t *args, int out_fd, char *errbuf, size_t errcap) {
    INQ_GUARD(assoc_impl(args, out_fd), errbuf, errcap)
}

extern "C" int inq_assoc_samples(const inq_assoc_args_t *args, char *names, size_t names_cap, double *y, double *cov, size_t cap,
                                 uint32_t *n_samples, uint32_t *k, char *errbuf, size_t errcap) {
    INQ_GUARD(assoc_samples_impl(args, names, names_cap, y, cov, cap, n_samples, k), errbuf, errcap)
}
