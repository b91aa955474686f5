// assoc.cc — `inquistr assoc` (the reference's scripts/STR_regression.R): reads a combined .inq and a phenotype
// file, hands the H1 / H2 pairs of the analysed samples of all loci to the GPU in one matrix (inq_assoc_rows) and prints the tested
// loci by ascending p-value.  With --firth the rows whose fit separation broke print Firth's fit (inq_assoc_rows_firth) in its place.
// Text in, text out; the regressions are not here.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <memory>
#include <string>
#include <thread>
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

struct Failure {
    int status;
    std::string message;
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

int assoc_impl(const inq_assoc_args_t *a, int out_fd) {
    check_args(a);
    // the HIP runtime starts while the text is read and parsed (as in outlier.cc)
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
    using clk = std::chrono::steady_clock;
    const bool timing = std::getenv("INQ_TIMING") != nullptr;
    const auto t_begin = clk::now();
    auto lap = [&](const char *what) {
        if (timing) std::fprintf(stderr, "[inq assoc] %-22s at %7.1f ms\n", what, std::chrono::duration<double, std::milli>(clk::now() - t_begin).count());
    };
    TextFile tf;
    {
        std::string lerr;
        if (!tf.load(a->combined, lerr)) throw Failure{INQ_EXIT_PANIC, lerr};
    }
    const char *const tdata = tf.data;
    lap("text in memory");
    std::vector<std::pair<size_t, size_t>> lines;
    find_lines(tdata, tf.size, lines);
    if (lines.empty()) throw Failure{INQ_EXIT_PANIC, "called `Option::unwrap()` on a `None` value (empty combined file)"};  // src/assoc.rs:49
    const Design d = make_design(a, std::string(tdata + lines[0].first, lines[0].second));
    const size_t ns = d.names.size(), k = d.cov_names.size();
    // value column -> where it goes in a row of the matrix (-1: a sample that is not analysed)
    std::vector<int32_t> dest(d.file_columns, -1);
    for (size_t i = 0; i < ns; ++i) dest[2 * d.column[i]] = (int32_t)(2 * i), dest[2 * d.column[i] + 1] = (int32_t)(2 * i + 1);

    // the loci asked for (--chr, --chr-begin / --chr-end), in file order
    const size_t n_lines = lines.size() - 1;
    const std::string want_chr = a->chr ? a->chr : "";
    std::vector<size_t> picked;  // line numbers
    picked.reserve(n_lines);
    for (size_t i = 0; i < n_lines; ++i) {
        const char *p = tdata + lines[i + 1].first, *end = p + lines[i + 1].second;
        if (p == end) continue;  // an empty line
        const char *t1 = (const char *)std::memchr(p, '\t', (size_t)(end - p));
        const char *t2 = t1 ? (const char *)std::memchr(t1 + 1, '\t', (size_t)(end - t1 - 1)) : nullptr;
        const char *t3 = t2 ? (const char *)std::memchr(t2 + 1, '\t', (size_t)(end - t2 - 1)) : nullptr;
        if (!t2) throw Failure{INQ_EXIT_PANIC, "index out of bounds: a line with fewer than three fields"};
        if (a->chr) {
            if ((size_t)(t1 - p) != want_chr.size() || std::memcmp(p, want_chr.data(), want_chr.size()) != 0) continue;
            if (a->chr_begin >= 0) {
                double b = 0, e = 0;
                if (!parse_finite(std::string(t1 + 1, t2), &b) || !parse_finite(std::string(t2 + 1, t3 ? t3 : end), &e))
                    throw Failure{INQ_EXIT_PANIC, "Failed to parse number"};
                if (!(b >= (double)a->chr_begin && e <= (double)a->chr_end)) continue;
            }
        }
        picked.push_back(i + 1);
    }
    const size_t n_rows = picked.size();
    std::unique_ptr<float[]> mat_mem(new float[std::max<size_t>(n_rows * 2 * ns, 1)]);
    float *const mat = mat_mem.get();
    const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    const size_t n_thr = std::max<size_t>(1, std::min<size_t>(hw, n_rows / 2048 + 1));
    std::vector<std::string> bad(n_thr);
    auto work = [&](size_t t) {
        const size_t lo = n_rows * t / n_thr, hi = n_rows * (t + 1) / n_thr;
        for (size_t r = lo; r < hi; ++r) {
            const char *p = tdata + lines[picked[r]].first, *end = p + lines[picked[r]].second;
            float *row = mat + r * 2 * ns;
            size_t field = 0;
            const char *f0 = p;
            for (const char *q = p;; ++q) {
                if (q == end || *q == '\t') {
                    if (field >= 3 && field - 3 < dest.size()) {
                        float v;
                        if (!parse_f32(f0, (size_t)(q - f0), &v)) {  // src/assoc.rs:82
                            bad[t] = "Failed to parse number";
                            return;
                        }
                        if (dest[field - 3] >= 0) row[dest[field - 3]] = v;
                    }
                    ++field;
                    f0 = q + 1;
                    if (q == end) break;
                }
            }
            if (field < 3 + dest.size()) {
                bad[t] = "a line with fewer values than the header has sample columns";
                return;
            }
        }
    };
    {
        std::vector<std::thread> th;
        for (size_t t = 1; t < n_thr; ++t) th.emplace_back(work, t);
        work(0);
        for (auto &x : th) x.join();
    }
    for (const auto &b : bad)
        if (!b.empty()) throw Failure{INQ_EXIT_PANIC, b};
    lap("numbers parsed");
    ctx_thread.join();
    lap("device context there");
    if (hrc != INQ_OK) throw Failure{INQ_EXIT_ERROR, std::string("cannot open HIP device: ") + inq_strerror(hrc)};
    std::vector<inq_assoc_row_t> rows(n_rows);
    // --firth: the same rows, and beside them Firth's fit of the ones the device picks
    const bool firth_on = a->firth != INQ_HOST_FIRTH_NO;
    std::vector<inq_assoc_firth_row_t> firth(firth_on ? n_rows : 0);
    if (firth_on)
        hrc = inq_assoc_rows_firth(ctx, mat, n_rows, (uint32_t)ns, d.y.data(), d.cov.data(), (uint32_t)k, a->str_mode, a->missing_cutoff,
                                   a->firth == INQ_HOST_FIRTH_ALWAYS ? INQ_ASSOC_FIRTH_ALWAYS : INQ_ASSOC_FIRTH_FALLBACK, rows.data(), firth.data());
    else
        hrc = inq_assoc_rows(ctx, mat, n_rows, (uint32_t)ns, d.y.data(), d.cov.data(), (uint32_t)k, a->outcome, a->str_mode, a->missing_cutoff,
                             rows.data());
    if (hrc != INQ_OK) {
        const std::string detail = hrc == INQ_ERR_HIP ? inq_last_error(ctx) : "";
        throw Failure{INQ_EXIT_ERROR, std::string("device call failed: ") + inq_strerror(hrc) + (detail.empty() ? "" : " [" + detail + "]")};
    }
    lap("kernels done");

    // what a row prints as beta, se and p: its Firth fit's where that is there and OK, else the ordinary fit's
    struct Printed {
        double beta, se, p;
        bool firth;
    };
    auto printed = [&](size_t r) {
        if (firth_on && firth[r].status == INQ_ASSOC_FIRTH_ROW_OK) return Printed{firth[r].beta, firth[r].se, firth[r].p, true};
        return Printed{rows[r].beta, rows[r].se, rows[r].p, false};
    };
    // tested rows by ascending printed p (a NaN behind every number), ties in file order; then, with all_rows, the others in file order
    std::vector<size_t> order;
    size_t per_status[7] = {0, 0, 0, 0, 0, 0, 0}, n_firth = 0;
    for (size_t r = 0; r < n_rows; ++r) {
        ++per_status[rows[r].status < 7 ? rows[r].status : INQ_ASSOC_ROW_SINGULAR];
        if (rows[r].status == INQ_ASSOC_ROW_OK || rows[r].status == INQ_ASSOC_ROW_NOT_CONVERGED) order.push_back(r);
        n_firth += printed(r).firth;
    }
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) {
        const double px = printed(x).p, py = printed(y).p;
        if (std::isnan(px) || std::isnan(py)) return !std::isnan(px) && std::isnan(py);
        return px < py;
    });
    if (a->all_rows)
        for (size_t r = 0; r < n_rows; ++r)
            if (rows[r].status != INQ_ASSOC_ROW_OK && rows[r].status != INQ_ASSOC_ROW_NOT_CONVERGED) order.push_back(r);
    const bool binary = a->outcome == INQ_ASSOC_BINARY;
    std::string model = std::string(a->phenotype) + "~x";
    for (const auto &c : d.cov_names) model += "+" + c;
    std::string out;
    if (binary) {
        const std::string &A = d.group1, &B = d.group2;
        out = "VariantID\tOR\tOR_L95\tOR_U95\tOR_stdErr\tPvalue\tN\t" + A + "_N\t" + B + "_N\tAvgSize\t" + A + "_AvgSize\t" + B + "_AvgSize\t" + B +
              "_" + A + "_absAvgSizeDiff\t" + B + "_" + A + "_OR_for_absAvgSizeDiff\tmodel\tbinaryOrder";
    } else {
        out = "VariantID\tBeta\tBeta_L95\tBeta_U95\tBeta_stdErr\tPvalue\tN\tAvgSize\tMinSize\tMaxSize\tMax_Min_absSizeDiff\tMax_Min_Beta_for_absSizeDiff\tmodel";
    }
    if (a->all_rows) out += "\tstatus";
    out += firth_on ? "\tmethod\n" : "\n";
    auto num = [&](double v) {
        inqhost::append_f64(out, v);
        out += '\t';
    };
    auto count = [&](uint32_t v) {
        out += std::to_string(v);
        out += '\t';
    };
    constexpr double z95 = 1.959963984540054;
    for (size_t r : order) {
        const inq_assoc_row_t &w = rows[r];
        {  // VariantID = chrom:begin_end, as the file spells them
            const char *p = tdata + lines[picked[r]].first, *end = p + lines[picked[r]].second;
            const char *t1 = (const char *)std::memchr(p, '\t', (size_t)(end - p));
            const char *t2 = (const char *)std::memchr(t1 + 1, '\t', (size_t)(end - t1 - 1));
            const char *t3 = (const char *)std::memchr(t2 + 1, '\t', (size_t)(end - t2 - 1));
            out.append(p, t1);
            out += ':';
            out.append(t1 + 1, t2);
            out += '_';
            out.append(t2 + 1, t3 ? t3 : end);
            out += '\t';
        }
        const Printed f = printed(r);
        const double lo = f.beta - z95 * f.se, hi = f.beta + z95 * f.se;
        if (binary) {
            const double diff = std::fabs(w.mean_g2 - w.mean_g1);
            num(std::exp(f.beta)), num(std::exp(lo)), num(std::exp(hi)), num(f.se), num(f.p);
            count(w.n), count(w.n_g1), count(w.n_g2);
            num(w.mean_all), num(w.mean_g1), num(w.mean_g2), num(diff), num(std::exp(diff * f.beta));
            out += model + "\t" + d.group1 + "," + d.group2;
        } else {
            const double diff = std::fabs(w.max_x - w.min_x);
            num(w.beta), num(lo), num(hi), num(w.se), num(w.p);
            count(w.n);
            num(w.mean_all), num(w.min_x), num(w.max_x), num(diff), num(diff * w.beta);
            out += model;
        }
        if (a->all_rows) out += std::string("\t") + kStatusNames[w.status < 7 ? w.status : INQ_ASSOC_ROW_SINGULAR];
        if (firth_on) out += f.firth ? "\tfirth" : "\tglm";
        out += '\n';
        if (out.size() > (1u << 20)) {
            if (!write_all(out_fd, out)) return INQ_EXIT_PANIC;
            out.clear();
        }
    }
    if (!write_all(out_fd, out)) return INQ_EXIT_PANIC;
    std::string tally = "[inq assoc] " + std::to_string(n_rows) + " loci, " + std::to_string(ns) + " samples:";
    for (int s = 0; s < 7; ++s) tally += std::string(" ") + kStatusNames[s] + " " + std::to_string(per_status[s]);
    if (firth_on) tally += "; fitted by Firth " + std::to_string(n_firth);
    std::fprintf(stderr, "%s\n", tally.c_str());
    return INQ_EXIT_OK;
}

template <class F> int reported(char *errbuf, size_t errcap, F &&body) {
    try {
        return body();
    } catch (const Failure &f) {
        set_err(errbuf, errcap, f.message);
        return f.status;
    } catch (const std::exception &e) {
        set_err(errbuf, errcap, std::string("internal error: ") + e.what());
        return INQ_EXIT_ERROR;
    } catch (...) {
        set_err(errbuf, errcap, "internal error");
        return INQ_EXIT_ERROR;
    }
}

}  // namespace

extern "C" int inq_assoc(const inq_assoc_args_t *args, int out_fd, char *errbuf, size_t errcap) {
    return reported(errbuf, errcap, [&] { return assoc_impl(args, out_fd); });
}

extern "C" int inq_assoc_samples(const inq_assoc_args_t *args, char *names, size_t names_cap, double *y, double *cov, size_t cap,
                                 uint32_t *n_samples, uint32_t *k, char *errbuf, size_t errcap) {
    return reported(errbuf, errcap, [&] {
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
    });
}
