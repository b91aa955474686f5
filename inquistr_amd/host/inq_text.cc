#include "inq_text.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace inqhost {

// decimal digits of a non-negative integer, appended
static void append_u64(std::string &out, uint64_t v) {
    char buf[24];
    int n = 0;
    do {
        buf[n++] = (char)('0' + v % 10);
        v /= 10;
    } while (v);
    while (n) out.push_back(buf[--n]);
}

// Rust's `{}` for f64 restricted to what the path produces: NaN, integers and halves ((a + b) as f64 / 2.0,
// src/call.rs:518) of at most 2^53 in magnitude take the fast path; anything else goes the general way below
void append_f64(std::string &out, double v) {
    if (std::isnan(v)) {
        out += "NaN";
        return;
    }
    const double a = std::fabs(v);
    if (a < 9007199254740992.0) {
        const uint64_t twice = (uint64_t)(a * 2.0);
        if ((double)twice == a * 2.0) {  // an integer or a half
            if (std::signbit(v)) out.push_back('-');
            append_u64(out, twice >> 1);
            if (twice & 1u) out += ".5";
            return;
        }
    }
    // anything else - never produced by the path - as Rust's Display prints it [3P core::fmt::float]: the SHORTEST decimal digits that
    // read back as v, written out positionally (no exponent; 2^60 is "1152921504606847000", not its exact digits), "inf", "-0"
    if (std::isinf(v)) {
        out += v < 0 ? "-inf" : "inf";
        return;
    }
    char e[40];
    int prec = 0;
    for (; prec <= 16; ++prec) {
        std::snprintf(e, sizeof e, "%.*e", prec, a);
        if (std::strtod(e, nullptr) == a) break;
    }
    if (prec > 16) std::snprintf(e, sizeof e, "%.16e", a);
    std::string digits;
    int exp10 = 0;
    for (const char *q = e; *q; ++q) {
        if (*q >= '0' && *q <= '9') digits.push_back(*q);
        else if (*q == 'e') {
            exp10 = std::atoi(q + 1);
            break;
        }
    }
    while (digits.size() > 1 && digits.back() == '0') digits.pop_back();
    if (std::signbit(v)) out.push_back('-');
    const int nd = (int)digits.size();
    if (exp10 >= nd - 1) {
        out += digits;
        out.append((size_t)(exp10 - (nd - 1)), '0');
    } else if (exp10 >= 0) {
        out.append(digits, 0, (size_t)exp10 + 1);
        out.push_back('.');
        out.append(digits, (size_t)exp10 + 1, std::string::npos);
    } else {
        out += "0.";
        out.append((size_t)(-exp10 - 1), '0');
        out += digits;
    }
}

std::string format_f64(double v) {
    std::string s;
    append_f64(s, v);
    return s;
}

void append_row(std::string &out, const std::string &chrom, uint32_t start, uint32_t end, double p1, double p2) {
    out += chrom;
    out.push_back('\t');
    append_u64(out, start);
    out.push_back('\t');
    append_u64(out, end);
    out.push_back('\t');
    append_f64(out, p1);
    out.push_back('\t');
    append_f64(out, p2);
}

// the same text through a bare pointer (the output stage formats 10^5 .. 10^6 rows): dst must hold row_capacity(chrom) bytes
static inline char *put_u64(char *p, uint64_t v) {
    char buf[24];
    int n = 0;
    do {
        buf[n++] = (char)('0' + v % 10);
        v /= 10;
    } while (v);
    while (n) *p++ = buf[--n];
    return p;
}
static inline char *put_f64(char *p, double v) {
    if (std::isnan(v)) {
        *p++ = 'N', *p++ = 'a', *p++ = 'N';
        return p;
    }
    const double a = std::fabs(v);
    if (a < 9007199254740992.0) {
        const uint64_t twice = (uint64_t)(a * 2.0);
        if ((double)twice == a * 2.0) {
            if (std::signbit(v)) *p++ = '-';
            p = put_u64(p, twice >> 1);
            if (twice & 1u) *p++ = '.', *p++ = '5';
            return p;
        }
    }
    std::string s;
    append_f64(s, v);  // the rare rest (not produced by the path): up to 1 + 309 digits + ".5"
    for (char c : s) *p++ = c;
    return p;
}
char *write_row(char *p, const std::string &chrom, uint32_t start, uint32_t end, double p1, double p2) {
    for (char c : chrom) *p++ = c;
    *p++ = '\t';
    p = put_u64(p, start);
    *p++ = '\t';
    p = put_u64(p, end);
    *p++ = '\t';
    p = put_f64(p, p1);
    *p++ = '\t';
    p = put_f64(p, p2);
    return p;
}

std::string format_row(const std::string &chrom, uint32_t start, uint32_t end, double p1, double p2) {
    std::string s;
    append_row(s, chrom, start, end, p1, p2);
    return s;
}

std::string format_header(const std::string &sample) {
    return "chromosome\tbegin\tend\t" + sample + "_H1\t" + sample + "_H2";
}

const char *const kEvidenceHeader = "chrom\tbegin\tend\tfetched\tkept\th1\th2\tclipped\tmin\tmax";

void append_evidence_row(std::string &out, const std::string &chrom, uint32_t start, uint32_t end, const inq_locus_evidence_t &e) {
    out += chrom;
    for (const uint32_t v : {start, end, e.n_fetched, e.n_kept, e.n_group1, e.n_group2, e.n_clip}) out += '\t', out += std::to_string(v);
    if ((uint64_t)e.n_group1 + e.n_group2 == 0)
        out += "\t.\t.";  // no Call behind either median: nothing to take extremes of
    else
        out += '\t', out += std::to_string(e.call_min), out += '\t', out += std::to_string(e.call_max);
}

const char *const kReadCallsHeader = "chrom\tbegin\tend\th1\th2\tother";

// one list of the file: the Calls comma-separated, a Clip with the suffix `c`; `.` for none
static void append_call_list(std::string &out, const inq_read_call_t *const *first, const inq_read_call_t *const *last) {
    out += '\t';
    if (first == last) out += '.';
    for (const inq_read_call_t *const *p = first; p != last; ++p) {
        if (p != first) out += ',';
        out += std::to_string((*p)->call);
        if ((*p)->flags & INQ_READ_CALL_CLIP) out += 'c';
    }
}

// the three lists of a target - h1, h2, other - from the records of its kept reads in file order, each list in the file's order
static void split_read_calls(const inq_read_call_t *calls, size_t n, bool unphased, std::vector<const inq_read_call_t *> (&g)[3]) {
    // ascending by (value, file order) - the records come in file order, so a stable sort by value: the tie rule of the reduces
    auto by_value = [](const inq_read_call_t *a, const inq_read_call_t *b) { return a->call < b->call; };
    for (size_t i = 0; i < n; ++i) g[unphased ? 0 : calls[i].group == 1 ? 0 : calls[i].group == 2 ? 1 : 2].push_back(calls + i);
    for (auto &v : g) std::stable_sort(v.begin(), v.end(), by_value);
    if (unphased) {  // src/call.rs:312-314: the sorted kept Calls are split at len / 2
        g[1].assign(g[0].begin() + n / 2, g[0].end());
        g[0].resize(n / 2);
    }
}

void append_read_calls_row(std::string &out, const std::string &chrom, uint32_t start, uint32_t end, const inq_read_call_t *calls, size_t n,
                           bool unphased) {
    out += chrom;
    for (const uint32_t v : {start, end}) out += '\t', out += std::to_string(v);
    std::vector<const inq_read_call_t *> g[3];  // h1, h2, other (`.` for an unphased call: the list is empty)
    split_read_calls(calls, n, unphased, g);
    for (const auto &v : g) append_call_list(out, v.data(), v.data() + v.size());
}

const char *const kReadTableHeader = "chrom\tbegin\tend\tgroup\tcall\tkind\tread\tpos\tstrand\tmapq";

// The lines of one target that name its kept reads, in the order of the read-calls lists: columns chrom .. read, then what `tail`
// appends for record k (it begins with its own tab), then the newline
template <class Tail>
static void append_read_lines(std::string &out, const std::string &chrom, uint32_t start, uint32_t end, const inq_read_call_t *calls,
                              const inq_read_origin_t *origins, const uint8_t *names, size_t n, bool unphased, Tail tail) {
    if (!n) return;
    std::vector<const inq_read_call_t *> g[3];
    split_read_calls(calls, n, unphased, g);
    std::vector<size_t> name_at(n + 1, 0);  // where record k's name begins
    for (size_t k = 0; k < n; ++k) name_at[k + 1] = name_at[k] + origins[k].name_len;
    const std::string locus = chrom + '\t' + std::to_string(start) + '\t' + std::to_string(end) + '\t';
    static const char *const kGroup[3] = {"h1", "h2", "other"};
    for (int q = 0; q < 3; ++q)
        for (const inq_read_call_t *rec : g[q]) {
            const size_t k = (size_t)(rec - calls);
            const inq_read_origin_t &o = origins[k];
            out += locus, out += kGroup[q], out += '\t', out += std::to_string(rec->call);
            out += (rec->flags & INQ_READ_CALL_CLIP) ? "\tClip\t" : "\tSpan\t";
            const char *name = (const char *)names + name_at[k];
            const size_t len = o.name_len ? ::strnlen(name, o.name_len) : 0;  // cut at the first NUL
            if (len) out.append(name, len);
            else out += '*';
            tail(out, k);
            out += '\n';
        }
}

void append_read_table_rows(std::string &out, const std::string &chrom, uint32_t start, uint32_t end, const inq_read_call_t *calls,
                            const inq_read_origin_t *origins, const uint8_t *names, size_t n, bool unphased) {
    append_read_lines(out, chrom, start, end, calls, origins, names, n, unphased, [origins](std::string &o_, size_t k) {
        const inq_read_origin_t &o = origins[k];
        o_ += '\t', o_ += std::to_string((int64_t)o.pos + 1);  // SAM POS
        o_ += (o.bits & INQ_READ_REVERSE) ? "\t-\t" : "\t+\t";
        o_ += std::to_string((unsigned)o.mapq);
    });
}

const char *const kReadSeqsHeader = "chrom\tbegin\tend\tgroup\tcall\tkind\tread\tqbeg\tlen\tseq";

void append_read_seq_rows(std::string &out, const std::string &chrom, uint32_t start, uint32_t end, const inq_read_call_t *calls,
                          const inq_read_origin_t *origins, const uint8_t *names, const inq_read_seq_t *seqs, const uint8_t *packed, size_t n,
                          bool unphased) {
    std::vector<size_t> seq_at(n + 1, 0);  // where record k's packed slice begins
    for (size_t k = 0; k < n; ++k) seq_at[k + 1] = seq_at[k] + ((size_t)seqs[k].n_bases + 1) / 2;
    append_read_lines(out, chrom, start, end, calls, origins, names, n, unphased, [&](std::string &o_, size_t k) {
        static const char kCodes[] = "=ACMGRSVTWYHKDBN";  // the BAM's 4-bit codes
        const inq_read_seq_t &q = seqs[k];
        o_ += '\t', o_ += std::to_string(q.q_beg), o_ += '\t', o_ += std::to_string(q.n_bases), o_ += '\t';
        if (!q.n_bases) o_ += '*';
        const uint8_t *b = packed + seq_at[k];
        for (uint32_t i = 0; i < q.n_bases; ++i) o_ += kCodes[(b[i >> 1] >> ((~i & 1u) * 4u)) & 15u];
    });
}

void seq_window(const uint32_t *cigar, uint32_t n_cigar, int32_t pos, uint32_t l_seq, uint32_t start, uint32_t end, uint32_t *q_beg,
                   uint32_t *n_bases) {
    *q_beg = *n_bases = 0;
    const uint32_t se = start - 10u, ee = end + 10u;  // u32, as the locus kernels build the window
    if ((int64_t)ee - 1 <= (int64_t)se) return;       // width 0 (empty or wrapped), and start = 9
    const int64_t x[2] = {(int64_t)se, (int64_t)ee - 1};
    uint64_t q[2] = {0, 0}, query = 0;  // query: the cursor in front of the op
    bool past[2] = {false, false};
    int64_t r = pos;
    // one op at a time, as call_from_cigar walks: Q(x) is the query cursor when the reference cursor reaches x, or - x lying inside an
    // M - that many bases into it; an insertion or clip AT x (r_op == x) lies behind it
    for (uint32_t i = 0; i < n_cigar; ++i) {
        const uint32_t op = cigar[i] & 15u;
        const uint64_t len = cigar[i] >> 4;
        const bool in_query = op == 0 || op == 1 || op == 4 || op == 7 || op == 8, in_ref = op == 0 || op == 2 || op == 3 || op == 7 || op == 8;
        for (int w = 0; w < 2; ++w) {
            if (past[w]) continue;
            if (r >= x[w]) {  // the cursor has reached x in front of this op: nothing from here on lies in front of x
                q[w] = query, past[w] = true;
            } else if (in_ref && in_query && r + (int64_t)len > x[w]) {
                q[w] = query + (uint64_t)(x[w] - r), past[w] = true;
            }
        }
        if (past[0] && past[1]) break;
        if (in_query) query += len;
        if (in_ref) r += (int64_t)len;
    }
    for (int w = 0; w < 2; ++w) {
        if (!past[w]) q[w] = query;  // the read ends in front of x: all of it
        if (q[w] > l_seq) q[w] = l_seq;
    }
    *q_beg = (uint32_t)q[0];
    *n_bases = (uint32_t)(q[1] - q[0]);
}

void pack_seq_slice(const uint8_t *seq, uint32_t q_beg, uint32_t n_bases, std::vector<uint8_t> &out) {
    auto base = [&](uint32_t k) -> uint8_t { return (seq[k >> 1] >> ((~k & 1u) * 4u)) & 15u; };
    for (uint32_t i = 0; i < n_bases; i += 2)
        out.push_back((uint8_t)(base(q_beg + i) << 4 | (i + 1 < n_bases ? base(q_beg + i + 1) : 0)));
}

// k and the k codes of a motif word; k = 0: no motif
static uint32_t motif_codes(uint64_t word, uint8_t (&m)[15]) {
    const uint32_t k = (uint32_t)(word >> 60);
    for (uint32_t i = 0; i < k; ++i) {
        m[i] = (uint8_t)(word >> (4u * i) & 15u);
        if (m[i] != 1 && m[i] != 2 && m[i] != 4 && m[i] != 8) return 0;
    }
    return k;
}

int motif_encode(const char *text, uint64_t *word) {
    *word = 0;
    if (!text || !*text) return kMotifEmpty;
    std::string t(text);
    for (char &ch : t) {
        if (ch >= 'a' && ch <= 'z') ch = (char)(ch - 'a' + 'A');
        if (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T') return kMotifLetter;
    }
    // the primitive root: the shortest prefix the text is a whole number of copies of
    size_t k = 1;
    for (; k < t.size(); ++k)
        if (t.size() % k == 0 && t.compare(k, t.size() - k, t, 0, t.size() - k) == 0) break;
    if (k > 15) return kMotifLong;
    uint64_t w = (uint64_t)k << 60;
    for (size_t i = 0; i < k; ++i) w |= (uint64_t)(t[i] == 'A' ? 1 : t[i] == 'C' ? 2 : t[i] == 'G' ? 4 : 8) << (4 * i);
    *word = w;
    return kMotifOk;
}

std::string motif_text(uint64_t word) {
    uint8_t m[15];
    const uint32_t k = motif_codes(word, m);
    if (!k) return ".";
    std::string t;
    for (uint32_t i = 0; i < k; ++i) t += m[i] == 1 ? 'A' : m[i] == 2 ? 'C' : m[i] == 4 ? 'G' : 'T';
    return t;
}

void motif_runs(const uint8_t *packed, uint32_t n_bases, uint64_t word, inq_read_motif_t *out) {
    *out = inq_read_motif_t{0, 0, 0, 0};
    uint8_t m[15];
    const uint32_t k = motif_codes(word, m), n = n_bases;
    if (!k || !n) return;
    auto base = [&](uint32_t i) -> uint8_t { return (packed[i >> 1] >> ((~i & 1u) * 4u)) & 15u; };
    std::vector<uint8_t> in_run(n, 0);  // position i lies in a run of >= k
    for (uint32_t r = 0; r < k; ++r) {
        uint32_t a = 0;  // where the open run began
        for (uint32_t i = 0; i <= n; ++i) {
            if (i < n && base(i) == m[((uint64_t)i + r) % k]) continue;
            // [a, i) is a run (empty where the base before missed too)
            const uint32_t len = i - a;
            if (len > out->run_len || (len == out->run_len && len && a < out->run_beg)) out->run_len = len, out->run_beg = a;
            if (len >= k) {
                ++out->n_runs;
                for (uint32_t j = a; j < i; ++j) in_run[j] = 1;
            }
            a = i + 1;
        }
    }
    for (uint32_t i = 0; i < n; ++i) out->motif_bases += in_run[i];
}

const char *const kReadMotifsHeader =
    "chrom\tbegin\tend\tgroup\tcall\tkind\tread\tqbeg\tlen\tmotif\trun_beg\trun_len\tunits\tmotif_bases\truns";

void append_read_motif_rows(std::string &out, const std::string &chrom, uint32_t start, uint32_t end, const inq_read_call_t *calls,
                            const inq_read_origin_t *origins, const uint8_t *names, const inq_read_seq_t *seqs, const inq_read_motif_t *motifs,
                            uint64_t word, size_t n, bool unphased) {
    const std::string motif = motif_text(word);
    const uint32_t k = motif == "." ? 0u : (uint32_t)motif.size();
    append_read_lines(out, chrom, start, end, calls, origins, names, n, unphased, [&](std::string &o_, size_t i) {
        o_ += '\t', o_ += std::to_string(seqs[i].q_beg), o_ += '\t', o_ += std::to_string(seqs[i].n_bases), o_ += '\t', o_ += motif;
        if (!k) {
            o_ += "\t.\t.\t.\t.\t.";
            return;
        }
        const inq_read_motif_t &t = motifs[i];
        for (const uint32_t v : {t.run_beg, t.run_len, t.run_len / k, t.motif_bases, t.n_runs}) o_ += '\t', o_ += std::to_string(v);
    });
}

void locus_motif_find(const uint8_t *packed, const uint32_t *n_bases, size_t n_records, inq_locus_motif_t *out) {
    *out = inq_locus_motif_t{0, 0, 0, 0, 0};
    constexpr uint32_t kMaxPeriod = 6;
    auto code_of = [](uint8_t c) -> int { return c == 1 ? 0 : c == 2 ? 1 : c == 4 ? 2 : c == 8 ? 3 : -1; };  // A C G T, -1: no base
    // every record's bases in turn: each(n, base) with base(i) the slice's i-th code
    auto each_record = [&](auto &&each) {
        const uint8_t *at = packed;
        for (size_t r = 0; r < n_records; ++r) {
            const uint32_t n = n_bases[r];
            each(n, [at](uint32_t i) -> uint8_t { return (at[i >> 1] >> ((~i & 1u) * 4u)) & 15u; });
            at += ((size_t)n + 1) / 2;
        }
    };
    uint64_t lag[kMaxPeriod + 1] = {0};
    each_record([&](uint32_t n, auto base) {
        out->bases += n;
        for (uint32_t i = 0; i < n; ++i) {
            const uint8_t c = base(i);
            if (code_of(c) < 0) continue;
            for (uint32_t k = 1; k <= kMaxPeriod && k <= i; ++k) lag[k] += base(i - k) == c;
        }
    });
    uint32_t p = 0;
    for (uint32_t k = 1; k <= kMaxPeriod; ++k)
        if (lag[k] > lag[p]) p = k;  // (lag[0] is 0: the smallest k with the largest count, none when all are 0)
    if (!p) return;
    out->period = p, out->tandem = lag[p];
    // the tandem copies by the smallest rotation of their p-mer, two bits a base with the first base on top: numeric order is A < C < G < T
    const uint32_t mask = (1u << (2 * p)) - 1;
    auto turn = [&](uint32_t v) { return ((v << 2) | v >> (2 * (p - 1))) & mask; };
    std::vector<uint64_t> count((size_t)mask + 1, 0);
    each_record([&](uint32_t n, auto base) {
        for (uint32_t i = 0; (uint64_t)i + 2 * p <= n; ++i) {
            uint32_t v = 0;
            bool copy = true;
            for (uint32_t t = 0; t < p && copy; ++t) {
                const int c = code_of(base(i + t));
                copy = c >= 0 && base(i + t) == base(i + p + t);
                v = v << 2 | (uint32_t)(c & 3);
            }
            if (!copy) continue;
            uint32_t least = v;
            for (uint32_t t = 1; t < p; ++t) v = turn(v), least = std::min(least, v);
            ++count[least];
        }
    });
    uint32_t win = 0;
    for (uint32_t v = 1; v <= mask; ++v)
        if (count[v] > count[win]) win = v;  // (ascending: among equal counts the smallest class)
    if (!count[win]) return;
    out->copies = count[win];
    uint32_t d = 1, turned = turn(win);  // the primitive root: the shortest d dividing p that turns the winner into itself
    for (; d < p; ++d, turned = turn(turned))
        if (p % d == 0 && turned == win) break;
    out->word = (uint64_t)d << 60;
    for (uint32_t t = 0; t < d; ++t) out->word |= (uint64_t)(1u << (win >> (2 * (p - 1 - t)) & 3u)) << (4 * t);
}

uint64_t motif_word_in_use(uint64_t given, uint64_t found) {
    uint8_t m[15];
    return motif_codes(given, m) ? given : found;
}

const char *const kLocusMotifsHeader = "chrom\tbegin\tend\treads\tbases\tmotif\tperiod\ttandem\tcopies\tcatalogue\tagrees";

int append_locus_motif_row(std::string &out, const std::string &chrom, uint32_t start, uint32_t end, uint64_t reads, const inq_locus_motif_t &found,
                           uint64_t catalogue_word) {
    const std::string motif = motif_text(found.word), catalogue = motif_text(catalogue_word);
    int agrees = -1;
    if (catalogue != ".") {  // a rotation of the found motif: the same length, and found somewhere in the found motif written twice
        agrees = motif != "." && motif.size() == catalogue.size() && (motif + motif).find(catalogue) != std::string::npos;
    }
    out += chrom;
    for (const uint64_t v : {(uint64_t)start, (uint64_t)end, reads, found.bases}) out += '\t', out += std::to_string(v);
    out += '\t', out += motif;
    for (const uint64_t v : {found.period, found.tandem, found.copies}) out += '\t', out += std::to_string(v);
    out += '\t', out += catalogue, out += '\t', out += agrees < 0 ? "." : agrees ? "1" : "0", out += '\n';
    return agrees;
}

static void erase_all(std::string &s, const std::string &pat) {
    size_t p = 0;
    while ((p = s.find(pat, p)) != std::string::npos) s.erase(p, pat.size());
}

std::string sample_name_from_path(const std::string &bam_path) {
    std::string p = bam_path;
    while (p.size() > 1 && p.back() == '/') p.pop_back();
    size_t slash = p.rfind('/');
    std::string name = slash == std::string::npos ? p : p.substr(slash + 1);
    if (name != "..") {
        size_t dot = name.rfind('.');
        if (dot != std::string::npos && dot != 0) name = name.substr(0, dot);
    }
    erase_all(name, ".bam");
    erase_all(name, ".cram");
    return name;
}

int human_compare(const std::string &a, const std::string &b) {
    size_t i = 0, j = 0;
    auto digit = [](char c) { return c >= '0' && c <= '9'; };
    while (i < a.size() && j < b.size()) {
        if (digit(a[i]) && digit(b[j])) {
            unsigned __int128 x = 0, y = 0;
            while (i < a.size() && digit(a[i])) x = x * 10 + (unsigned)(a[i++] - '0');
            while (j < b.size() && digit(b[j])) y = y * 10 + (unsigned)(b[j++] - '0');
            if (x != y) return x < y ? -1 : 1;
        } else {
            unsigned char ca = (unsigned char)a[i], cb = (unsigned char)b[j];
            if (ca != cb) return ca < cb ? -1 : 1;
            ++i;
            ++j;
        }
    }
    if (i < a.size()) return 1;
    if (j < b.size()) return -1;
    return 0;
}

}  // namespace inqhost
