// text_input.h — what the two commands over a combined .inq, `outlier` and `assoc`, share.  Reading: the line reader, the field splitter,
// Rust's f32 parser, the first three fields of a line, the walk over its value fields, the whole text in memory with its lines
// (CombinedText).  Running: the thread rule and the runner of the parse, the device context created in the background (BackgroundCtx),
// the lap timer (Laps), the failed device call, the buffered writer of the result (OutBuffer).  A step that fails throws an
// inqhost::Failure; INQ_GUARD at the C entry turns it into the message and the exit status.  Header only; each command includes it.
#pragma once
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/inquistr_host.h"
#include "host_common.h"

namespace inq {
namespace textin {

using inqhost::Failure;
using inqhost::set_err;
using inqhost::write_all;

// utils::reader (src/utils.rs:7-13): niffler sniffs the compression from the first bytes; zlib's gz layer does
// the same for gzip / plain text (bzip2, xz and zstd inputs are not supported here)
struct Lines {
    gzFile gz = nullptr;
    bool open(const char *path) {
        gz = gzopen(path, "rb");
        if (gz) gzbuffer(gz, 1 << 20);
        return gz != nullptr;
    }
    bool next(std::string &line) {  // BufRead::lines(): split on '\n', a trailing '\r' goes too
        line.clear();
        char buf[1 << 16];
        bool got = false;
        for (;;) {
            if (!gzgets(gz, buf, sizeof buf)) break;
            got = true;
            const size_t n = std::strlen(buf);
            line.append(buf, n);
            if (n && buf[n - 1] == '\n') break;
        }
        if (!got) return false;
        if (!line.empty() && line.back() == '\n') line.pop_back();
        if (!line.empty() && line.back() == '\r') line.pop_back();
        return true;
    }
    ~Lines() {
        if (gz) gzclose(gz);
    }
};

inline void split_tabs(const std::string &s, std::vector<std::pair<size_t, size_t>> &out) {
    out.clear();
    size_t p = 0;
    for (;;) {
        const size_t t = s.find('\t', p);
        if (t == std::string::npos) {
            out.emplace_back(p, s.size() - p);
            return;
        }
        out.emplace_back(p, t - p);
        p = t + 1;
    }
}

// Rust's `str::parse::<f32>`: [+-]? ( inf | infinity | nan | digits [. digits] [e [+-] digits] ), nothing around it
inline bool parse_f32(const char *s, size_t n, float *out) {
    // What a combined .inq holds - integers, halves, NaN (src/call.rs:57-65, 518-520) - without strtof: up to six digits with
    // nothing, ".0" or ".5" behind them are exact in f32 (< 2^23), so any correctly rounding parser returns this value.
    {
        size_t k = 0;
        const bool neg = n && s[0] == '-';
        if (neg) k = 1;
        if (n - k == 3 && s[k] == 'N' && s[k + 1] == 'a' && s[k + 2] == 'N' && !neg) {
            *out = std::numeric_limits<float>::quiet_NaN();
            return true;
        }
        uint32_t v = 0;
        size_t d = 0;
        while (k < n && d < 7 && (unsigned)(s[k] - '0') < 10u) v = v * 10u + (uint32_t)(s[k] - '0'), ++k, ++d;
        if (d >= 1 && d <= 6) {
            float f = (float)v;
            bool ok = k == n;
            if (!ok && n - k == 2 && s[k] == '.' && (s[k + 1] == '0' || s[k + 1] == '5')) {
                if (s[k + 1] == '5') f += 0.5f;
                ok = true;
            }
            if (ok) {
                *out = neg ? -f : f;
                return true;
            }
        }
    }
    size_t i = 0;
    if (i < n && (s[i] == '+' || s[i] == '-')) ++i;
    auto word = [&](const char *w) {
        const size_t m = std::strlen(w);
        if (n - i != m) return false;
        for (size_t k = 0; k < m; ++k)
            if ((s[i + k] | 0x20) != w[k]) return false;
        return true;
    };
    bool ok = word("inf") || word("infinity") || word("nan");
    if (!ok) {
        size_t j = i, digits = 0;
        while (j < n && s[j] >= '0' && s[j] <= '9') ++j, ++digits;
        if (j < n && s[j] == '.') {
            ++j;
            while (j < n && s[j] >= '0' && s[j] <= '9') ++j, ++digits;
        }
        if (!digits) return false;
        if (j < n && (s[j] == 'e' || s[j] == 'E')) {
            ++j;
            if (j < n && (s[j] == '+' || s[j] == '-')) ++j;
            size_t ed = 0;
            while (j < n && s[j] >= '0' && s[j] <= '9') ++j, ++ed;
            if (!ed) return false;
        }
        if (j != n) return false;
    }
    char tmp[128];
    if (n >= sizeof tmp) {  // absurdly long literal: strtof on a heap copy
        std::string t(s, n);
        *out = std::strtof(t.c_str(), nullptr);
        return true;
    }
    std::memcpy(tmp, s, n);
    tmp[n] = 0;
    *out = std::strtof(tmp, nullptr);  // correctly rounded, like Rust
    return true;
}

inline std::string strip_hap(std::string s) {  // .replace("_H1", "").replace("_H2", ""), src/outlier.rs:108,128
    for (const char *pat : {"_H1", "_H2"}) {
        size_t p = 0;
        while ((p = s.find(pat, p)) != std::string::npos) s.erase(p, 3);
    }
    return s;
}

// chrom, begin, end of a line as they stand in the file; false: the line has fewer than three fields
struct Span {
    const char *p;
    size_t n;
};
inline bool first_three(const char *p, const char *end, Span out[3]) {
    const char *t1 = (const char *)std::memchr(p, '\t', (size_t)(end - p));
    const char *t2 = t1 ? (const char *)std::memchr(t1 + 1, '\t', (size_t)(end - t1 - 1)) : nullptr;
    if (!t2) return false;
    const char *t3 = (const char *)std::memchr(t2 + 1, '\t', (size_t)(end - t2 - 1));
    out[0] = Span{p, (size_t)(t1 - p)}, out[1] = Span{t1 + 1, (size_t)(t2 - t1 - 1)}, out[2] = Span{t2 + 1, (size_t)((t3 ? t3 : end) - t2 - 1)};
    return true;
}

// The value fields of a line (column 3 on): f(k, begin, length) for value k = 0, 1, ...; f returns false to stop the walk.  Returns the
// number of fields of the whole line, the first three included, or kWalkStopped.  A template, so that f inlines: this is the parse loop.
constexpr size_t kWalkStopped = (size_t)-1;
template <class F> inline size_t walk_values(const char *p, const char *end, F &&f) {
    size_t field = 0;
    const char *f0 = p;
    for (const char *q = p;; ++q) {
        if (q == end || *q == '\t') {
            if (field >= 3 && !f(field - 3, f0, (size_t)(q - f0))) return kWalkStopped;
            ++field;
            f0 = q + 1;
            if (q == end) break;
        }
    }
    return field;
}

// How many threads work on `items` things when one thread is worth starting per `per_thread` of them (16 at the most), and the
// runner: fn(t) for t = 0 .. n_thr - 1, t = 0 on the calling thread
inline size_t thread_count(size_t items, size_t per_thread) {
    const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    return std::max<size_t>(1, std::min<size_t>(hw, items / per_thread + 1));
}
template <class F> inline void on_threads(size_t n_thr, F &&fn) {
    std::vector<std::thread> th;
    for (size_t t = 1; t < n_thr; ++t) th.emplace_back([&fn, t] { fn(t); });
    fn(0);
    for (auto &x : th) x.join();
}
constexpr size_t kLinesPerThread = 2048;  // of the parse of both commands

// A whole file in memory: a plain file is mapped (no copy: the page cache is the buffer; round 2 pulled 139 MB through gzread, 0.1 s
// on one thread), a gzip file inflated.
struct TextFile {
    std::string text;
    const char *data = nullptr;
    size_t size = 0;
    struct Mapping {
        void *p = MAP_FAILED;
        size_t len = 0;
        ~Mapping() {
            if (p != MAP_FAILED) ::munmap(p, len);
        }
    } mapping;
    bool load(const char *path, std::string &err) {
        {
            int fd = ::open(path, O_RDONLY);
            unsigned char magic[2] = {0, 0};
            struct stat st;
            const bool plain = fd >= 0 && ::fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0 && ::pread(fd, magic, 2, 0) == 2 &&
                               !(magic[0] == 0x1f && magic[1] == 0x8b);
            if (plain) {
                mapping.len = (size_t)st.st_size;
                mapping.p = ::mmap(nullptr, mapping.len, PROT_READ, MAP_PRIVATE, fd, 0);
                if (mapping.p != MAP_FAILED) {
                    (void)::madvise(mapping.p, mapping.len, MADV_WILLNEED);
                    data = (const char *)mapping.p;
                    size = mapping.len;
                }
            }
            if (fd >= 0) ::close(fd);
        }
        if (!data) {
            Lines in;
            if (!in.open(path)) {
                err = "Problem opening file";
                return false;
            }
            char buf[1 << 16];
            int got;
            while ((got = gzread(in.gz, buf, sizeof buf)) > 0) text.append(buf, (size_t)got);
            if (got < 0) {
                err = "Problem reading file";
                return false;
            }
            data = text.data();
            size = text.size();
        }
        return true;
    }
};

// BufRead::lines(): split on '\n' (a trailing '\r' goes too); no line after a final newline.  The newlines are found by
// several threads, each over its own stretch of the text (4 MiB is worth a thread).  lines: (offset, length)
inline void find_lines(const char *tdata, size_t tsize, std::vector<std::pair<size_t, size_t>> &lines) {
    const size_t parts = thread_count(tsize, 4u << 20);
    std::vector<std::vector<size_t>> nl(parts);  // positions of '\n' per stretch
    on_threads(parts, [&](size_t t) {
        const size_t lo = tsize * t / parts, hi = tsize * (t + 1) / parts;
        nl[t].reserve((hi - lo) / 256 + 16);
        for (size_t p = lo; p < hi;) {
            const char *q = (const char *)std::memchr(tdata + p, '\n', hi - p);
            if (!q) break;
            nl[t].push_back((size_t)(q - tdata));
            p = (size_t)(q - tdata) + 1;
        }
    });
    size_t total = 1;
    for (auto &v : nl) total += v.size();
    lines.reserve(total);
    size_t p = 0;
    auto push = [&](size_t e) {
        size_t len = e - p;
        if (len && tdata[p + len - 1] == '\r') --len;
        lines.emplace_back(p, len);
        p = e + 1;
    };
    for (auto &v : nl)
        for (size_t e : v) push(e);
    if (p < tsize) push(tsize);
}

// The combined file and its lines: read(), split(), then header() and the loci 0 .. loci() - 1 behind it.  The three are apart
// because the commands print a lap between them.
struct CombinedText {
    TextFile file;
    std::vector<std::pair<size_t, size_t>> lines;
    void read(const char *path) {
        std::string err;
        if (!file.load(path, err)) throw Failure{INQ_EXIT_PANIC, err};
    }
    void split() { find_lines(file.data, file.size, lines); }
    std::string header() const {  // lines.next().unwrap(), src/outlier.rs:36
        if (lines.empty()) throw Failure{INQ_EXIT_PANIC, "called `Option::unwrap()` on a `None` value (empty combined file)"};
        return std::string(file.data + lines[0].first, lines[0].second);
    }
    size_t loci() const { return lines.size() - 1; }
    const char *begin(size_t locus) const { return file.data + lines[locus + 1].first; }
    const char *end(size_t locus) const { return begin(locus) + lines[locus + 1].second; }
};

// "[inq <tag>] <what> at <ms>" on stderr since the timer was made, with INQ_TIMING set (to anything)
struct Laps {
    const char *tag;
    bool on = inqhost::timing_level() != 0;
    inqhost::Clock::time_point t0 = inqhost::Clock::now();
    void operator()(const char *what) const {
        if (on) std::fprintf(stderr, "[inq %s] %-22s at %7.1f ms\n", tag, what, inqhost::ms(t0, inqhost::Clock::now()));
    }
};

// The device context, created on a thread of its own while the text is read and parsed: the HIP runtime takes 0.1 - 0.3 s to start.
// Whoever leaves the command, by return or by Failure, joins the thread; the context is destroyed unless the process is about to end.
struct BackgroundCtx {
    inq_ctx_t *ctx = nullptr;
    int rc = INQ_OK;
    std::thread thread;
    explicit BackgroundCtx(int device) : thread([this, device] { rc = inq_ctx_create(device, &ctx); }) {}
    inq_ctx_t *wait(const Laps &lap) {
        thread.join();
        lap("device context there");
        if (rc != INQ_OK) throw Failure{INQ_EXIT_ERROR, std::string("cannot open HIP device: ") + inq_strerror(rc)};
        return ctx;
    }
    ~BackgroundCtx() {
        if (thread.joinable()) thread.join();
        if (!inqhost::fast_exit()) inq_ctx_destroy(ctx);
    }
};

// A device call of these commands that returned rc != INQ_OK: always INQ_EXIT_ERROR (inqhost::device_call_failed is `call`'s: there a
// domain error is one of the reference's panics)
[[noreturn]] inline void device_call_failed(int rc, inq_ctx_t *ctx) {
    const std::string detail = rc == INQ_ERR_HIP ? inq_last_error(ctx) : "";
    throw Failure{INQ_EXIT_ERROR, std::string("device call failed: ") + inq_strerror(rc) + (detail.empty() ? "" : " [" + detail + "]")};
}

// The result on its way to out_fd: appended to `text`, written at 1 MiB and at the end; a write that fails is INQ_EXIT_PANIC
struct OutBuffer {
    int fd;
    std::string text;
    void flush() {
        if (!write_all(fd, text)) throw Failure{INQ_EXIT_PANIC, ""};
        text.clear();
    }
    void line_done() {
        if (text.size() > (1u << 20)) flush();
    }
};

}  // namespace textin
}  // namespace inq
