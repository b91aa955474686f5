// text_input.h — reading a combined .inq (and the small tab-separated files beside it) as `outlier` and `assoc` both do: the line
// reader, the field splitter, Rust's f32 parser, the whole text in memory and its lines.  Header only; each command includes it.
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

namespace inq {
namespace textin {

inline void set_err(char *buf, size_t cap, const std::string &m) {
    if (buf && cap) std::snprintf(buf, cap, "%s", m.c_str());
}

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

inline bool write_all(int fd, const std::string &s) {
    size_t off = 0;
    while (off < s.size()) {
        ssize_t w = ::write(fd, s.data() + off, s.size() - off);
        if (w <= 0) return false;
        off += (size_t)w;
    }
    return true;
}

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
// several threads, each over its own stretch of the text.  lines: (offset, length)
inline void find_lines(const char *tdata, size_t tsize, std::vector<std::pair<size_t, size_t>> &lines) {
    {
        const unsigned hw0 = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
        const size_t parts = std::max<size_t>(1, std::min<size_t>(hw0, tsize / (4u << 20) + 1));
        std::vector<std::vector<size_t>> nl(parts);  // positions of '\n' per stretch
        std::vector<std::thread> th;
        auto scan = [&](size_t t) {
            const size_t lo = tsize * t / parts, hi = tsize * (t + 1) / parts;
            nl[t].reserve((hi - lo) / 256 + 16);
            for (size_t p = lo; p < hi;) {
                const char *q = (const char *)std::memchr(tdata + p, '\n', hi - p);
                if (!q) break;
                nl[t].push_back((size_t)(q - tdata));
                p = (size_t)(q - tdata) + 1;
            }
        };
        for (size_t t = 1; t < parts; ++t) th.emplace_back(scan, t);
        scan(0);
        for (auto &x : th) x.join();
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
}

}  // namespace textin
}  // namespace inq
