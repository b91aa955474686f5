// host_common.h - what every piece of the host library shares, the BAM driver (driver_internal.h) and the text commands (text_input.h)
// alike: the two environment switches, the clock, the error buffer, write(2) until done, a failure with its exit status and the guard
// of the C entries.  Header only; it includes nothing of the project but the public header.
#pragma once
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <string>

#include "../../include/inquistr_host.h"

namespace inqhost {

// The two switches every piece of the host library asks about, each read from the environment here and nowhere else in the library.
// INQ_FAST_EXIT=1 (the CLI sets it): the process is about to end, what it holds may be left to the operating system.
inline bool fast_exit() {
    const char *e = std::getenv("INQ_FAST_EXIT");
    return e && e[0] == '1';
}
// INQ_TIMING: 0 = silent (not set), 1 = the [inq timing] lines of a call and the laps of a text command (any value, "0" too),
// 2 = every stage as well
inline int timing_level() {
    const char *e = std::getenv("INQ_TIMING");
    return !e ? 0 : e[0] == '2' ? 2 : 1;
}
using Clock = std::chrono::steady_clock;
inline double secs(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double>(b - a).count(); }
inline double ms(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

inline void set_err(char *buf, size_t cap, const std::string &m) {
    if (buf && cap) std::snprintf(buf, cap, "%s", m.c_str());
}
inline bool write_all(int fd, const char *data, size_t len) {
    size_t off = 0;
    while (off < len) {
        ssize_t w = ::write(fd, data + off, len - off);
        if (w <= 0) return false;
        off += (size_t)w;
    }
    return true;
}
inline bool write_all(int fd, const std::string &s) { return write_all(fd, s.data(), s.size()); }

// what a command throws to end with an exit status and a message (INQ_EXIT_PANIC: one of the reference's panics)
struct Failure {
    int status;
    std::string message;
};

}  // namespace inqhost

// public entries: no C++ exception may unwind across the C ABI.  A Failure is the entry's own status and message; `fail` is what the
// entry returns for anything else
#define INQ_GUARD_AS(fail, expr, errbuf, errcap)                                      \
    try {                                                                             \
        return expr;                                                                  \
    } catch (const inqhost::Failure &f) {                                             \
        inqhost::set_err(errbuf, errcap, f.message);                                  \
        return f.status;                                                              \
    } catch (const std::exception &e) {                                               \
        inqhost::set_err(errbuf, errcap, std::string("internal error: ") + e.what()); \
        return fail;                                                                  \
    } catch (...) {                                                                   \
        inqhost::set_err(errbuf, errcap, "internal error");                           \
        return fail;                                                                  \
    }
#define INQ_GUARD(expr, errbuf, errcap) INQ_GUARD_AS(INQ_EXIT_ERROR, expr, errbuf, errcap)
