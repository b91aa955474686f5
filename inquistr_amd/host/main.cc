// main.cc — `inquistr call`: the CLI surface of the reference's `call` subcommand (src/main.rs:27-64),
// same flags and defaults.  Other subcommands of the reference are out of scope.
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/inquistr_host.h"
#include "host_common.h"
#include "hostapi.h"
#include "serve.h"

static void usage(FILE *f) {
    std::fputs(
        "Call lengths\n\nUsage: inquistr call [OPTIONS] <BAM>\n\nArguments:\n  <BAM>  bam file to call STRs in\n\nOptions:\n"
        "  -r, --region <REGION>            region string to genotype expansion in\n"
        "  -R, --region-file <REGION_FILE>  Bed file with region(s) to genotype expansion(s) in\n"
        "  -m, --minlen <MINLEN>            minimal length of insertion/deletion operation [default: 5]\n"
        "  -s, --support <SUPPORT>          minimal number of supporting reads [default: 3]\n"
        "  -t, --threads <THREADS>          Number of parallel threads to use [default: 1]\n"
        "  -u, --unphased                   If reads have to be considered unphased\n"
        "      --sample-name <SAMPLE_NAME>  sample name to use in output\n"
        "      --reference <REFERENCE>      reference fasta for cram decoding\n"
        "      --device <N>                 HIP device ordinal [default: 0]\n"
        "      --devices <N,N,...>          several HIP devices: the loci are split among them by BAM bytes, same output\n"
        "      --ctx-option <KEY=VALUE>     a device-context option (include/inquistr_hip.h, inq_ctx_set_option), repeatable\n"
        "      --ties <FILE>                write the loci whose unphased split is tie-ambiguous there, as BED (empty when phased)\n"
        "      --evidence <FILE>            write the read evidence behind every row there: fetched, kept, h1, h2, clipped, min, max\n"
        "      --read-calls <FILE>          write the per-read Calls behind every row's two medians there: h1, h2, other\n"
        "      --read-table <FILE>          write one line per kept read there: group, call, kind, read name, pos, strand, mapq\n"
        "      --read-seqs <FILE>           write one line per kept read there: group, call, kind, read name, and the read's bases over the locus\n"
        "      --read-motifs <FILE>         write one line per kept read there: group, call, kind, read name, and the pure runs of the locus's motif\n"
        "                                   in the read's bases over the locus (longest run, motif units, bases in runs, number of runs)\n"
        "      --motif <STR>                the motif of every target for --read-motifs (default: column 4 of the BED; needed with -r);\n"
        "                                   `auto`: the motif found in each target's own kept reads (works with -r and three-column BEDs)\n"
        "      --locus-motifs <FILE>        write one line per target there: the motif of 1 to 6 bases its kept reads repeat (period, lag\n"
        "                                   count, tandem copies), the catalogue's motif (--motif, else column 4) and whether they agree\n"
        "  -h, --help                       Print help\n",
        f);
}

// The arguments behind the subcommand, one at a time: `arg` as it stands, and for `--key=value` the two halves (`key`, `inl`); any
// other argument is its own key.  A command that takes `--key=value` matches on `key`, one that does not (cohort, serve) on `arg`.
struct Options {
    int argc;
    char **argv;
    int i = 1;  // argv[1] is the subcommand
    Options(int argc_, char **argv_) : argc(argc_), argv(argv_) {}
    std::string arg, key;
    const char *inl = nullptr;
    bool next() {
        if (++i >= argc) return false;
        arg = key = argv[i];
        inl = nullptr;
        const size_t eq = arg.find('=');
        if (arg.size() > 2 && arg[0] == '-' && arg[1] == '-' && eq != std::string::npos) key = arg.substr(0, eq), inl = argv[i] + eq + 1;
        return true;
    }
    // the value of the option at hand: the part behind `=` when it carried one, else the next argument (the cursor moves on to it)
    const char *need() {
        if (inl) return inl;
        if (i + 1 >= argc) {
            std::fprintf(stderr, "error: a value is required for '%s' but none was supplied\n", argv[i]);
            std::exit(2);
        }
        return argv[++i];
    }
    bool dashed() const { return arg.size() > 1 && arg[0] == '-'; }
};

static int unexpected(const std::string &s) {
    std::fprintf(stderr, "error: unexpected argument '%s' found\n", s.c_str());
    return 2;
}

// the value of an option that takes one of a few words; any other word ends the process as a usage error
struct Word {
    const char *word;
    int value;
};
static int choice(const char *v, const char *flag, std::initializer_list<Word> words) {
    std::string possible;
    for (const Word &w : words) {
        if (std::strcmp(v, w.word) == 0) return w.value;
        possible += std::string(possible.empty() ? "" : ", ") + w.word;
    }
    std::fprintf(stderr, "error: invalid value '%s' for '%s'\n  [possible values: %s]\n", v, flag, possible.c_str());
    std::exit(2);
}

// a command's message on stderr: the reference's panic form for 101
static void complain(int rc, const char *err) {
    if (rc != 0) std::fprintf(stderr, rc == INQ_EXIT_PANIC ? "thread 'main' panicked:\n%s\n" : "%s\n", err);
}

// How a command that used the device ends: its message, then - the rows went out through write(2), nothing is buffered - past the
// atexit handlers of the HIP runtime (0.15 - 0.2 s of tear-down for a process that is over).  Every such command sets INQ_FAST_EXIT=1
// unless the user set it: INQ_FAST_EXIT=0 leaves normally (profilers write their output at exit).
static int leave(int rc, const char *err) {
    if (err) complain(rc, err);
    std::fflush(nullptr);
    if (inqhost::fast_exit()) std::_Exit(rc);
    return rc;
}

// A command that ends the process with it and uses the device: it sets INQ_FAST_EXIT=1 (unless the user set it) before the host library runs -
// the device context is left to the operating system - and goes out through leave()
template <class F> static int finish(F &&command) {
    char err[1024] = {0};
    ::setenv("INQ_FAST_EXIT", "1", 0);
    return leave(command(err, sizeof err), err);
}

static int cmd_combine(int argc, char **argv) {  // src/main.rs:65-71: one or more .inq files
    if (argc < 3) {
        std::fputs("error: the following required arguments were not provided:\n  <CALLS>...\n\nUsage: inquistr combine <CALLS>...\n", stderr);
        return 2;
    }
    char err[1024] = {0};
    int rc = inq::host_api().combine(argv + 2, (size_t)(argc - 2), 1, err, sizeof err);
    complain(rc, err);
    return rc;
}

static int cmd_outlier(int argc, char **argv) {  // src/main.rs:75-99; numbers go through strtoul / strtof / strtol unchecked, and there is no -h
    inq_outlier_args_t o;
    std::memset(&o, 0, sizeof o);
    o.minsize = 10;
    o.zscore = 3.0f;
    o.method = INQ_OUTLIER_ZSCORE;
    for (Options p(argc, argv); p.next();) {
        const std::string &key = p.key;
        if (key == "--minsize") o.minsize = (uint32_t)std::strtoul(p.need(), nullptr, 10);
        else if (key == "-z" || key == "--zscore") o.zscore = std::strtof(p.need(), nullptr);
        else if (key == "--method") o.method = choice(p.need(), "--method <METHOD>", {{"zscore", INQ_OUTLIER_ZSCORE}, {"dbscan", INQ_OUTLIER_DBSCAN}});
        else if (key == "-s" || key == "--sample") o.sample = p.need();
        else if (key == "-S" || key == "--subset") o.subset_file = p.need();
        else if (key == "--device") o.device = (int32_t)std::strtol(p.need(), nullptr, 10);
        else if (p.dashed() || o.combined) return unexpected(p.arg);
        else o.combined = argv[p.i];
    }
    if (!o.combined) {
        std::fputs("error: the following required arguments were not provided:\n  <COMBINED>\n\nUsage: inquistr outlier [OPTIONS] <COMBINED>\n", stderr);
        return 2;
    }
    return finish([&](char *err, size_t cap) { return inq::host_api().outlier(&o, 1, err, cap); });
}

// Not a subcommand of the reference's binary: its scripts/STR_regression.R (one glm() per locus), the regressions on the device
static int cmd_assoc(int argc, char **argv) {
    static const char *const kUsage =
        "Usage: inquistr assoc <COMBINED> --phenocovar <FILE> --phenotype <COL> --outcome <binary|continuous>\n"
        "                      [--binary-order <A,B>] [--covariates <c1,c2,...>] [--str-mode <max|min|mean>]\n"
        "                      [--missing-cutoff <0.8>] [--chr <CHR> [--chr-begin <N> --chr-end <N>]] [--all-rows] [--device <N>]\n"
        "                      [--firth <no|fallback|always>]\n";
    inq_assoc_args_t o;
    std::memset(&o, 0, sizeof o);
    o.missing_cutoff = 0.8;
    o.outcome = -1;
    o.str_mode = INQ_ASSOC_MAX;
    o.chr_begin = o.chr_end = -1;
    auto number = [&](const char *s, const char *flag) {  // a number with nothing behind it
        char *e = nullptr;
        const double v = std::strtod(s, &e);
        if (!*s || *e) {
            std::fprintf(stderr, "error: invalid value '%s' for '%s'\n", s, flag);
            std::exit(2);
        }
        return v;
    };
    for (Options p(argc, argv); p.next();) {
        const std::string &key = p.key;
        if (key == "--phenocovar") o.phenocovar = p.need();
        else if (key == "--phenotype") o.phenotype = p.need();
        else if (key == "--binary-order") o.binary_order = p.need();
        else if (key == "--covariates") o.covariates = p.need();
        else if (key == "--chr") o.chr = p.need();
        else if (key == "--chr-begin") o.chr_begin = (int64_t)number(p.need(), "--chr-begin <N>");
        else if (key == "--chr-end") o.chr_end = (int64_t)number(p.need(), "--chr-end <N>");
        else if (key == "--missing-cutoff") o.missing_cutoff = number(p.need(), "--missing-cutoff <CUTOFF>");
        else if (key == "--all-rows") o.all_rows = 1;
        else if (key == "--firth") {
            // a value that is none of the three goes on as it is: the host entry refuses it (101), as it does --firth with continuous
            const std::string m = p.need();
            o.firth = m == "no" ? INQ_HOST_FIRTH_NO : m == "fallback" ? INQ_HOST_FIRTH_FALLBACK : m == "always" ? INQ_HOST_FIRTH_ALWAYS : -1;
        }
        else if (key == "--device") o.device = (int32_t)number(p.need(), "--device <N>");
        else if (key == "--outcome") o.outcome = choice(p.need(), "--outcome <OUTCOME>", {{"binary", INQ_ASSOC_BINARY}, {"continuous", INQ_ASSOC_CONTINUOUS}});
        else if (key == "--str-mode") o.str_mode = choice(p.need(), "--str-mode <MODE>", {{"max", INQ_ASSOC_MAX}, {"min", INQ_ASSOC_MIN}, {"mean", INQ_ASSOC_MEAN}});
        else if (key == "-h" || key == "--help") {
            std::fputs(kUsage, stdout);
            return 0;
        }
        else if (p.dashed() || o.combined) return unexpected(p.arg);
        else o.combined = argv[p.i];
    }
    if (!o.combined || !o.phenocovar || !o.phenotype || o.outcome < 0) {
        std::fputs("error: the following required arguments were not provided:\n  <COMBINED> --phenocovar <FILE> --phenotype <COL> --outcome <OUTCOME>\n\n", stderr);
        std::fputs(kUsage, stderr);
        return 2;
    }
    return finish([&](char *err, size_t cap) { return inq::host_api().assoc(&o, 1, err, cap); });
}

// Not a subcommand of the reference: the loop a user writes around `inquiSTR call` for a cohort (one call per BAM with the
// same targets, then `combine`), run in ONE process so that the HIP runtime starts once.  Every <out-dir>/<sample>.inq is
// byte for byte what `inquistr call <BAM> ...` prints.  (`--key=value` is not split here: the whole argument is matched.)
static int cmd_cohort(int argc, char **argv) {
    inq_call_args_t base;
    std::memset(&base, 0, sizeof base);
    base.minlen = 5, base.support = 3, base.threads = 1;
    std::string out_dir, combined;
    std::vector<std::string> bams;
    bool ties = false;  // --ties: <out-dir>/<sample>.ties.bed next to each .inq
    for (Options p(argc, argv); p.next();) {
        const std::string &k = p.arg;
        if (k == "-r" || k == "--region") base.region = p.need();
        else if (k == "-R" || k == "--region-file" || k == "--region_file") base.region_file = p.need();
        else if (k == "-m" || k == "--minlen") base.minlen = (uint32_t)std::strtoul(p.need(), nullptr, 10);
        else if (k == "-s" || k == "--support") base.support = std::strtoull(p.need(), nullptr, 10);
        else if (k == "-t" || k == "--threads") base.threads = std::strtoull(p.need(), nullptr, 10);
        else if (k == "-u" || k == "--unphased") base.unphased = 1;
        else if (k == "--device") base.device = (int32_t)std::strtol(p.need(), nullptr, 10);
        else if (k == "-o" || k == "--out-dir") out_dir = p.need();
        else if (k == "--combined") combined = p.need();
        else if (k == "--ties") ties = true;
        else if (k == "--read-table") {  // (a cohort's calls run on a session, which writes no read table)
            std::fputs("error: '--read-table <FILE>' cannot be used with cohort: a session does not write the read table\n", stderr);
            return 2;
        }
        else if (k == "--read-seqs") {  // (likewise)
            std::fputs("error: '--read-seqs <FILE>' cannot be used with cohort: a session does not write the read-seqs file\n", stderr);
            return 2;
        }
        else if (p.dashed()) return unexpected(k);
        else bams.push_back(k);
    }
    if (bams.empty() || out_dir.empty()) {
        std::fputs("Usage: inquistr cohort [-r REGION | -R BED] [-m N] [-s N] [-t N] [-u] [--device N] [--ties] --out-dir DIR [--combined FILE] <BAM>...\n", stderr);
        return 2;
    }
    ::setenv("INQ_FAST_EXIT", "1", 0);
    inq_session_t *S = nullptr;
    if (inq::host_api().session_open(base.device, &S) != 0) return 1;
    std::vector<inq_call_args_t> args(bams.size(), base);
    std::vector<std::string> outs(bams.size()), ties_paths(bams.size());
    std::vector<int> fds(bams.size(), -1), st(bams.size(), 0);
    for (size_t k = 0; k < bams.size(); ++k) {
        args[k].bam = bams[k].c_str();
        char name[4096];
        inq::host_api().host_sample_name(bams[k].c_str(), name, sizeof name);
        outs[k] = out_dir + "/" + name + ".inq";
        if (ties) ties_paths[k] = out_dir + "/" + name + ".ties.bed", args[k].ties_path = ties_paths[k].c_str();
        fds[k] = ::open(outs[k].c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (fds[k] < 0) {
            std::fprintf(stderr, "cannot write %s\n", outs[k].c_str());
            return 1;
        }
    }
    char err[2048] = {0};
    int rc = inq::host_api().session_call_many(S, args.data(), args.size(), fds.data(), st.data(), err, sizeof err);
    for (int fd : fds) ::close(fd);
    for (size_t k = 0; k < bams.size(); ++k)
        if (st[k] != 0) std::fprintf(stderr, "%s: exit status %d\n", bams[k].c_str(), st[k]);
    complain(rc, err);
    if (rc == 0 && !combined.empty()) {
        int cfd = ::open(combined.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        std::vector<const char *> files;
        for (auto &o : outs) files.push_back(o.c_str());
        rc = cfd < 0 ? 1 : inq::host_api().combine(files.data(), files.size(), cfd, err, sizeof err);
        if (cfd >= 0) ::close(cfd);
        if (rc != 0) std::fprintf(stderr, "%s\n", err);
    }
    rc = leave(rc, nullptr);  // (what there was to say has been said)
    inq::host_api().session_close(S);
    return rc;
}

// Not a subcommand of the reference: a process that keeps the device context, so that `inquistr call` - one process per
// sample, as workflow managers start it - does not pay the HIP runtime's start-up (0.1 - 0.4 s) per file.  `call` hands
// its arguments and its stdout to the server named by INQ_SERVER=<socket>; without one it runs as always.
// (`--key=value` is not split here either, and every word that is no option of it is unexpected.)
static int cmd_serve(int argc, char **argv) {
    std::string sock;
    int device = 0;
    double idle = 0.0;
    for (Options p(argc, argv); p.next();) {
        const std::string &k = p.arg;
        if (k == "--socket") sock = p.need();
        else if (k == "--device") device = (int)std::strtol(p.need(), nullptr, 10);
        else if (k == "--idle-exit") idle = std::strtod(p.need(), nullptr);
        else if (k == "--quit") {
            if (sock.empty()) sock = std::getenv("INQ_SERVER") ? std::getenv("INQ_SERVER") : "";
            if (sock == "auto") sock = inq::auto_socket_path(device);
            return inq::client_quit(sock.c_str()) ? 0 : 1;
        }
        else return unexpected(k);
    }
    if (sock.empty()) {
        std::fputs("Usage: inquistr serve --socket PATH [--device N] [--idle-exit SECONDS]\n       inquistr serve --socket PATH --quit\n", stderr);
        return 2;
    }
    ::setenv("INQ_FAST_EXIT", "1", 0);
    return inq::serve_main(sock.c_str(), device, idle);
}

// what `call` writes beside the .inq through arguments of inq_genotype_repeats_locus_motifs (they are no fields of inq_call_args_t)
struct CallFiles {
    const char *read_calls = nullptr;    // --read-calls
    const char *read_table = nullptr;    // --read-table
    const char *read_seqs = nullptr;     // --read-seqs
    const char *read_motifs = nullptr;   // --read-motifs
    const char *motif = nullptr;         // --motif: one motif for every target of the read-motifs file
    const char *locus_motifs = nullptr;  // --locus-motifs
};

// the call in this process, on `devices` (none: the one of a.device); st: one entry per device, or null
static int call_here(const inq_call_args_t &a, const CallFiles &f, const std::vector<int32_t> &devices, inq_part_stats_t *st, char *err, size_t cap) {
    return inq::host_api().genotype_repeats_locus_motifs(&a, devices.empty() ? nullptr : devices.data(), devices.size(), 1 /* stdout */, f.read_calls,
                                                         f.read_table, f.read_seqs, f.read_motifs, f.motif, f.locus_motifs, st, err, cap);
}

// INQ_SERVER is set: the call is handed to the server there.  Returns the process's exit status, or -1 when no server is there (the
// call then runs here, as without INQ_SERVER)
static int call_on_server(const char *server_env, const inq_call_args_t &a, const CallFiles &f) {
    // a server's calls run on a session, which writes none of these files: said here, before a server is looked for
    const struct {
        const char *flag, *noun, *path;
    } refused[] = {{"--evidence", "evidence file", a.evidence_path},     {"--read-calls", "read-calls file", f.read_calls},
                   {"--read-table", "read table", f.read_table},         {"--read-seqs", "read-seqs file", f.read_seqs},
                   {"--read-motifs", "read-motifs file", f.read_motifs}, {"--locus-motifs", "locus-motifs file", f.locus_motifs}};
    for (const auto &r : refused)
        if (r.path) {
            std::fprintf(stderr, "error: '%s <FILE>' cannot be used with INQ_SERVER set: a server does not write the %s\n", r.flag, r.noun);
            return 2;
        }
    // INQ_SERVER=auto: this user's server for the device, started (detached; it leaves after INQ_SERVER_IDLE seconds without a
    // call, 120 by default) when none is running - the first call of a batch pays the start-up, the others find the context there
    std::string server_path = server_env;
    if (server_path == "auto") {
        server_path = inq::auto_socket_path(a.device);
        char exe[4096];
        const ssize_t n = ::readlink("/proc/self/exe", exe, sizeof exe - 1);
        const char *idle = std::getenv("INQ_SERVER_IDLE");
        if (n > 0) {
            exe[n] = 0;
            (void)inq::ensure_server(exe, server_path.c_str(), a.device, idle && *idle ? std::strtod(idle, nullptr) : 120.0);
        }
    }
    const char *server = server_path.c_str();
    int st = 0;
    std::string msg;
    const int got = inq::client_call(server, &a, 1 /* stdout */, &st, &msg);
    if (got > 0) {
        complain(st, msg.c_str());
        return st;
    }
    if (got < 0) {
        std::fprintf(stderr, "the server at %s went away during the call\n", server);
        return 1;
    }
    return -1;
}

static int cmd_call(int argc, char **argv) {
    if (argc == 2) {  // arg_required_else_help
        usage(stderr);
        return 2;
    }
    inq_call_args_t a;
    std::memset(&a, 0, sizeof a);
    a.minlen = 5;
    a.support = 3;
    a.threads = 1;
    std::string bam;
    CallFiles f;
    std::vector<int32_t> devices;  // --devices: one part of the targets per entry (an ordinal may repeat: N parts on one GPU)
    std::vector<std::pair<std::string, long long>> ctx_options;  // --ctx-option key=value
    auto num = [&](const char *s, const char *flag) -> unsigned long long {  // digits only: no sign, nothing behind them
        char *e = nullptr;
        const unsigned long long v = std::strtoull(s, &e, 10);
        if (!*s || *s == '-' || *e) {
            std::fprintf(stderr, "error: invalid value '%s' for '%s'\n", s, flag);
            std::exit(2);
        }
        return v;
    };
    for (Options p(argc, argv); p.next();) {
        const std::string &key = p.key;
        if (key == "-r" || key == "--region") a.region = p.need();
        else if (key == "-R" || key == "--region-file" || key == "--region_file") a.region_file = p.need();
        else if (key == "-m" || key == "--minlen") a.minlen = (uint32_t)num(p.need(), "--minlen");
        else if (key == "-s" || key == "--support") a.support = num(p.need(), "--support");
        else if (key == "-t" || key == "--threads") a.threads = num(p.need(), "--threads");
        else if (key == "-u" || key == "--unphased") a.unphased = 1;
        else if (key == "--sample-name" || key == "--sample_name") a.sample_name = p.need();
        else if (key == "--reference") a.reference = p.need();
        else if (key == "--device") a.device = (int32_t)num(p.need(), "--device");
        else if (key == "--ties") a.ties_path = p.need();
        else if (key == "--evidence") a.evidence_path = p.need();
        else if (key == "--read-calls") f.read_calls = p.need();
        else if (key == "--read-table") f.read_table = p.need();
        else if (key == "--read-seqs") f.read_seqs = p.need();
        else if (key == "--read-motifs") f.read_motifs = p.need();
        else if (key == "--motif") f.motif = p.need();
        else if (key == "--locus-motifs") f.locus_motifs = p.need();
        else if (key == "--devices") {
            const std::string list = p.need();
            for (size_t b = 0; b <= list.size();) {
                const size_t e = std::min(list.find(',', b), list.size());
                devices.push_back((int32_t)num(list.substr(b, e - b).c_str(), "--devices"));
                b = e + 1;
            }
        }
        else if (key == "--ctx-option") {  // KEY=VALUE: the value is the whole text behind the flag, its own `=` included
            const std::string kv = p.inl ? p.inl : p.need();
            const size_t e2 = kv.find('=');
            char *endp = nullptr;
            const long long v = e2 == std::string::npos ? 0 : std::strtoll(kv.c_str() + e2 + 1, &endp, 10);
            if (e2 == std::string::npos || e2 == 0 || e2 + 1 == kv.size() || (endp && *endp)) {
                std::fprintf(stderr, "error: invalid value '%s' for '--ctx-option <KEY=VALUE>'\n", kv.c_str());
                return 2;
            }
            ctx_options.emplace_back(kv.substr(0, e2), v);
        }
        else if (key == "-h" || key == "--help") {
            usage(stdout);
            return 0;
        }
        else if (p.dashed() || !bam.empty()) return unexpected(p.arg);
        else bam = p.arg;
    }
    if (bam.empty()) {
        std::fputs("error: the following required arguments were not provided:\n  <BAM>\n", stderr);
        return 2;
    }
    a.bam = bam.c_str();
    for (const auto &kv : ctx_options)  // (a call handed to a server runs on the server's context: its options are the server's)
        if (inq::host_api().ctx_option(kv.first.c_str(), kv.second) != 0) {
            std::fprintf(stderr, "error: invalid value '%s=%lld' for '--ctx-option <KEY=VALUE>': no such option, or value out of range\n", kv.first.c_str(), kv.second);
            return 2;
        }
    if (devices.size() == 1) a.device = devices[0], devices.clear();
    if (!devices.empty()) {
        // one process, one thread + one device context per listed device (host/multi_device.cc); a server holds ONE device.
        // Not through finish(): the [inq part] lines stand between the message and the way out
        char err[1024] = {0};
        ::setenv("INQ_FAST_EXIT", "1", 0);
        std::vector<inq_part_stats_t> st(devices.size());
        int rc = call_here(a, f, devices, st.data(), err, sizeof err);
        complain(rc, err);
        if (inqhost::timing_level())
            for (size_t r = 0; r < st.size(); ++r)
                std::fprintf(stderr,
                             "[inq part] %zu of %zu on device %d: status %d, %llu loci, %llu spans, %.1f MB of BAM read by %d reader threads, rows %.3f s "
                             "(span loop %.3f s = %.2f GB/s, waiting for the loader %.3f s, device calls %.3f s), front end %s\n",
                             r, st.size(), st[r].device, st[r].status, (unsigned long long)st[r].loci, (unsigned long long)st[r].spans,
                             st[r].bam_bytes_read / 1e6, st[r].io_threads, st[r].rows_s, st[r].span_loop_s,
                             st[r].span_loop_s > 0 ? st[r].bam_bytes_read / 1e9 / st[r].span_loop_s : 0.0, st[r].wait_loader_s, st[r].device_calls_s,
                             st[r].front == 2 ? "device" : st[r].front == 1 ? "host" : "-");
        return leave(rc, nullptr);
    }
    if (const char *server_env = std::getenv("INQ_SERVER"); server_env && *server_env) {
        const int status = call_on_server(server_env, a, f);
        if (status >= 0) return status;
    }
    return finish([&](char *err, size_t cap) { return call_here(a, f, devices, nullptr, err, cap); });
}

int main(int argc, char **argv) {
    const std::string cmd = argc >= 2 ? argv[1] : "";
    if (cmd == "combine") return cmd_combine(argc, argv);
    if (cmd == "outlier") return cmd_outlier(argc, argv);
    if (cmd == "assoc") return cmd_assoc(argc, argv);
    if (cmd == "cohort") return cmd_cohort(argc, argv);
    if (cmd == "serve") return cmd_serve(argc, argv);
    if (cmd == "call") return cmd_call(argc, argv);
    if (cmd == "-h" || cmd == "--help") {
        std::puts("Tool to genotype STRs from long reads (MI355X build: `call` only)\n\nUsage: inquistr call [OPTIONS] <BAM>");
        return 0;
    }
    std::fputs("error: this build provides the `call`, `combine`, `outlier`, `assoc` (and `cohort`: many `call`s in one process; `serve`: a process that keeps the device context for `call`s with INQ_SERVER set) subcommands only\n\nUsage: inquistr call [OPTIONS] <BAM>\n", stderr);
    return 2;
}
