"""Every word the command line says, held to what the commit before said: exit status, standard output and standard error, byte for byte.

`tests/golden/cli_parent_messages.json` was recorded from the parent commit's `inquistr` + host library on a machine without a device:
the usage errors of every subcommand (exit status 2), the six `INQ_SERVER` refusals, and every input failure of `assoc` and `outlier`
(exit status 101) with its full message.  All inputs stand at fixed relative names in the working directory, so no recorded text names a
temporary path.  Two cases (DEVICE_CASES: `outlier` on a file whose bad line comes after a good one) get as far as the device: without
one they end in the "no CPU fallback" failure, which is what the record holds; with one they print the good lines' output and then
panic, and `tests/golden/assoc_parent_output.json` (recorded from the parent commit on an MI355X) holds them to that, beside a dozen
whole runs of `assoc` on the small cohort `tests/golden/assoc_cohort.inq`."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CLI = os.path.join(ROOT, "inquistr_amd", "lib", "inquistr")

NAMES = [f"S{i}" for i in range(8)]
HEAD = "chromosome\tbegin\tend\t" + "\t".join(f"{n}_H{h}" for n in NAMES for h in (1, 2))
# five loci of sixteen values (8 samples x 2 haplotypes), as fixed text
ROWS = [f"chr{1 + i % 2}\t{100 * i}\t{100 * i + 20}\t" + "\t".join(str(5 + (7 * i + 3 * k + k * k) % 15) for k in range(16)) for i in range(5)]
DEVICE_CASES = ("outlier: two fields after a good line", "outlier: unparseable number after a good line")


def write_inputs(d):
    """the inputs of every case, at fixed names under d (the working directory of every run)"""
    def put(name, text):
        with open(os.path.join(d, name), "w") as f:
            f.write(text)

    put("c.tsv", HEAD + "\n" + "\n".join(ROWS) + "\n")
    put("p.tsv", "individual\tgrp\tage\tw\n" + "".join(f"{n}\t{'Y' if i % 2 else 'N'}\t{30 + i}\t{'NA' if i == 3 else i * 1.5}\n"
                                                       for i, n in enumerate(NAMES[:7])) + "ZZ\tY\t1\t1\n")
    put("bad.tsv", HEAD + "\n" + ROWS[0] + "\n" + ROWS[1].replace("\t", "\tx", 4).replace("\tx", "\t", 3) + "\n" + ROWS[2] + "\n")
    put("short.tsv", HEAD + "\n" + ROWS[0] + "\nchr1\t5\n" + ROWS[2] + "\n")
    put("odd.tsv", HEAD + "\tS9_H1\n" + ROWS[0] + "\t3\n")
    put("empty.tsv", "")
    put("nosamples.tsv", "chromosome\tbegin\tend\n" + "chr1\t1\t2\n")
    put("subset.txt", "S1\nS2\n")


def cases():
    """(name, arguments after `inquistr`, extra environment)"""
    out = []

    def add(name, *args, env=None):
        out.append((name, [str(a) for a in args], env or {}))

    def both(name, cmd, front, key, value):  # `--key value` and `--key=value`
        add(f"{name}, two words", cmd, *front, key, value)
        add(f"{name}, one word", cmd, *front, f"{key}={value}")

    # 1. the top level
    add("no subcommand")
    add("bogus subcommand", "bogus")
    add("top -h", "-h")
    add("top --help", "--help")
    # 2. usage errors
    add("outlier: no positional", "outlier")
    add("outlier: flag without value", "outlier", "c.tsv", "--minsize")
    add("outlier: unknown flag", "outlier", "c.tsv", "--bogus")
    add("outlier: unknown flag with value", "outlier", "c.tsv", "--bogus=1")
    add("outlier: second positional", "outlier", "c.tsv", "d.tsv")
    add("outlier: -h is no flag", "outlier", "-h")
    both("outlier: bad --method", "outlier", ["c.tsv"], "--method", "kmeans")
    base = ["--phenocovar", "p.tsv", "--phenotype", "grp", "--outcome", "binary", "--binary-order", "N,Y"]
    add("assoc: no arguments", "assoc")
    add("assoc: no positional", "assoc", *base)
    add("assoc: no outcome", "assoc", "c.tsv", "--phenocovar", "p.tsv", "--phenotype", "grp")
    add("assoc: flag without value", "assoc", "c.tsv", "--phenocovar")
    add("assoc: unknown flag", "assoc", "c.tsv", *base, "--bogus")
    add("assoc: unknown flag with value", "assoc", "c.tsv", *base, "--bogus=1")
    add("assoc: second positional", "assoc", "c.tsv", "d.tsv", *base)
    both("assoc: bad --outcome", "assoc", ["c.tsv"], "--outcome", "ordinal")
    both("assoc: bad --str-mode", "assoc", ["c.tsv"], "--str-mode", "median")
    both("assoc: bad --missing-cutoff", "assoc", ["c.tsv", *base], "--missing-cutoff", "abc")
    both("assoc: bad --chr-begin", "assoc", ["c.tsv", *base], "--chr-begin", "1x")
    both("assoc: bad --device", "assoc", ["c.tsv", *base], "--device", "x")
    add("assoc: empty --device", "assoc", "c.tsv", *base, "--device=")
    add("assoc -h", "assoc", "-h")
    add("assoc --help after arguments", "assoc", "c.tsv", "--help")
    add("call: no arguments", "call")
    add("call: no positional", "call", "-r", "chr1:1-2")
    add("call: flag without value", "call", "x.bam", "--minlen")
    add("call: unknown flag", "call", "x.bam", "--bogus")
    add("call: unknown flag with value", "call", "x.bam", "--bogus=1")
    add("call: second positional", "call", "x.bam", "y.bam")
    add("call -h", "call", "x.bam", "-h")
    both("call: negative --minlen", "call", ["x.bam"], "--minlen", "-3")
    both("call: bad --threads", "call", ["x.bam"], "--threads", "4x")
    both("call: bad --devices", "call", ["x.bam"], "--devices", "0,x")
    add("call: empty --support", "call", "x.bam", "--support=")
    add("call: --ctx-option without its value", "call", "x.bam", "--ctx-option")
    both("call: --ctx-option without =", "call", ["x.bam"], "--ctx-option", "novalue")
    both("call: --ctx-option with an empty key", "call", ["x.bam"], "--ctx-option", "=5")
    both("call: --ctx-option with an empty value", "call", ["x.bam"], "--ctx-option", "k=")
    both("call: --ctx-option with a bad number", "call", ["x.bam"], "--ctx-option", "k=1x")
    add("cohort: no --out-dir", "cohort", "x.bam")
    add("cohort: no BAM", "cohort", "--out-dir", "out")
    add("cohort: --device=1", "cohort", "--device=1", "--out-dir", "out", "x.bam")
    add("cohort: unknown flag", "cohort", "--out-dir", "out", "--bogus", "x.bam")
    add("cohort: flag without value", "cohort", "x.bam", "--out-dir")
    add("cohort: --read-table", "cohort", "--out-dir", "out", "--read-table", "t.txt", "x.bam")
    add("cohort: --read-seqs", "cohort", "--out-dir", "out", "x.bam", "--read-seqs", "s.txt")
    add("serve: no socket", "serve")
    add("serve: stray word", "serve", "--socket", "s.sock", "stray")
    add("serve: --socket=s.sock", "serve", "--socket=s.sock")
    add("serve: flag without value", "serve", "--socket")
    # 3. what a call handed to a server cannot write: said before a server is looked for (nothing listens at no.sock)
    server = {"INQ_SERVER": "no.sock"}
    for flag in ("--evidence", "--read-calls", "--read-table", "--read-seqs", "--read-motifs", "--locus-motifs"):
        add(f"server: {flag}", "call", "x.bam", flag, "f.txt", env=server)
    add("server: --locus-motifs and --read-table", "call", "x.bam", "--locus-motifs", "l.txt", "--read-table=t.txt", env=server)
    add("server: --read-motifs and --evidence", "call", "--read-motifs", "m.txt", "x.bam", "--evidence", "e.txt", env=server)
    # 4. input failures: the reference's panics, exit status 101
    add("assoc: no combined file", "assoc", "missing.tsv", *base)
    add("assoc: no phenotype file", "assoc", "c.tsv", "--phenocovar", "missing.tsv", "--phenotype", "grp", "--outcome", "continuous")
    add("assoc: no --binary-order", "assoc", "c.tsv", "--phenocovar", "p.tsv", "--phenotype", "grp", "--outcome", "binary")
    add("assoc: one value in --binary-order", "assoc", "c.tsv", "--phenocovar", "p.tsv", "--phenotype", "grp", "--outcome", "binary", "--binary-order", "N")
    add("assoc: phenotype is no column", "assoc", "c.tsv", "--phenocovar", "p.tsv", "--phenotype", "nope", "--outcome", "continuous")
    add("assoc: covariate is no column", "assoc", "c.tsv", *base, "--covariates", "age,height")
    add("assoc: seven covariates", "assoc", "c.tsv", *base, "--covariates", "a,b,c,d,e,f,g")
    add("assoc: no numbers in the phenotype", "assoc", "c.tsv", "--phenocovar", "p.tsv", "--phenotype", "grp", "--outcome", "continuous")
    add("assoc: no sample in either group", "assoc", "c.tsv", "--phenocovar", "p.tsv", "--phenotype", "grp", "--outcome", "binary", "--binary-order", "P,Q")
    add("assoc: --chr-begin alone", "assoc", "c.tsv", *base, "--chr", "chr1", "--chr-begin", "5")
    add("assoc: --chr-begin without --chr", "assoc", "c.tsv", *base, "--chr-begin", "5", "--chr-end", "9")
    add("assoc: unparseable number", "assoc", "bad.tsv", *base)
    add("assoc: two fields", "assoc", "short.tsv", *base)
    add("assoc: odd sample columns", "assoc", "odd.tsv", *base)
    add("assoc: empty file", "assoc", "empty.tsv", *base)
    add("assoc: empty phenotype file", "assoc", "c.tsv", "--phenocovar", "empty.tsv", "--phenotype", "grp", "--outcome", "continuous")
    add("assoc: header without samples", "assoc", "nosamples.tsv", *base)
    add("assoc: --firth maybe", "assoc", "c.tsv", *base, "--firth", "maybe")
    add("assoc: --firth always, continuous", "assoc", "c.tsv", "--phenocovar", "p.tsv", "--phenotype", "age", "--outcome", "continuous", "--firth=always")
    add("assoc: NaN cutoff", "assoc", "c.tsv", *base, "--missing-cutoff", "nan")
    add("outlier: no file", "outlier", "missing.tsv")
    add("outlier: -s with -S", "outlier", "c.tsv", "-s", "S1", "-S", "subset.txt")
    add("outlier: no subset file", "outlier", "c.tsv", "--subset=missing.txt")
    add("outlier: empty file", "outlier", "empty.tsv")
    add("outlier: header without samples", "outlier", "nosamples.tsv", "--method", "dbscan")
    add(DEVICE_CASES[0], "outlier", "short.tsv", "--minsize", "0", "-z", "1.0")
    add(DEVICE_CASES[1], "outlier", "bad.tsv", "--minsize=0", "--zscore=1.0", "--method=dbscan")
    return out


def run(cli, args, env, cwd):
    e = {k: v for k, v in os.environ.items() if k not in ("INQ_SERVER", "INQ_TIMING", "INQ_FAST_EXIT", "INQ_HOST_LIB")}
    e.update(env)
    r = subprocess.run([cli] + args, capture_output=True, text=True, cwd=cwd, env=e)
    return {"status": r.returncode, "stdout": r.stdout, "stderr": r.stderr}


def _have_gpu():
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:
        return False


def test_every_message_is_the_parents(tmp_path):
    rec = json.load(open(os.path.join(GOLDEN, "cli_parent_messages.json")))
    all_cases = cases()
    assert sorted(rec) == sorted(name for name, _, _ in all_cases)
    write_inputs(tmp_path)
    on_device = _have_gpu()
    for name, args, env in all_cases:
        if on_device and name in DEVICE_CASES:
            continue  # they get past the "no CPU fallback" failure there: test_outlier_prints_before_a_late_panic holds them
        assert run(CLI, args, env, tmp_path) == rec[name], name


# the runs of `assoc` on tests/golden/assoc_cohort.inq: 36 samples (one of them NaN at every locus, one with a third group, one
# without a score, one the phenotype file does not list) x 28 loci (a constant one, a low-call-rate one, a one-group one, two separated ones)
ASSOC_BINARY = ["--phenocovar", "assoc_cohort_pheno.tsv", "--phenotype", "group", "--outcome", "binary", "--binary-order", "Control,Patient"]
ASSOC_CONTINUOUS = ["--phenocovar", "assoc_cohort_pheno.tsv", "--phenotype", "score", "--outcome", "continuous"]
ASSOC_RUNS = {
    "binary": ["assoc_cohort.inq", *ASSOC_BINARY],
    "binary, covariates": ["assoc_cohort.inq", *ASSOC_BINARY, "--covariates", "age,sex"],
    "continuous": ["assoc_cohort.inq", *ASSOC_CONTINUOUS],
    "continuous, covariates": ["assoc_cohort.inq", *ASSOC_CONTINUOUS, "--covariates=age,sex"],
    "binary, min": ["assoc_cohort.inq", *ASSOC_BINARY, "--str-mode", "min"],
    "continuous, mean": ["assoc_cohort.inq", *ASSOC_CONTINUOUS, "--str-mode=mean", "--covariates", "age"],
    "binary, all rows": ["assoc_cohort.inq", *ASSOC_BINARY, "--all-rows", "--covariates", "age"],
    "continuous, all rows": ["assoc_cohort.inq", *ASSOC_CONTINUOUS, "--all-rows"],
    "binary, chr2": ["assoc_cohort.inq", *ASSOC_BINARY, "--chr", "chr2"],
    "binary, part of chr1": ["assoc_cohort.inq", *ASSOC_BINARY, "--chr", "chr1", "--chr-begin", "2000", "--chr-end", "8000", "--all-rows"],
    "binary, no locus": ["assoc_cohort.inq", *ASSOC_BINARY, "--chr", "chrX"],
    "firth fallback": ["assoc_cohort.inq", *ASSOC_BINARY, "--firth", "fallback", "--all-rows"],
    "firth always": ["assoc_cohort.inq", *ASSOC_BINARY, "--firth=always", "--covariates", "age,sex"],
    "gzip, binary": ["assoc_cohort.inq.gz", *ASSOC_BINARY, "--covariates", "age,sex", "--all-rows"],
    "gzip, continuous": ["assoc_cohort.inq.gz", *ASSOC_CONTINUOUS],
    "low cutoff": ["assoc_cohort.inq", *ASSOC_BINARY, "--missing-cutoff", "0.3", "--all-rows"],
}


@pytest.mark.gpu
def test_assoc_prints_what_the_commit_before_printed():
    rec = json.load(open(os.path.join(GOLDEN, "assoc_parent_output.json")))["assoc"]
    assert sorted(rec) == sorted(ASSOC_RUNS)
    for name, args in ASSOC_RUNS.items():
        got = run(CLI, ["assoc"] + args, {}, GOLDEN)
        assert got == rec[name], name
        assert got["status"] == 0 and got["stdout"].count("\n") >= 1, name


@pytest.mark.gpu
def test_outlier_prints_before_a_late_panic(tmp_path):
    """DEVICE_CASES on the device: the loci in front of the bad line are computed and printed, then the panic"""
    rec = json.load(open(os.path.join(GOLDEN, "assoc_parent_output.json")))["outlier"]
    assert sorted(rec) == sorted(DEVICE_CASES)
    write_inputs(tmp_path)
    for name, args, env in cases():
        if name in DEVICE_CASES:
            got = run(CLI, args, env, tmp_path)
            assert got == rec[name], name
            assert got["status"] == 101 and got["stdout"].startswith("chrom\tbegin\tend\toutliers\n"), name
