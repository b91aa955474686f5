"""The per-read Calls behind each row (`inquistr call --read-calls FILE`, inq_genotype_repeats_reads) without a GPU: the record's layout
in the header and in the bindings, the text of one line against a plain-Python restatement, the invariant that ties the file to the
.inq (median_str_length of the parsed h1 / h2 is the row), a path that cannot be written, and a call with INQ_SERVER set."""
import ctypes as C
import math
import os
import random
import subprocess

import numpy as np
import pytest

from inquistr_amd import call, hipcall
from oracle import pyoracle as py
from tests.test_tie_report import make_tie_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = (("call", 0, 8), ("read", 8, 4), ("group", 12, 1), ("flags", 13, 1), ("reserved", 14, 2))
HEADER = "chrom\tbegin\tend\th1\th2\tother"
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


# ---- the file, restated: a Call is (kind, value, group) with kind "Span" / "Clip", in file order ------------------------------------
def split_calls(calls, unphased):
    """(h1, h2, other): what median_str_length is handed for phase1 / phase2 (src/call.rs:312-314 / :358), and the kept reads of HP 0;
    each ascending by (value, file order)"""
    by_value = lambda lst: sorted(lst, key=lambda c: c[1])  # (stable: equal values stay in file order)
    if unphased:
        s = by_value(calls)
        return s[: len(s) // 2], s[len(s) // 2 :], []
    return tuple(by_value([c for c in calls if pick(c[2])]) for pick in (lambda g: g == 1, lambda g: g == 2, lambda g: g not in (1, 2)))


def list_text(calls):
    return ",".join(f"{c[1]}c" if c[0] == "Clip" else str(c[1]) for c in calls) if calls else "."


def row_text(chrom, start, end, calls, unphased):
    return f"{chrom}\t{start}\t{end}\t" + "\t".join(list_text(part) for part in split_calls(calls, unphased))


def parse_list(text):
    """one list of the file -> [(kind, value)], as median_str_length takes them"""
    if text == ".":
        return []
    return [("Clip", int(t[:-1])) if t.endswith("c") else ("Span", int(t)) for t in text.split(",")]


def records(calls):
    """[(kind, value, group)] -> inq_read_call_t records (read = the position in the list)"""
    rec = np.zeros(len(calls), dtype=hipcall.READ_CALL_DTYPE)
    for i, (kind, value, group) in enumerate(calls):
        rec[i] = (value, i, group, hipcall.READ_CALL_CLIP if kind == "Clip" else 0, 0)
    return rec


def library_row(chrom, start, end, calls, unphased, cap=1 << 16):
    L = call.load()
    rec = records(calls)
    buf = C.create_string_buffer(cap)
    n = L.inq_host_format_read_calls_row(chrom.encode(), start, end, rec.ctypes.data if len(rec) else None, len(rec), 1 if unphased else 0, buf, cap)
    return n, buf.value.decode()


def same_f64(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


# ---- the record ---------------------------------------------------------------------------------------------------------------------
def test_record_layout_in_header_and_bindings(tmp_path):
    src = tmp_path / "layout.c"
    lines = "".join(f'    printf("{n} %zu %zu\\n", offsetof(inq_read_call_t, {n}), sizeof(((inq_read_call_t *)0)->{n}));\n' for n, _, _ in FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "inquistr_hip.h"\nint main(void) {\n'
                   '    printf("size %zu %d %u\\n", sizeof(inq_read_call_t), INQ_ABI_VERSION, INQ_READ_CALL_CLIP);\n' + lines + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[0] == "size 16 5 1"
    assert out[1 : 1 + len(FIELDS)] == [f"{n} {o} {s}" for n, o, s in FIELDS]
    assert C.sizeof(hipcall.ReadCallC) == 16 == hipcall.READ_CALL_DTYPE.itemsize
    for n, o, s in FIELDS:
        f = getattr(hipcall.ReadCallC, n)
        assert (f.offset, f.size) == (o, s), n
        assert hipcall.READ_CALL_DTYPE.fields[n][1] == o and hipcall.READ_CALL_DTYPE.fields[n][0].itemsize == s, n
    assert hipcall.READ_CALL_DTYPE.fields["call"][0].kind == "i" and hipcall.READ_CALL_DTYPE.fields["read"][0].kind == "u"
    assert hipcall.READ_CALL_CLIP == 1
    # the arguments of a call did not grow: the file has an entry of its own
    assert call.CallArgsC._fields_[-1][0] == "evidence_path"
    assert hasattr(call.load(), "inq_genotype_repeats_reads")


# ---- one line -----------------------------------------------------------------------------------------------------------------------
S, K = "Span", "Clip"
ROW_CASES = [
    # (name, calls in file order, unphased, the line behind chrom / begin / end, written by hand)
    ("nothing, phased", [], False, ".\t.\t."),
    ("nothing, unphased", [], True, ".\t.\t."),
    ("one read, unphased: len / 2 = 0", [(S, 5, 0)], True, ".\t5\t."),
    ("one read of HP 2", [(S, 5, 2)], False, ".\t5\t."),
    ("the issue's example", [(K, 12, 1), (S, 7, 1), (S, -20, 1), (S, 0, 1)], False, "-20,0,7,12c\t.\t."),
    ("negative Calls", [(S, -7, 1), (S, -31, 2), (K, -2, 2), (S, -30, 1)], False, "-30,-7\t-31,-2c\t."),
    ("beyond 2^32 and the i64 ends", [(S, I64_MAX, 1), (S, 1 << 32, 1), (K, I64_MIN, 1), (S, -(1 << 32) - 1, 2), (K, I64_MAX, 2)], False,
     f"{I64_MIN}c,{1 << 32},{I64_MAX}\t{-(1 << 32) - 1},{I64_MAX}c\t."),
    ("phased with HP 0 reads", [(S, 3, 0), (S, 9, 1), (K, 1, 0), (S, 4, 2), (S, 2, 1), (S, -5, 0)], False, "2,9\t4\t-5,1c,3"),
    ("HP 0 only", [(S, 3, 0), (K, 3, 0)], False, ".\t.\t3,3c"),
    ("unphased, odd", [(S, 9, 0), (S, 1, 0), (K, 5, 0), (S, 3, 0), (S, 7, 0)], True, "1,3\t5c,7,9\t."),
    ("unphased, even", [(S, 9, 0), (S, 1, 0), (K, 5, 0), (S, 3, 0)], True, "1,3\t5c,9\t."),
    ("unphased: the HP does not matter", [(S, 9, 2), (S, 1, 1), (K, 5, 0), (S, 3, 2)], True, "1,3\t5c,9\t."),
    # equal values of mixed Span / Clip across the split: file order decides which of them h1 takes
    ("tie, the Clip first in the file", [(S, 1, 0), (K, 4, 0), (S, 4, 0), (S, 8, 0)], True, "1,4c\t4,8\t."),
    ("tie, the Span first in the file", [(S, 1, 0), (S, 4, 0), (K, 4, 0), (S, 8, 0)], True, "1,4\t4c,8\t."),
    ("tie of five around an odd split", [(K, 4, 0), (S, 4, 0), (K, 4, 0), (S, 4, 0), (S, 4, 0)], True, "4c,4\t4c,4,4\t."),
    ("phased ties keep file order inside a group", [(K, 4, 1), (S, 4, 1), (S, 4, 2), (K, 4, 2), (S, 4, 1)], False, "4c,4,4\t4,4c\t."),
]


@pytest.mark.parametrize("name,calls,unphased,want", ROW_CASES, ids=[c[0] for c in ROW_CASES])
def test_format_read_calls_row(name, calls, unphased, want):
    line = "chr7\t1000\t1050\t" + want
    assert row_text("chr7", 1000, 1050, calls, unphased) == line, "the restatement against the hand-written line"
    assert library_row("chr7", 1000, 1050, calls, unphased) == (len(line), line)


def test_format_row_coordinates_and_small_buffer():
    calls = [(K, 12, 1), (S, 7, 1), (S, -20, 2)]
    line = "chrX\t4294967295\t4294967295\t7,12c\t-20\t."
    assert library_row("chrX", 4294967295, 4294967295, calls, False) == (len(line), line)
    # the length is the whole line's, also when the buffer is too small for it (snprintf)
    n, text = library_row("chrX", 4294967295, 4294967295, calls, False, cap=8)
    assert n == len(line) and text == line[:7]
    n, text = library_row("chrX", 4294967295, 4294967295, calls, False, cap=1)
    assert n == len(line) and text == ""


def _random_calls(rng):
    n = rng.choice([0, 1, 2, 3, 4, 5, 6, 7, 9, 12, 20, 33])
    few = rng.random() < 0.5  # few distinct values: ties of mixed Span / Clip at the split
    return [(K if rng.random() < 0.3 else S, rng.randint(-3, 3) if few else rng.randint(-500, 500), rng.choice([0, 1, 1, 2, 2])) for _ in range(n)]


@pytest.mark.parametrize("unphased", [False, True])
def test_medians_of_the_parsed_lists_are_the_row(unphased):
    """The invariant that ties the file to the .inq: median_str_length of the parsed h1 / h2 is what the reference's per-locus function
    computes from the same Calls (pyoracle.genotype_repeat_phased / _unphased: the grouping by HP, the stable sort and the split)."""
    rng = random.Random(20_250 + unphased)
    tie_splits = 0
    for _ in range(200):
        calls = _random_calls(rng)
        n, text = library_row("c", 10, 20, calls, unphased)
        assert n == len(text) and text == row_text("c", 10, 20, calls, unphased)
        h1, h2, other = (parse_list(t) for t in text.split("\t")[3:])
        kv = [(k, v) for k, v, _g in calls]
        if unphased:
            s = sorted(kv, key=lambda c: c[1])
            k = len(s) // 2
            g1, g2 = s[:k], s[k:]
            assert other == []
            tie_splits += 1 <= k < len(s) and s[k - 1][1] == s[k][1] and s[k - 1][0] != s[k][0]
        else:
            g1, g2 = [(k, v) for k, v, g in calls if g == 1], [(k, v) for k, v, g in calls if g == 2]
            assert len(other) == sum(1 for c in calls if c[2] == 0)
        assert len(h1) == len(g1) and len(h2) == len(g2)
        for support in (1, 3, 5):
            assert same_f64(py.median_str_length(h1, support), py.median_str_length(g1, support)), (calls, support)
            assert same_f64(py.median_str_length(h2, support), py.median_str_length(g2, support)), (calls, support)
    assert not unphased or tie_splits > 5, "the lists reach the tie rule"


# ---- the command line and the entry ---------------------------------------------------------------------------------------------------
def _env():
    e = dict(os.environ)
    e.pop("INQ_SERVER", None)
    return e


def test_cli_unwritable_read_calls_path(tmp_path):
    bam, bed, _loci, _recs, _ties = make_tie_case(tmp_path)
    bad = "/nonexistent/dir/r.tsv"
    for extra in ([], ["--devices", "0,0"]):
        r = subprocess.run([call.CLI_PATH, "call", bam, "-R", bed, "-u", "--read-calls", bad] + extra, capture_output=True, text=True, env=_env(),
                           timeout=120)
        assert r.returncode == 1, r.stderr
        assert r.stdout == ""
        assert bad in r.stderr and "read-calls file" in r.stderr


def test_library_unwritable_read_calls_path(tmp_path):
    bam, bed, _loci, _recs, _ties = make_tie_case(tmp_path)
    bad = str(tmp_path / "missing" / "r.tsv")
    out = tmp_path / "o.inq"
    for devices in (None, [0, 0]):
        with open(out, "w") as f, pytest.raises(call.CallError) as e:
            call.genotype_repeats(bam, None, bed, 5, 3, 1, True, None, None, out=f, read_calls=bad, devices=devices)
        assert e.value.status == 1 and bad in e.value.message and "read-calls file" in e.value.message
        assert out.read_text() == ""
    # the other two files are opened first, beside it
    ev = tmp_path / "e.tsv"
    with open(out, "w") as f, pytest.raises(call.CallError):
        call.genotype_repeats(bam, None, bed, 5, 3, 1, True, None, None, out=f, evidence=str(ev), read_calls=bad)
    assert ev.exists() and out.read_text() == ""


def test_cli_read_calls_with_a_server_is_refused(tmp_path):
    """Exit status 2 before any server is looked for: the socket named here does not exist, and a call without --read-calls would run
    here instead."""
    bam, bed, _loci, _recs, _ties = make_tie_case(tmp_path)
    rc_file = tmp_path / "r.tsv"
    env = _env()
    env["INQ_SERVER"] = str(tmp_path / "no.sock")
    r = subprocess.run([call.CLI_PATH, "call", bam, "-R", bed, "--read-calls", str(rc_file)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 2, r.stderr
    assert r.stdout == "" and "--read-calls" in r.stderr and "INQ_SERVER" in r.stderr
    assert not rc_file.exists()
    # the flag needs a value, has a help line ...
    r = subprocess.run([call.CLI_PATH, "call", bam, "-R", bed, "--read-calls"], capture_output=True, text=True, env=_env(), timeout=120)
    assert r.returncode == 2
    r = subprocess.run([call.CLI_PATH, "call", "--help"], capture_output=True, text=True, env=_env(), timeout=120)
    assert r.returncode == 0 and "--read-calls <FILE>" in r.stdout
    # ... and belongs to `call` alone
    r = subprocess.run([call.CLI_PATH, "cohort", "-R", bed, "--read-calls", str(rc_file), "--out-dir", str(tmp_path), bam], capture_output=True,
                       text=True, env=_env(), timeout=120)
    assert r.returncode == 2 and "--read-calls" in r.stderr


def _outcome(fn):
    try:
        fn()
        return None
    except call.CallError as e:
        return (e.status, e.message)


def test_new_entry_fails_as_loudly_as_the_old_one(tmp_path):
    """Where there is no GPU the entry ends as inq_genotype_repeats does: the same status, the same message, nothing on stdout (where
    there is one, both succeed with the same text)."""
    bam, bed, _loci, _recs, _ties = make_tie_case(tmp_path)
    a, b, rc_file = tmp_path / "a.inq", tmp_path / "b.inq", tmp_path / "r.tsv"
    with open(a, "w") as f:
        plain = _outcome(lambda: call.genotype_repeats(bam, None, bed, 5, 3, 1, True, None, None, out=f))
    with open(b, "w") as f:
        new = _outcome(lambda: call.genotype_repeats(bam, None, bed, 5, 3, 1, True, None, None, out=f, read_calls=str(rc_file)))
    assert new == plain
    assert a.read_text() == b.read_text()
    if plain is not None:
        assert plain[0] != 0 and plain[1] and b.read_text() == ""
    assert rc_file.exists()  # opened before any device work
