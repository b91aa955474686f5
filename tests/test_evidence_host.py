"""Per-locus read evidence (`inquistr call --evidence FILE`, inq_call_args_t.evidence_path) without a GPU: the record's layout in the
header and in the bindings, the text of one line, a path that cannot be written, and the entries that refuse the request."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from inquistr_amd import call, hipcall
from tests.test_tie_report import make_tie_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = (("n_fetched", 0, 4), ("n_kept", 4, 4), ("n_group1", 8, 4), ("n_group2", 12, 4), ("n_clip", 16, 4), ("reserved", 20, 4),
          ("call_min", 24, 8), ("call_max", 32, 8))
HEADER = "chrom\tbegin\tend\tfetched\tkept\th1\th2\tclipped\tmin\tmax"


def test_record_layout_in_header_and_bindings(tmp_path):
    # the header, through a C compiler
    src = tmp_path / "layout.c"
    lines = "".join(f'    printf("{n} %zu %zu\\n", offsetof(inq_locus_evidence_t, {n}), sizeof(((inq_locus_evidence_t *)0)->{n}));\n' for n, _, _ in FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "inquistr_hip.h"\nint main(void) {\n'
                   '    printf("size %zu %d\\n", sizeof(inq_locus_evidence_t), INQ_ABI_VERSION);\n' + lines + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[0] == "size 40 5"
    assert out[1 : 1 + len(FIELDS)] == [f"{n} {o} {s}" for n, o, s in FIELDS]
    # ctypes and numpy
    assert C.sizeof(hipcall.LocusEvidenceC) == 40 == hipcall.EVIDENCE_DTYPE.itemsize
    for n, o, s in FIELDS:
        f = getattr(hipcall.LocusEvidenceC, n)
        assert (f.offset, f.size) == (o, s), n
        assert hipcall.EVIDENCE_DTYPE.fields[n][1] == o and hipcall.EVIDENCE_DTYPE.fields[n][0].itemsize == s, n
    assert hipcall.EVIDENCE_DTYPE.fields["call_min"][0].kind == "i" and hipcall.EVIDENCE_DTYPE.fields["n_clip"][0].kind == "u"
    # the arguments of a call: the new field is the last one
    assert call.CallArgsC._fields_[-1][0] == "evidence_path" and call.CallArgsC._fields_[-2][0] == "ties_path"
    assert call.CallArgsC.evidence_path.offset == call.CallArgsC.ties_path.offset + 8


def _row(chrom, start, end, *vals, cap=512):
    L = call.load()
    e = hipcall.LocusEvidenceC(*vals)
    buf = C.create_string_buffer(cap)
    n = L.inq_host_format_evidence_row(chrom.encode(), start, end, C.byref(e), buf, cap)
    return n, buf.value.decode()


def test_format_evidence_row():
    # (n_fetched, n_kept, n_group1, n_group2, n_clip, reserved, call_min, call_max)
    line = "chr7\t1000\t1050\t9\t6\t3\t3\t1\t0\t20"
    assert _row("chr7", 1000, 1050, 9, 6, 3, 3, 1, 0, 0, 20) == (len(line), line)
    # nobody in either group: `.` for both extremes, whatever the fields hold
    assert _row("chr2", 5000, 5030, 0, 0, 0, 0, 0, 0, 0, 0)[1] == "chr2\t5000\t5030\t0\t0\t0\t0\t0\t.\t."
    assert _row("chr2", 5000, 5030, 4, 2, 0, 0, 0, 0, 77, -3)[1] == "chr2\t5000\t5030\t4\t2\t0\t0\t0\t.\t."
    # one group is enough for numbers; a negative minimum (deletions)
    assert _row("1", 10, 10, 5, 5, 0, 2, 0, 0, -31, -7)[1] == "1\t10\t10\t5\t5\t0\t2\t0\t-31\t-7"
    assert _row("1", 10, 10, 5, 5, 2, 0, 2, 0, -31, 12)[1] == "1\t10\t10\t5\t5\t2\t0\t2\t-31\t12"
    # 2^31-scale and beyond: counts are u32, extremes i64, coordinates u32
    big = _row("chrX", 4294967295, 4294967295, 4294967295, 2147483648, 2147483648, 2147483647, 2147483649, 0, -(1 << 63), (1 << 63) - 1)[1]
    assert big == ("chrX\t4294967295\t4294967295\t4294967295\t2147483648\t2147483648\t2147483647\t2147483649\t"
                   "-9223372036854775808\t9223372036854775807")
    assert _row("c", 1, 2, 1, 1, 1, 0, 0, 0, -2147483649, 2147483648)[1] == "c\t1\t2\t1\t1\t1\t0\t0\t-2147483649\t2147483648"
    # the length is the whole line's, also when the buffer is too small for it (snprintf)
    n, text = _row("chr7", 1000, 1050, 9, 6, 3, 3, 1, 0, 0, 20, cap=8)
    assert n == len(line) and text == line[:7]


def _env():
    e = dict(os.environ)
    e.pop("INQ_SERVER", None)
    return e


def test_cli_unwritable_evidence_path(tmp_path):
    bam, bed, _loci, _recs, _ties = make_tie_case(tmp_path)
    bad = "/nonexistent/dir/e.tsv"
    for extra in ([], ["--devices", "0,0"]):
        r = subprocess.run([call.CLI_PATH, "call", bam, "-R", bed, "-u", "--evidence", bad] + extra, capture_output=True, text=True, env=_env(),
                           timeout=120)
        assert r.returncode == 1, r.stderr
        assert r.stdout == ""
        assert bad in r.stderr and "evidence file" in r.stderr


def test_library_unwritable_evidence_path(tmp_path):
    bam, bed, _loci, _recs, _ties = make_tie_case(tmp_path)
    bad = str(tmp_path / "missing" / "e.tsv")
    out = tmp_path / "o.inq"
    with open(out, "w") as f, pytest.raises(call.CallError) as e:
        call.genotype_repeats(bam, None, bed, 5, 3, 1, True, None, None, out=f, evidence=bad)
    assert e.value.status == 1 and bad in e.value.message and "evidence file" in e.value.message
    assert out.read_text() == ""
    with open(out, "w") as f, pytest.raises(call.CallError) as e:
        call.genotype_repeats_devices(bam, None, bed, [0, 0], 5, 3, 1, True, None, out=f, evidence=bad)
    assert e.value.status == 1 and bad in e.value.message
    assert out.read_text() == ""


def test_cli_evidence_with_a_server_is_refused(tmp_path):
    """Exit status 2 before any server is looked for: the socket named here does not exist, and a call without --evidence would run
    (and fail for want of a GPU or succeed) here instead."""
    bam, bed, _loci, _recs, _ties = make_tie_case(tmp_path)
    ev = tmp_path / "e.tsv"
    env = _env()
    env["INQ_SERVER"] = str(tmp_path / "no.sock")
    r = subprocess.run([call.CLI_PATH, "call", bam, "-R", bed, "--evidence", str(ev)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 2, r.stderr
    assert r.stdout == "" and "--evidence" in r.stderr and "INQ_SERVER" in r.stderr
    assert not ev.exists()
    # the flag needs a value
    r = subprocess.run([call.CLI_PATH, "call", bam, "-R", bed, "--evidence"], capture_output=True, text=True, env=_env(), timeout=120)
    assert r.returncode == 2
    # ... and belongs to `call` alone
    r = subprocess.run([call.CLI_PATH, "cohort", "-R", bed, "--evidence", str(ev), "--out-dir", str(tmp_path), bam], capture_output=True, text=True,
                       env=_env(), timeout=120)
    assert r.returncode == 2 and "--evidence" in r.stderr


def test_sessions_runs_and_rows_refuse_evidence(tmp_path):
    bam, bed, loci, _recs, _ties = make_tie_case(tmp_path)
    L = call.load()
    ev = tmp_path / "e.tsv"
    a = call._args(bam, None, bed, 5, 3, 1, True, None, None, evidence=str(ev))
    err = C.create_string_buffer(1024)
    # a prepared run
    h = C.c_void_p()
    assert L.inq_run_open(C.byref(a), C.byref(h), err, len(err)) == 1
    assert not h.value and b"evidence" in err.value
    # ... also on a session, and the session's own calls (no device is touched before the refusal)
    sess = call.Session(0)
    try:
        err = C.create_string_buffer(1024)
        assert L.inq_session_run_open(sess._h, C.byref(a), C.byref(h), err, len(err)) == 1
        assert not h.value and b"evidence" in err.value
        out = tmp_path / "s.inq"
        with open(out, "w") as f:
            err = C.create_string_buffer(1024)
            assert L.inq_session_call(sess._h, C.byref(a), f.fileno(), err, len(err)) == 1
            assert b"evidence" in err.value
            st = (C.c_int * 1)()
            fds = (C.c_int * 1)(f.fileno())
            err = C.create_string_buffer(1024)
            assert L.inq_session_call_many(sess._h, C.byref(a), 1, fds, st, err, len(err)) == 1
            assert st[0] == 1 and b"evidence" in err.value
        assert out.read_text() == ""
    finally:
        sess.close()
    # rows instead of text
    idx = np.arange(len(loci), dtype=np.uint32)
    p1, p2 = np.zeros(len(loci)), np.zeros(len(loci))
    err = C.create_string_buffer(1024)
    assert L.inq_genotype_repeats_rows(C.byref(a), idx.ctypes.data, len(idx), p1.ctypes.data, p2.ctypes.data, err, len(err)) == 1
    assert b"evidence" in err.value
    assert not ev.exists()
    # the same arguments without the field open as always
    run = call.Run(bam, None, bed)
    assert run.n_targets == len(loci)
    run.close()
