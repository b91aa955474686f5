"""The read table (`inquistr call --read-table FILE`, inq_genotype_repeats_table) without a GPU: the lines of one target against
hand-written text, inq_read_origin_t's layout in the header and in the bindings, the names the host sweep keeps for its batches, the
command line, a path that cannot be written, and the entry's failure where there is no GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from inquistr_amd import call, hipcall
from oracle import pyoracle as py
from tests.read_table_case import TABLE_HEADER, table_lines
from tests.test_read_calls_host import records
from tests.test_tie_report import make_tie_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = (("pos", 0, 4), ("mapq", 4, 1), ("bits", 5, 1), ("name_len", 6, 2))
S, K = "Span", "Clip"
REV = 0x10


# ---- the lines of one target -----------------------------------------------------------------------------------------------------------
def library_rows(chrom, start, end, reads, unphased, cap=1 << 16):
    """reads: (kind, value, HP, name, pos, flag, mapq) in file order, as tests.read_table_case.file_reads gives them"""
    L = call.load()
    rec = records([r[:3] for r in reads])
    org = np.zeros(len(reads), dtype=hipcall.ORIGIN_DTYPE)
    raw = b""
    for i, (_k, _v, _g, name, pos, flag, mapq) in enumerate(reads):
        nb = name.encode("latin1")
        org[i] = (pos, mapq, (hipcall_bits(flag)), len(nb))
        raw += nb
    names = np.frombuffer(raw + b"\xff", dtype=np.uint8)  # (a byte behind the last name that must not be read into a line)
    buf = C.create_string_buffer(cap)
    n = L.inq_host_format_read_table_rows(chrom.encode(), start, end, rec.ctypes.data if len(rec) else None, org.ctypes.data if len(org) else None,
                                          names.ctypes.data, len(rec), 1 if unphased else 0, buf, cap)
    return n, buf.value.decode("latin1")


def hipcall_bits(flag):
    from inquistr_amd import batch as B

    return (B.INQ_READ_REVERSE if flag & REV else 0) | (B.INQ_READ_UNMAPPED if flag & 4 else 0) | B.INQ_READ_HAS_HP


ROW_CASES = [
    ("no kept read", [], False, ""),
    ("no kept read, unphased", [], True, ""),
    ("phased, all three groups, both strands",
     [(K, 12, 1, "readA", 99, 0, 60), (S, 7, 0, "q", 104, REV, 11), (S, -20, 1, "readB/1", 100, REV, 255), (S, 0, 2, "c" * 254, 0, 0, 0),
      (S, 3, 2, "zz", 2147483646, 0, 20)], False,
     "c7\t10\t50\th1\t-20\tSpan\treadB/1\t101\t-\t255\n" "c7\t10\t50\th1\t12\tClip\treadA\t100\t+\t60\n"
     "c7\t10\t50\th2\t0\tSpan\t" + "c" * 254 + "\t1\t+\t0\n" "c7\t10\t50\th2\t3\tSpan\tzz\t2147483647\t+\t20\n"
     "c7\t10\t50\tother\t7\tSpan\tq\t105\t-\t11\n"),
    ("unphased, odd: len / 2 = 2 lines of h1, then three of h2, never `other`",
     [(S, 9, 2, "e", 5, 0, 60), (S, 1, 1, "a", 1, REV, 60), (K, 5, 0, "c", 3, 0, 60), (S, 3, 0, "b", 2, 0, 60), (S, 7, 0, "d", 4, REV, 60)], True,
     "c7\t10\t50\th1\t1\tSpan\ta\t2\t-\t60\n" "c7\t10\t50\th1\t3\tSpan\tb\t3\t+\t60\n" "c7\t10\t50\th2\t5\tClip\tc\t4\t+\t60\n"
     "c7\t10\t50\th2\t7\tSpan\td\t5\t-\t60\n" "c7\t10\t50\th2\t9\tSpan\te\t6\t+\t60\n"),
    ("one read, unphased: it is h2's", [(S, 5, 0, "only", 7, 0, 30)], True, "c7\t10\t50\th2\t5\tSpan\tonly\t8\t+\t30\n"),
    ("an empty name is `*`, and so is a leading NUL; a NUL inside cuts the name",
     [(S, 1, 1, "", 10, 0, 60), (S, 2, 1, "\0abc", 11, 0, 60), (S, 3, 1, "ab\0cd", 12, REV, 60), (S, 4, 1, "*", 13, 0, 60), (S, 5, 1, "tail", 14, 0, 60)], False,
     "c7\t10\t50\th1\t1\tSpan\t*\t11\t+\t60\n" "c7\t10\t50\th1\t2\tSpan\t*\t12\t+\t60\n" "c7\t10\t50\th1\t3\tSpan\tab\t13\t-\t60\n"
     "c7\t10\t50\th1\t4\tSpan\t*\t14\t+\t60\n" "c7\t10\t50\th1\t5\tSpan\ttail\t15\t+\t60\n"),
    ("ties keep file order; a negative pos (-1) prints 0",
     [(K, 4, 0, "first", -1, 0, 60), (S, 4, 0, "second", 8, 0, 60), (K, 4, 0, "third", 9, 0, 60), (S, 4, 0, "fourth", 10, 0, 60)], True,
     "c7\t10\t50\th1\t4\tClip\tfirst\t0\t+\t60\n" "c7\t10\t50\th1\t4\tSpan\tsecond\t9\t+\t60\n" "c7\t10\t50\th2\t4\tClip\tthird\t10\t+\t60\n"
     "c7\t10\t50\th2\t4\tSpan\tfourth\t11\t+\t60\n"),
]


@pytest.mark.parametrize("name,reads,unphased,want", ROW_CASES, ids=[c[0] for c in ROW_CASES])
def test_format_read_table_rows(name, reads, unphased, want):
    assert table_lines("c7", 10, 50, reads, unphased) == want, "the restatement against the hand-written lines"
    assert library_rows("c7", 10, 50, reads, unphased) == (len(want), want)
    # the length is the whole text's, also when the buffer is too small for it (snprintf)
    n, text = library_rows("c7", 10, 50, reads, unphased, cap=9)
    assert n == len(want) and text == want[:8]


def test_header_line():
    assert TABLE_HEADER.split("\t") == ["chrom", "begin", "end", "group", "call", "kind", "read", "pos", "strand", "mapq"]


# ---- the record ------------------------------------------------------------------------------------------------------------------------
def test_origin_layout_in_header_and_bindings(tmp_path):
    src = tmp_path / "layout.c"
    lines = "".join(f'    printf("{n} %zu %zu\\n", offsetof(inq_read_origin_t, {n}), sizeof(((inq_read_origin_t *)0)->{n}));\n' for n, _, _ in FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "inquistr_host.h"\nint main(void) {\n'
                   '    printf("size %zu %d %zu %zu\\n", sizeof(inq_read_origin_t), INQ_ABI_VERSION, sizeof(inq_span_t), sizeof(inq_call_args_t));\n'
                   + lines + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[0] == f"size 8 5 {C.sizeof(hipcall.SpanC)} {C.sizeof(call.CallArgsC)}"
    assert out[1 : 1 + len(FIELDS)] == [f"{n} {o} {s}" for n, o, s in FIELDS]
    assert C.sizeof(hipcall.ReadOriginC) == 8 == hipcall.ORIGIN_DTYPE.itemsize
    for n, o, s in FIELDS:
        f = getattr(hipcall.ReadOriginC, n)
        assert (f.offset, f.size) == (o, s), n
        assert hipcall.ORIGIN_DTYPE.fields[n][1] == o and hipcall.ORIGIN_DTYPE.fields[n][0].itemsize == s, n
    assert hipcall.ORIGIN_DTYPE.fields["pos"][0].kind == "i" and hipcall.ORIGIN_DTYPE.fields["name_len"][0].kind == "u"
    # the arguments of a call did not grow: the file has an entry of its own, the widest of its family
    assert call.CallArgsC._fields_[-1][0] == "evidence_path"
    L = call.load()
    assert hasattr(L, "inq_genotype_repeats_table") and hasattr(L, "inq_frontend_read_names") and hasattr(L, "inq_host_format_read_table_rows")


# ---- the host sweep's names ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,unphased,threads,words", [(61, False, 1, 0), (62, True, 1, 1500), (63, False, 3, 600)])
def test_host_sweep_keeps_the_names_of_its_batches(tmp_path, seed, unphased, threads, words):
    """For every locus of every batch the reads behind its pairs are the records fetch() yields, in file order: same name, same pos,
    same strand and MAPQ - also in batches cut by the word limit, whose reads are re-packed, and from the worker pool."""
    from tests.test_host_frontend import REFS, _make_case

    bam, bed, loci, recs = _make_case(tmp_path, seed, n_loci=30)
    k = 0
    for t in range(len(REFS)):  # _make_case names its records read0, read1, ... in file order
        for r in recs[t]:
            r.tags["name"] = f"read{k}".encode()
            k += 1
    fe = call.FrontEnd(bam, region_file=bed, threads=threads, unphased=unphased, max_batch_words=words)
    with pytest.raises(call.CallError):
        fe.read_names()  # no batch is out yet
    seen, n_batches = set(), 0
    for batch, idx in fe.batches():
        names = fe.read_names()
        assert len(names) == batch.n_reads
        n_batches += 1
        for j, target in enumerate(idx):
            _chrom, s, e, t = loci[int(target)]
            want = py._fetch(recs[t], t, s - 10, e + 10)
            got = batch.pair_read[int(batch.locus_pair_off[j]) : int(batch.locus_pair_off[j + 1])]
            assert [names[int(r)] for r in got] == [r.tags["name"] for r in want], (target, "names")
            assert [int(batch.reads["pos"][int(r)]) for r in got] == [r.pos for r in want]
            assert [int(batch.reads["mapq"][int(r)]) for r in got] == [r.mapq for r in want]
            assert [bool(batch.reads["bits"][int(r)] & 0x02) for r in got] == [bool(r.flag & REV) for r in want]
            seen.add(int(target))
    assert seen == set(range(len(loci))) and (not words or n_batches > 3)
    fe.close()


# ---- the command line and the entry ----------------------------------------------------------------------------------------------------
def _env():
    e = dict(os.environ)
    e.pop("INQ_SERVER", None)
    return e


def test_cli_read_table_flag(tmp_path):
    bam, bed, _loci, _recs, _ties = make_tie_case(tmp_path)
    table = tmp_path / "t.tsv"
    env = _env()
    env["INQ_SERVER"] = str(tmp_path / "no.sock")  # refused before any server is looked for: the socket does not exist
    r = subprocess.run([call.CLI_PATH, "call", bam, "-R", bed, "--read-table", str(table)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 2, r.stderr
    assert r.stdout == "" and "--read-table" in r.stderr and "INQ_SERVER" in r.stderr
    assert not table.exists()
    r = subprocess.run([call.CLI_PATH, "call", bam, "-R", bed, "--read-table"], capture_output=True, text=True, env=_env(), timeout=120)
    assert r.returncode == 2 and "--read-table" in r.stderr
    r = subprocess.run([call.CLI_PATH, "call", "--help"], capture_output=True, text=True, env=_env(), timeout=120)
    assert r.returncode == 0 and "--read-table <FILE>" in r.stdout
    r = subprocess.run([call.CLI_PATH, "cohort", "-R", bed, "--read-table", str(table), "--out-dir", str(tmp_path), bam], capture_output=True,
                       text=True, env=_env(), timeout=120)
    assert r.returncode == 2 and "--read-table" in r.stderr and not table.exists()


def test_unwritable_read_table_path(tmp_path):
    bam, bed, _loci, _recs, _ties = make_tie_case(tmp_path)
    bad = str(tmp_path / "missing" / "t.tsv")
    for extra in ([], ["--devices", "0,0"]):
        r = subprocess.run([call.CLI_PATH, "call", bam, "-R", bed, "-u", "--read-table", bad] + extra, capture_output=True, text=True, env=_env(),
                           timeout=120)
        assert r.returncode == 1, r.stderr
        assert r.stdout == "" and bad in r.stderr and "read table" in r.stderr
    out = tmp_path / "o.inq"
    for devices in (None, [0, 0]):
        ev, rcf, tf = tmp_path / f"e{devices}.tsv", tmp_path / f"r{devices}.tsv", tmp_path / f"t{devices}.bed"
        with open(out, "w") as f, pytest.raises(call.CallError) as e:
            call.genotype_repeats(bam, None, bed, 5, 3, 1, True, None, None, out=f, ties=str(tf), evidence=str(ev), read_calls=str(rcf),
                                  read_table=bad, devices=devices)
        assert e.value.status == 1 and bad in e.value.message and "read table" in e.value.message
        assert out.read_text() == ""
        assert ev.exists() and rcf.exists() and tf.exists()  # the other report files are opened first, beside it


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
    a, b, table = tmp_path / "a.inq", tmp_path / "b.inq", tmp_path / "t.tsv"
    with open(a, "w") as f:
        plain = _outcome(lambda: call.genotype_repeats(bam, None, bed, 5, 3, 1, True, None, None, out=f))
    with open(b, "w") as f:
        new = _outcome(lambda: call.genotype_repeats(bam, None, bed, 5, 3, 1, True, None, None, out=f, read_table=str(table)))
    assert new == plain
    assert a.read_text() == b.read_text()
    if plain is not None:
        assert plain[0] != 0 and plain[1] and b.read_text() == ""
    assert table.exists()  # opened before any device work
