"""The bases behind each Call (`inquistr call --read-seqs FILE`, inq_genotype_repeats_seqs) without a GPU: the host library's
sequential window walk against the Q(x) formula, what a slice is made of against the Call, the file's lines against hand-written text,
inq_read_seq_t's layout, the SEQ the host sweep keeps, the command line, a path that cannot be written, and the failure without a GPU."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from inquistr_amd import call, hipcall
from oracle import pyoracle as py
from tests import gen
from tests import read_seq_case as rs
from tests.read_seq_case import make_seq_case
from tests.test_read_calls_host import records
from tests.test_read_table_host import hipcall_bits
from tests.test_tie_report import make_tie_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, K = "Span", "Clip"


def host_window(words, pos, l_seq, start, end):
    L = call.load()
    w = np.ascontiguousarray(words, dtype=np.uint32)
    q, n = C.c_uint32(0xFFFFFFFF), C.c_uint32(0xFFFFFFFF)
    assert L.inq_host_seq_window(w.ctypes.data if len(w) else None, len(w), pos, l_seq, start, end, C.byref(q), C.byref(n)) == 0
    return q.value, n.value


# ---- the walk against the formula ------------------------------------------------------------------------------------------------------
SE, EE = 990, 1060  # of the locus (1000, 1050)
EDGE = [
    ("no op at all", [], 995, 50),
    ("one M over the whole window", [("M", 500)], 800, 500),
    ("the window edge mid-M on both sides", [("M", 100), ("I", 3), ("M", 100)], 950, 203),
    ("an op boundary exactly on se and on ee - 1", [("M", 10), ("M", 69), ("M", 10)], SE - 10, 89),
    ("I at r_op = se - 1", [("M", 9), ("I", 5), ("M", 200)], SE - 10, 214),
    ("I at r_op = se", [("M", 10), ("I", 5), ("M", 200)], SE - 10, 215),
    ("I at r_op = ee - 2", [("M", 78), ("I", 5), ("M", 200)], SE - 10, 283),
    ("I at r_op = ee - 1", [("M", 79), ("I", 5), ("M", 200)], SE - 10, 284),
    ("S at r_op = se, then one at ee - 2", [("M", 10), ("S", 7), ("M", 68), ("S", 9), ("M", 30)], SE - 10, 124),
    ("a D spanning se", [("M", 5), ("D", 20), ("M", 200)], SE - 10, 205),
    ("an N spanning se", [("M", 5), ("N", 20), ("M", 200)], SE - 10, 205),
    ("a D spanning ee - 1", [("M", 75), ("D", 20), ("M", 200)], SE - 10, 275),
    ("an N spanning ee - 1", [("M", 75), ("N", 20), ("M", 200)], SE - 10, 275),
    ("a D over the whole window: an empty slice", [("M", 5), ("D", 300), ("M", 20)], SE - 10, 25),
    ("leading S, the read starts inside the window", [("S", 40), ("M", 200)], 1010, 240),
    ("leading S, the read starts on se", [("S", 40), ("M", 200)], SE, 240),
    ("leading S, the read starts at se - 1", [("S", 40), ("M", 200)], SE - 1, 240),
    ("leading S, the read starts on ee - 2 and on ee - 1", [("S", 40), ("M", 200)], EE - 2, 240),
    ("leading S at ee - 1: behind the window", [("S", 40), ("M", 200)], EE - 1, 240),
    ("trailing S, the read ends inside the window", [("M", 100), ("S", 33)], 950, 133),
    ("trailing S, the read ends on se", [("M", 40), ("S", 33)], SE - 40, 73),
    ("trailing S, the read ends on ee - 1", [("M", 100), ("S", 33)], EE - 1 - 100, 133),
    ("H, P and op code 9 move nothing", [("H", 30), ("M", 50), ("P", 4), (9, 17), ("I", 2), ("M", 50), (15, 3), ("H", 9)], 960, 102),
    ("= and X count as M", [("=", 30), ("X", 5), ("=", 100)], 970, 135),
    ("pos = -1", [("M", 2000)], -1, 2000),
    ("l_seq 0: SEQ `*`", [("M", 300)], 900, 0),
    ("l_seq shorter than the CIGAR's query length, cut inside the slice", [("M", 300)], 900, 120),
    ("l_seq shorter than q_beg", [("M", 300)], 900, 50),
    ("the read ends in front of the window", [("M", 50)], 100, 50),
    ("the read starts behind it", [("M", 50)], 2000, 50),
]


@pytest.mark.parametrize("name,cigar,pos,l_seq", EDGE, ids=[e[0] for e in EDGE])
def test_edge_list_against_the_formula(name, cigar, pos, l_seq):
    w = rs.words_of(cigar)
    want = rs.window(w, pos, l_seq, 1000, 1050)
    assert host_window(w, pos, l_seq, 1000, 1050) == want
    assert want[0] + want[1] <= l_seq


def test_known_answers():
    """a few of the edge list by hand: the formula itself is held to something"""
    hw = lambda cigar, pos, l_seq: rs.window(rs.words_of(cigar), pos, l_seq, 1000, 1050)
    assert hw([("M", 500)], 800, 500) == (190, 69)  # bases at reference [990, 1059)
    assert hw([("M", 9), ("I", 5), ("M", 200)], SE - 10, 214) == (15, 69)  # the I at se - 1 lies in front of the slice
    assert hw([("M", 10), ("I", 5), ("M", 200)], SE - 10, 215) == (10, 74)  # ... the one at se inside it
    assert hw([("M", 78), ("I", 5), ("M", 200)], SE - 10, 283) == (10, 74)  # at ee - 2: 68 matched + 5 + 1
    assert hw([("M", 79), ("I", 5), ("M", 200)], SE - 10, 284) == (10, 69)  # at ee - 1: behind it
    assert hw([("S", 40), ("M", 200)], 1010, 240) == (0, 89)  # q_beg 0, the clip included: 40 + [1010, 1059)
    assert hw([("M", 100), ("S", 33)], 950, 133) == (40, 93)  # runs to l_seq
    assert hw([("M", 5), ("D", 300), ("M", 20)], SE - 10, 25) == (5, 0)
    assert hw([("M", 300)], 900, 120) == (90, 30) and hw([("M", 300)], 900, 50) == (50, 0) and hw([("M", 300)], 900, 0) == (0, 0)
    assert hw([("M", 2000)], -1, 2000) == (991, 69)


@pytest.mark.parametrize("start,end", [(9, 50), (0, 5), (5, 4294967290), (100, 4294967290), (1000, 1000), (4294967280, 4294967290)])
def test_windows_without_width(start, end):
    """start < 10 takes start_ext below 0, end + 10 past 2^32 wraps: (0, 0); a locus of length 0 still has its 20 bases of flank"""
    w = rs.words_of([("M", 4000)])
    got = host_window(w, 0, 4000, start, end)
    assert got == rs.window(w, 0, 4000, start, end)
    assert (got == (0, 0)) == ((start, end) != (1000, 1000))


@pytest.mark.parametrize("seed", range(6))
def test_random_cigars_and_what_a_slice_is_made_of(seed):
    """n_bases == matched bases in the window + inserted + clipped bases in the window; for a read that is no accidental 2D and
    minlen 0 the Call is the same I and S ops less the D ops"""
    rng = random.Random(900 + seed)
    n_checked = 0
    for _ in range(150):
        start = rng.randint(2000, 3000)
        end = start + rng.choice([0, 1, 30, 250])
        rec = gen.random_locus_reads(rng, start, end, 1, long_every=rng.choice([0, 0, 1]))[0]
        w = rs.words_of(rec.cigar)
        qlen = sum(n for o, n in rec.cigar if o in "MIS=X")
        q_beg, n_bases = host_window(w, rec.pos, qlen, start, end)
        assert (q_beg, n_bases) == rs.window(w, rec.pos, qlen, start, end)
        matched, ins, dele = rs.window_sums(w, rec.pos, start, end)
        assert n_bases == matched + ins
        short = max(0, qlen - 7)
        assert host_window(w, rec.pos, short, start, end) == rs.window(w, rec.pos, short, start, end)
        if not py.is_accidental_2d(rec):
            kind, value = py.call_from_cigar(rec, 0, start - 10, end + 10)
            assert value == ins - dele, rec.cigar
            n_checked += 1
    assert n_checked > 50


# ---- the lines of one target -----------------------------------------------------------------------------------------------------------
def library_rows(chrom, start, end, reads, unphased, cap=1 << 16):
    """reads: (kind, value, HP, name, q_beg, codes) in file order"""
    L = call.load()
    rec = records([r[:3] for r in reads])
    org = np.zeros(len(reads), dtype=hipcall.ORIGIN_DTYPE)
    sq = np.zeros(len(reads), dtype=hipcall.SEQ_DTYPE)
    raw, packed = b"", b""
    for i, (_k, _v, _g, name, q_beg, codes) in enumerate(reads):
        nb = name.encode("latin1")
        org[i] = (5, 60, hipcall_bits(0), len(nb))
        sq[i] = (q_beg, len(codes))
        raw += nb
        packed += rs.pack(codes)
    names = np.frombuffer(raw + b"\xff", dtype=np.uint8)
    pk = np.frombuffer(packed + b"\xff", dtype=np.uint8)  # (a byte behind the last slice that must not be read into a line)
    buf = C.create_string_buffer(cap)
    n = L.inq_host_format_read_seq_rows(chrom.encode(), start, end, rec.ctypes.data if len(rec) else None, org.ctypes.data if len(org) else None,
                                        names.ctypes.data, sq.ctypes.data if len(sq) else None, pk.ctypes.data, len(rec), 1 if unphased else 0,
                                        buf, cap)
    return n, buf.value.decode("latin1")


ALL16 = list(range(16))
ROW_CASES = [
    ("no kept read", [], False, ""),
    ("an empty slice is `*`; all 16 codes; odd and even lengths",
     [(S, 0, 1, "e", 7, []), (K, 36, 1, "all", 0, ALL16), (S, -3, 2, "odd", 4294967295, [1, 2, 4]), (S, 2, 2, "even", 12, [8, 15]),
      (S, 9, 0, "one", 3, [4])], False,
     "c7\t10\t50\th1\t0\tSpan\te\t7\t0\t*\n" "c7\t10\t50\th1\t36\tClip\tall\t0\t16\t=ACMGRSVTWYHKDBN\n"
     "c7\t10\t50\th2\t-3\tSpan\todd\t4294967295\t3\tACG\n" "c7\t10\t50\th2\t2\tSpan\teven\t12\t2\tTN\n" "c7\t10\t50\tother\t9\tSpan\tone\t3\t1\tG\n"),
    ("unphased: sorted by value, the slices travel with their reads",
     [(S, 9, 0, "c", 1, [1, 1, 1]), (S, 1, 0, "a", 2, [2]), (K, 5, 0, "b", 3, [4, 4])], True,
     "c7\t10\t50\th1\t1\tSpan\ta\t2\t1\tC\n" "c7\t10\t50\th2\t5\tClip\tb\t3\t2\tGG\n" "c7\t10\t50\th2\t9\tSpan\tc\t1\t3\tAAA\n"),
]


@pytest.mark.parametrize("name,reads,unphased,want", ROW_CASES, ids=[c[0] for c in ROW_CASES])
def test_format_read_seq_rows(name, reads, unphased, want):
    assert rs.seq_lines("c7", 10, 50, reads, unphased) == want, "the restatement against the hand-written lines"
    assert library_rows("c7", 10, 50, reads, unphased) == (len(want), want)
    n, text = library_rows("c7", 10, 50, reads, unphased, cap=9)
    assert n == len(want) and text == want[:8]


def test_header_line_and_unpack():
    assert rs.SEQS_HEADER.split("\t") == ["chrom", "begin", "end", "group", "call", "kind", "read", "qbeg", "len", "seq"]
    assert hipcall.unpack_seq(np.frombuffer(rs.pack(ALL16 + [3]), dtype=np.uint8), 17) == "=ACMGRSVTWYHKDBNM"
    assert rs.pack([1, 2, 4]) == b"\x12\x40"


# ---- the record and the symbols --------------------------------------------------------------------------------------------------------
def test_seq_record_layout_and_symbols(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "inquistr_host.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %d\\n", sizeof(inq_read_seq_t), offsetof(inq_read_seq_t, q_beg), offsetof(inq_read_seq_t, n_bases), '
                   "INQ_ABI_VERSION);\n    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout == "8 0 4 5\n"
    assert C.sizeof(hipcall.ReadSeqC) == 8 == hipcall.SEQ_DTYPE.itemsize
    assert hipcall.SEQ_DTYPE.fields["q_beg"][1] == 0 and hipcall.SEQ_DTYPE.fields["n_bases"][1] == 4
    assert call.CallArgsC._fields_[-1][0] == "evidence_path"  # the arguments of a call did not grow
    L = call.load()
    for sym in ("inq_genotype_repeats_seqs", "inq_frontend_read_seqs", "inq_host_format_read_seq_rows", "inq_host_seq_window"):
        assert hasattr(L, sym) and sym in call.HOST_ABI_SYMBOLS, sym
    D = hipcall.load()
    for sym in ("inq_call_span_deferred_seqs", "inq_call_flush_seqs", "inq_read_seqs_fetch", "inq_span_fetch_seqs", "inq_seq_windows",
                "inq_seq_window_tile"):
        assert hasattr(D, sym) and sym in hipcall.ABI_SYMBOLS, sym
    assert D.inq_seq_window_tile() == 16
    # every entry that takes a context refuses none: no device is touched, nothing is written
    assert D.inq_seq_windows(None, None, None, None, None) == -1 and D.inq_read_seqs_fetch(None, None, 0, None, 0) == -1
    assert D.inq_call_flush_seqs(None, None, 0, None, None, None, None, None, None) == -1
    assert D.inq_span_fetch_seqs(None, None, None, None, None, 0) == -1 and D.inq_call_span_deferred_seqs(None, None, -1, None) == -1


# ---- the host sweep's SEQ --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,unphased,threads,words", [(71, False, 1, 0), (72, True, 1, 1500), (73, False, 3, 600)])
def test_host_sweep_keeps_the_seq_of_its_batches(tmp_path, seed, unphased, threads, words):
    bam, bed, loci, recs = make_seq_case(tmp_path, seed)
    fe = call.FrontEnd(bam, region_file=bed, threads=threads, unphased=unphased, max_batch_words=words, keep_seqs=True)
    with pytest.raises(call.CallError):
        fe.read_seqs()  # no batch is out yet
    seen = set()
    for batch, idx in fe.batches():
        l_seq, off, raw = fe.read_seqs()
        assert len(l_seq) == batch.n_reads and np.array_equal(np.diff(off.astype(np.int64)), (l_seq.astype(np.int64) + 1) // 2)
        for j, target in enumerate(idx):
            _chrom, s, e, t = loci[int(target)]
            want = py._fetch(recs[t], t, s - 10, e + 10)
            got = batch.pair_read[int(batch.locus_pair_off[j]) : int(batch.locus_pair_off[j + 1])]
            assert [int(l_seq[int(r)]) for r in got] == [len(r.tags["seq"]) for r in want]
            assert [raw[int(off[int(r)]) : int(off[int(r) + 1])].tobytes() for r in got] == [rs.pack(r.tags["seq"]) for r in want], target
            seen.add(int(target))
    assert seen == set(range(len(loci)))
    fe.close()
    # a handle that is not asked keeps none
    fe = call.FrontEnd(bam, region_file=bed, threads=threads, unphased=unphased)
    for _batch, _idx in fe.batches():
        with pytest.raises(call.CallError):
            fe.read_seqs()
        break
    fe.close()


# ---- the command line and the entry ----------------------------------------------------------------------------------------------------
def _env():
    e = dict(os.environ)
    e.pop("INQ_SERVER", None)
    return e


def test_cli_read_seqs_flag(tmp_path):
    bam, bed, _loci, _recs, _ties = make_tie_case(tmp_path)
    out = tmp_path / "s.tsv"
    env = _env()
    env["INQ_SERVER"] = str(tmp_path / "no.sock")  # refused before any server is looked for: the socket does not exist
    r = subprocess.run([call.CLI_PATH, "call", bam, "-R", bed, "--read-seqs", str(out)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 2, r.stderr
    assert r.stdout == "" and "--read-seqs" in r.stderr and "INQ_SERVER" in r.stderr
    assert not out.exists()
    r = subprocess.run([call.CLI_PATH, "call", bam, "-R", bed, "--read-seqs"], capture_output=True, text=True, env=_env(), timeout=120)
    assert r.returncode == 2 and "--read-seqs" in r.stderr
    r = subprocess.run([call.CLI_PATH, "call", "--help"], capture_output=True, text=True, env=_env(), timeout=120)
    assert r.returncode == 0 and "--read-seqs <FILE>" in r.stdout
    r = subprocess.run([call.CLI_PATH, "cohort", "-R", bed, "--read-seqs", str(out), "--out-dir", str(tmp_path), bam], capture_output=True,
                       text=True, env=_env(), timeout=120)
    assert r.returncode == 2 and "--read-seqs" in r.stderr and not out.exists()


def test_unwritable_read_seqs_path(tmp_path):
    bam, bed, _loci, _recs, _ties = make_tie_case(tmp_path)
    bad = str(tmp_path / "missing" / "s.tsv")
    for extra in ([], ["--devices", "0,0"]):
        r = subprocess.run([call.CLI_PATH, "call", bam, "-R", bed, "-u", "--read-seqs", bad] + extra, capture_output=True, text=True, env=_env(),
                           timeout=120)
        assert r.returncode == 1, r.stderr
        assert r.stdout == "" and bad in r.stderr and "read-seqs file" in r.stderr
    out, table = tmp_path / "o.inq", tmp_path / "t.tsv"
    with open(out, "w") as f, pytest.raises(call.CallError) as e:
        call.genotype_repeats(bam, None, bed, 5, 3, 1, True, None, None, out=f, read_table=str(table), read_seqs=bad)
    assert e.value.status == 1 and bad in e.value.message and "read-seqs file" in e.value.message
    assert out.read_text() == "" and table.exists()  # the other report files are opened first, beside it


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
    a, b, seqs = tmp_path / "a.inq", tmp_path / "b.inq", tmp_path / "s.tsv"
    with open(a, "w") as f:
        plain = _outcome(lambda: call.genotype_repeats(bam, None, bed, 5, 3, 1, True, None, None, out=f))
    with open(b, "w") as f:
        new = _outcome(lambda: call.genotype_repeats(bam, None, bed, 5, 3, 1, True, None, None, out=f, read_seqs=str(seqs)))
    assert new == plain
    assert a.read_text() == b.read_text()
    if plain is not None:
        assert plain[0] != 0 and plain[1] and b.read_text() == ""
    assert seqs.exists()  # opened before any device work
