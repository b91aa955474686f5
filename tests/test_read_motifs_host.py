"""The motif runs of the bases behind each Call (`inquistr call --read-motifs FILE`, inq_genotype_repeats_motifs) without a GPU: the
contract's known answers through the numpy restatement and through the host library's sequential walk, the two against each other on
random slices, the motif encoder, column 4 of the BED, the file's lines against hand-written text, inq_read_motif_t's layout, the new
symbols, and the command line."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from inquistr_amd import call, hipcall
from tests import read_motif_case as rm
from tests import read_seq_case as rs
from tests.test_host_frontend import GOLDEN, _make_case
from tests.test_read_calls_host import records
from tests.test_read_table_host import hipcall_bits
from tests.test_tie_report import make_tie_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, K = "Span", "Clip"


def host_runs(codes, word):
    """inq_host_motif_runs over the packed codes, with a byte behind them that must not count"""
    L = call.load()
    packed = np.frombuffer(rs.pack(codes) + b"\x24", dtype=np.uint8)
    out = np.full(1, 0xFFFFFFFF, dtype=hipcall.MOTIF_DTYPE)
    assert L.inq_host_motif_runs(packed.ctypes.data, len(codes), word, out.ctypes.data) == 0
    return tuple(int(x) for x in out[0])


def host_encode(text):
    L = call.load()
    w = C.c_uint64(0xFFFFFFFFFFFFFFFF)
    rc = L.inq_host_motif_encode(None if text is None else text.encode(), C.byref(w))
    return rc, w.value


# ---- the three forms -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text,motif,beg,length,bases,runs", rm.KNOWN, ids=[f"{k[0] or 'empty'}-{k[1]}" for k in rm.KNOWN])
def test_known_answers(text, motif, beg, length, bases, runs):
    word = hipcall.encode_motif(motif)
    assert host_encode(motif) == (0, word)
    assert rm.motif_runs(rm.codes_of(text), word) == (beg, length, bases, runs), "the restatement"
    assert host_runs(rm.codes_of(text), word) == (beg, length, bases, runs), "the host walk"


def test_a_literal_word_counts_each_equivalent_rotation():
    """the device and the walk take a word literally: CAGCAG has every run of CAG at two rotations"""
    word = rm.literal_word("CAGCAG")
    codes = rm.codes_of("CAGCAGCAGCAGTTCAGCAGCAG")
    assert rm.motif_runs(codes, word) == (0, 12, 21, 4) == host_runs(codes, word)
    assert rm.motif_runs(codes, hipcall.encode_motif("CAGCAG")) == (0, 12, 21, 2)
    for bad in (0, 3 << 60 | 0x321, 3 << 60 | 0x021, 2 << 60 | 0xF1):  # k = 0; a code that is none of A C G T; 0; N
        assert rm.motif_runs(codes, bad) == (0, 0, 0, 0) == host_runs(codes, bad)
    # nibbles between k and 15 are not read
    assert host_runs(codes, hipcall.encode_motif("CAG") | 0xABC << 12) == rm.motif_runs(codes, hipcall.encode_motif("CAG"))


MOTIFS = ["A", "CA", "CAG", "AAG", "GGCCCC", "CCCCGCCCCGCG", "ACGTACGTACGTAAA", "AAAAAAAAAAAAAAC"] + [
    "".join("ACGT"[(i * i + k) % 4] for i in range(k)) for k in range(1, 16)]


@pytest.mark.parametrize("p_hit", [0.0, 0.5, 0.9, 1.0])
def test_walk_against_restatement_on_random_slices(p_hit):
    rng = random.Random(int(p_hit * 100) + 7)
    lengths = sorted(set([0, 1, 2, 3, 299, 300] + [16 * q + d for q in range(1, 19) for d in (-1, 0, 1)]))
    n = 0
    for motif in MOTIFS:
        word = rm.literal_word(motif)
        assert 1 <= len(motif) <= 15
        for length in rng.sample(lengths, 14) + [0, 300]:
            phase = rng.randrange(len(motif))
            codes = rm.repeat_codes(motif, length, phase)
            for i in range(length):
                if rng.random() >= p_hit:
                    codes[i] = rng.randrange(16)  # any code, those outside ACGT among them
            want = rm.motif_runs(codes, word)
            assert host_runs(codes, word) == want, (motif, length, phase)
            if p_hit == 1.0 and length:
                assert want[:2] == (0, length) and want[2] == (length if length >= len(motif) else 0)
            n += 1
    assert n == len(MOTIFS) * 16


# ---- the encoder -----------------------------------------------------------------------------------------------------------------------
def test_encoder():
    cag = 3 << 60 | 4 << 8 | 1 << 4 | 2  # k in nibble 15; C A G in nibbles 0 1 2
    assert host_encode("CAG") == (0, cag) and hipcall.encode_motif("CAG") == cag
    assert host_encode("cAg") == (0, cag) and hipcall.encode_motif("cag") == cag
    assert host_encode("CAGCAG") == (0, cag) and host_encode("CAG" * 6) == (0, cag), "reduced to the primitive root"
    assert host_encode("T") == (0, 1 << 60 | 8) and host_encode("TTTTTTTTTTTTTTTTTTTT") == (0, 1 << 60 | 8)
    m15, m16 = "ACGTACGTACGTAAA", "ACGTACGTACGTAAAC"
    rc, w = host_encode(m15)
    assert rc == 0 and w >> 60 == 15 and w == hipcall.encode_motif(m15) == rm.literal_word(m15)
    assert host_encode(m15 * 2) == (0, w)
    codes = {(".", 2), ("", 1), (None, 1), ("GCN", 2), ("CAG,CCG", 2), ("CA G", 2), (m16, 3), (m16 * 2, 3)}
    for text, rc_want in codes:
        assert host_encode(text) == (rc_want, 0), text
        if text is not None:
            assert hipcall.encode_motif(text) == 0, text
    assert len({rc for _t, rc in codes}) == 3, "each refusal has its own value"
    for motif in MOTIFS:
        assert host_encode(motif)[1] == hipcall.encode_motif(motif)


# ---- column 4 of the BED ---------------------------------------------------------------------------------------------------------------
def test_bed_column_four(tmp_path):
    bam, _, _, _ = _make_case(tmp_path, 6, n_loci=3)

    def read(text):
        p = str(tmp_path / "t.bed")
        open(p, "w").write(text)
        fe = call.FrontEnd(bam, region_file=p)
        got = fe.targets(), fe.target_names()
        fe.close()
        return got

    two = [("chr1", 100, 200), ("chr2", 300, 400)]
    assert read("chr1\t100\t200\n#c\n\nchr2\t300\t400\r\n") == (two, [None, None])
    assert read("chr1\t100\t200\tCAG\nchr2\t300\t400\t.\n") == (two, ["CAG", "."])
    assert read("chr1\t100\t200\tname\t0\t+\nchr2\t300\t400\tn2\t1\t-\n") == (two, ["name", "n2"])
    assert read('chr1\t100\t200\t"CAG"\nchr2\t300\t400\t"C""A\tG"\n') == (two, ["CAG", 'C"A\tG'])
    fe = call.FrontEnd(bam, region="chr1:100-200")
    assert fe.targets() == [("chr1", 100, 200)] and fe.target_names() == [None]
    fe.close()
    with pytest.raises(call.CallError) as e:  # records of unequal length stay refused
        read("chr1\t100\t200\nchr2\t300\t400\tCAG\n")
    assert e.value.status == 101


def test_reference_bed_parses_as_before(tmp_path):
    from tools import bamio

    bam = str(tmp_path / "plumbing.bam")
    w = bamio.BamWriter(bam, [("chr7", 159345973)])
    w.add("r", 0, 0, 154778000, 60, [("M", 2000)], [("HP", "C", 1)])
    w.close()
    fe = call.FrontEnd(bam, region_file=os.path.join(GOLDEN, "reference_test.bed"))
    assert fe.targets() == [("chr7", 154778571, 154779363)]
    n_cols = len(open(os.path.join(GOLDEN, "reference_test.bed")).readline().rstrip("\n").split("\t"))
    assert fe.target_names() == ([None] if n_cols < 4 else [open(os.path.join(GOLDEN, "reference_test.bed")).readline().rstrip("\n").split("\t")[3]])
    fe.close()


# ---- the lines of one target -----------------------------------------------------------------------------------------------------------
def library_rows(chrom, start, end, reads, unphased, word, cap=1 << 16):
    """reads: (kind, value, HP, name, q_beg, codes) in file order; the records are the restatement's"""
    L = call.load()
    rec = records([r[:3] for r in reads])
    org = np.zeros(len(reads), dtype=hipcall.ORIGIN_DTYPE)
    sq = np.zeros(len(reads), dtype=hipcall.SEQ_DTYPE)
    mt = rm.records_of([r[5] for r in reads], [word] * len(reads))
    raw = b""
    for i, (_k, _v, _g, name, q_beg, codes) in enumerate(reads):
        nb = name.encode("latin1")
        org[i] = (5, 60, hipcall_bits(0), len(nb))
        sq[i] = (q_beg, len(codes))
        raw += nb
    names = np.frombuffer(raw + b"\xff", dtype=np.uint8)
    buf = C.create_string_buffer(cap)
    n = L.inq_host_format_read_motif_rows(chrom.encode(), start, end, rec.ctypes.data if len(rec) else None, org.ctypes.data if len(org) else None,
                                          names.ctypes.data, sq.ctypes.data if len(sq) else None, mt.ctypes.data if len(mt) else None, word,
                                          len(rec), 1 if unphased else 0, buf, cap)
    return n, buf.value.decode("latin1")


c = rm.codes_of
ROW_CASES = [
    ("no kept read", [], False, "CAG", ""),
    ("units are whole motif copies; an empty slice; an interruption",
     [(S, 0, 1, "e", 7, []), (K, 36, 1, "pure", 0, c("AGCAGCAGCAGCA")), (S, -3, 2, "cut", 4294967295, c("TTCAGCAGCAACAGCAGTT")),
      (S, 9, 0, "short", 3, c("CA"))], False, "CAGCAG",
     "c7\t10\t50\th1\t0\tSpan\te\t7\t0\tCAG\t0\t0\t0\t0\t0\n" "c7\t10\t50\th1\t36\tClip\tpure\t0\t13\tCAG\t0\t13\t4\t13\t1\n"
     "c7\t10\t50\th2\t-3\tSpan\tcut\t4294967295\t19\tCAG\t2\t8\t2\t14\t2\n" "c7\t10\t50\tother\t9\tSpan\tshort\t3\t2\tCAG\t0\t2\t0\t0\t0\n"),
    ("a target whose motif does not encode: `.` in the motif field and the five behind it",
     [(S, 1, 1, "a", 2, c("CAGCAG")), (K, 5, 2, "b", 0, [])], False, "GCN",
     "c7\t10\t50\th1\t1\tSpan\ta\t2\t6\t.\t.\t.\t.\t.\t.\n" "c7\t10\t50\th2\t5\tClip\tb\t0\t0\t.\t.\t.\t.\t.\t.\n"),
    ("unphased: sorted by value, the runs travel with their reads",
     [(S, 9, 0, "c", 1, c("AAAA")), (S, 1, 0, "a", 2, c("CGA")), (K, 5, 0, "b", 3, c("NAAN"))], True, "a",
     "c7\t10\t50\th1\t1\tSpan\ta\t2\t3\tA\t2\t1\t1\t1\t1\n" "c7\t10\t50\th2\t5\tClip\tb\t3\t4\tA\t1\t2\t2\t2\t1\n"
     "c7\t10\t50\th2\t9\tSpan\tc\t1\t4\tA\t0\t4\t4\t4\t1\n"),
]


@pytest.mark.parametrize("name,reads,unphased,motif,want", ROW_CASES, ids=[r[0] for r in ROW_CASES])
def test_format_read_motif_rows(name, reads, unphased, motif, want):
    word = hipcall.encode_motif(motif)
    assert rm.motif_lines("c7", 10, 50, reads, unphased, word) == want, "the restatement against the hand-written lines"
    assert library_rows("c7", 10, 50, reads, unphased, word) == (len(want), want)
    n, text = library_rows("c7", 10, 50, reads, unphased, word, cap=9)
    assert n == len(want) and text == want[:8]


def test_header_line():
    assert rm.MOTIFS_HEADER.split("\t") == ["chrom", "begin", "end", "group", "call", "kind", "read", "qbeg", "len", "motif", "run_beg", "run_len",
                                            "units", "motif_bases", "runs"]
    assert rm.MOTIFS_HEADER.split("\t")[:9] == rs.SEQS_HEADER.split("\t")[:9]


# ---- the record and the symbols --------------------------------------------------------------------------------------------------------
def test_motif_record_layout_and_symbols(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "inquistr_host.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %zu %zu %d\\n", sizeof(inq_read_motif_t), offsetof(inq_read_motif_t, run_beg), '
                   "offsetof(inq_read_motif_t, run_len), offsetof(inq_read_motif_t, motif_bases), offsetof(inq_read_motif_t, n_runs), "
                   "INQ_ABI_VERSION);\n    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout == "16 0 4 8 12 5\n"
    assert C.sizeof(hipcall.ReadMotifC) == 16 == hipcall.MOTIF_DTYPE.itemsize
    assert [hipcall.MOTIF_DTYPE.fields[f][1] for f in ("run_beg", "run_len", "motif_bases", "n_runs")] == [0, 4, 8, 12]
    assert call.CallArgsC._fields_[-1][0] == "evidence_path"  # the arguments of a call did not grow
    L = call.load()
    for sym in ("inq_genotype_repeats_motifs", "inq_host_format_read_motif_rows", "inq_host_motif_encode", "inq_host_motif_runs",
                "inq_frontend_target_name"):
        assert hasattr(L, sym) and sym in call.HOST_ABI_SYMBOLS, sym
    D = hipcall.load()
    for sym in ("inq_call_flush_motifs", "inq_read_motifs_fetch", "inq_motif_runs", "inq_read_motif_tile"):
        assert hasattr(D, sym) and sym in hipcall.ABI_SYMBOLS, sym
    assert D.inq_read_motif_tile() == 16 and D.inq_abi_version() == 5
    assert hipcall._SIDE_SUFFIXES[-1] == "_motifs"
    # every entry that takes a context refuses none: no device is touched, nothing is written
    assert D.inq_read_motifs_fetch(None, None, 0) == -1
    assert D.inq_motif_runs(None, None, 0, None, 0, None, None, 0, None) == -1
    assert D.inq_call_flush_motifs(None, None, 0, None, None, None, None, None, None, None) == -1
    assert L.inq_host_motif_runs(None, 5, 0, None) == 1


# ---- the command line ------------------------------------------------------------------------------------------------------------------
def _env():
    e = dict(os.environ)
    e.pop("INQ_SERVER", None)
    return e


def test_cli_read_motifs_flags(tmp_path):
    bam, bed, _loci, _recs, _ties = make_tie_case(tmp_path)
    out = tmp_path / "m.tsv"
    env = _env()
    env["INQ_SERVER"] = str(tmp_path / "no.sock")  # refused before any server is looked for: the socket does not exist
    r = subprocess.run([call.CLI_PATH, "call", bam, "-R", bed, "--read-motifs", str(out), "--motif", "CAG"], capture_output=True, text=True,
                       env=env, timeout=120)
    assert r.returncode == 2, r.stderr
    assert r.stdout == "" and "--read-motifs" in r.stderr and "INQ_SERVER" in r.stderr
    assert not out.exists()
    for flag in ("--read-motifs", "--motif"):
        r = subprocess.run([call.CLI_PATH, "call", bam, "-R", bed, flag], capture_output=True, text=True, env=_env(), timeout=120)
        assert r.returncode == 2 and flag in r.stderr
    r = subprocess.run([call.CLI_PATH, "call", "--help"], capture_output=True, text=True, env=_env(), timeout=120)
    assert r.returncode == 0 and "--read-motifs <FILE>" in r.stdout and "--motif <STR>" in r.stdout
    r = subprocess.run([call.CLI_PATH, "cohort", "-R", bed, "--read-motifs", str(out), "--out-dir", str(tmp_path), bam], capture_output=True,
                       text=True, env=_env(), timeout=120)
    assert r.returncode == 2 and "--read-motifs" in r.stderr and not out.exists()


def test_no_motif_anywhere_is_an_error(tmp_path):
    """a BED of three columns (make_tie_case writes one) and no --motif: exit 1, the message names column 4, stdout stays empty"""
    bam, bed, _loci, _recs, _ties = make_tie_case(tmp_path)
    assert len(open(bed).readline().split("\t")) == 3
    out = tmp_path / "m.tsv"
    for extra in ([], ["--devices", "0,0"], ["-t", "3"]):
        r = subprocess.run([call.CLI_PATH, "call", bam, "-R", bed, "-u", "--read-motifs", str(out)] + extra, capture_output=True, text=True,
                           env=_env(), timeout=120)
        assert r.returncode == 1, r.stderr
        assert r.stdout == "" and "column 4" in r.stderr and "--motif" in r.stderr
    r = subprocess.run([call.CLI_PATH, "call", bam, "-R", bed, "-u", "--read-motifs", str(out), "--motif", "GCN"], capture_output=True, text=True,
                       env=_env(), timeout=120)
    assert r.returncode == 1 and r.stdout == "" and "GCN" in r.stderr
    o = tmp_path / "o.inq"
    with open(o, "w") as f, pytest.raises(call.CallError) as e:
        call.genotype_repeats(bam, None, bed, 5, 3, 1, True, None, None, out=f, read_motifs=str(out))
    assert e.value.status == 1 and "column 4" in e.value.message and o.read_text() == ""


def test_unwritable_read_motifs_path(tmp_path):
    bam, bed, _loci, _recs, _ties = make_tie_case(tmp_path)
    bad = str(tmp_path / "missing" / "m.tsv")
    for extra in ([], ["--devices", "0,0"]):
        r = subprocess.run([call.CLI_PATH, "call", bam, "-R", bed, "-u", "--motif", "CAG", "--read-motifs", bad] + extra, capture_output=True,
                           text=True, env=_env(), timeout=120)
        assert r.returncode == 1, r.stderr
        assert r.stdout == "" and bad in r.stderr and "read-motifs file" in r.stderr
    out, seqs = tmp_path / "o.inq", tmp_path / "s.tsv"
    with open(out, "w") as f, pytest.raises(call.CallError) as e:
        call.genotype_repeats(bam, None, bed, 5, 3, 1, True, None, None, out=f, read_seqs=str(seqs), read_motifs=bad, motif="CAG")
    assert e.value.status == 1 and bad in e.value.message and "read-motifs file" in e.value.message
    assert out.read_text() == "" and seqs.exists()  # the other report files are opened first, beside it
