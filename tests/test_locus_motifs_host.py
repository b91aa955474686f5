"""The motif each locus's reads repeat (`inquistr call --locus-motifs FILE`, `--motif auto`, inq_genotype_repeats_locus_motifs) without a
GPU: the contract's known answers through the numpy restatement and through the host library's base-by-base walk, the two against each
other on random codes and on noisy repeats, the ties, the file's line against hand-written text, inq_locus_motif_t's layout, the new
symbols, the command line, and how often the rule recovers a motif nobody typed in."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from inquistr_amd import call, hipcall
from tests import locus_motif_case as lm
from tests import read_motif_case as rm
from tests import read_seq_case as rs
from tests.test_host_frontend import GOLDEN
from tests.test_tie_report import make_tie_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_find(slices):
    """inq_host_locus_motif_find over the slices packed back to back, with a byte behind them that must not count"""
    L = call.load()
    packed = np.frombuffer(b"".join(rs.pack(c) for c in slices) + b"\x24", dtype=np.uint8)
    lens = np.array([len(c) for c in slices], dtype=np.uint32)
    out = np.full(1, 0xFFFFFFFFFFFFFFFF, dtype=hipcall.LOCUS_MOTIF_DTYPE)
    assert L.inq_host_locus_motif_find(packed.ctypes.data, lens.ctypes.data if len(lens) else None, len(lens), out.ctypes.data) == 0
    return tuple(int(x) for x in out[0])


# ---- the contract ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text,lags,p,motif,copies", lm.KNOWN, ids=[k[0] for k in lm.KNOWN])
def test_known_answers(text, lags, p, motif, copies):
    codes = rm.codes_of(text)
    if lags is not None:
        assert tuple(lm.lag_counts([codes])) == lags
    word = rm.literal_word(motif) if motif else 0
    want = (word, p, len(text), lm.lag_counts([codes])[p - 1] if p else 0, copies)
    assert lm.find([codes]) == want, "the restatement"
    assert host_find([codes]) == want, "the host walk"


def test_known_lag_of_the_interrupted_copy():
    """period and lag count stay where no copy is whole: word 0, copies 0"""
    assert lm.find([rm.codes_of("CAGNCAG")]) == (0, 4, 7, 3, 0) == host_find([rm.codes_of("CAGNCAG")])
    assert lm.find([rm.codes_of("CAGCA")]) == (0, 3, 5, 2, 0) == host_find([rm.codes_of("CAGCA")])


def test_ties_and_the_primitive_root():
    c = rm.codes_of
    # T_2 == T_4, both the largest: the smaller period
    two = [c("ACAC"), c("ACGTAC")]
    assert lm.lag_counts(two)[1] == lm.lag_counts(two)[3] == 2 == max(lm.lag_counts(two))
    assert lm.find(two)[1] == 2 == host_find(two)[1]
    # two classes with equal counts: the smaller class
    tie = [c("CACACAGAGAG")]
    assert lm.class_counts(tie, 2) == {"AC": 3, "AG": 3} and lm.find(tie)[0] == rm.literal_word("AC") == host_find(tie)[0]
    # period 4 by the lag counts of several 4-mers' repeats, the largest class among them ACAC: out comes its root AC
    root = [c("AC" * 6), c("ACGT" * 2 + "A"), c("AGGT" * 2 + "A")]
    t = lm.lag_counts(root)
    assert t[3] > t[1] and lm.class_counts(root, 4) == {"ACAC": 5, "ACGT": 2, "AGGT": 2}
    assert lm.find(root) == (rm.literal_word("AC"), 4, 30, t[3], 5) == host_find(root)
    # no record, and records without a base
    assert lm.find([]) == (0, 0, 0, 0, 0) == host_find([])
    assert lm.find([c("NNNN"), c("")]) == (0, 0, 4, 0, 0) == host_find([c("NNNN"), c("")])
    # `=` (code 0) equals itself and is no base
    assert lm.find([np.zeros(9, dtype=np.uint8)]) == (0, 0, 9, 0, 0) == host_find([np.zeros(9, dtype=np.uint8)])


@pytest.mark.parametrize("alphabet", [16, 4, 2], ids=["codes0-15", "acgt", "two-letters"])
def test_walk_against_restatement_on_random_codes(alphabet):
    rng = random.Random(2000 + alphabet)
    pick = {16: list(range(16)), 4: [1, 2, 4, 8], 2: [1, 4]}[alphabet]
    seen = set()
    for _ in range(150):
        slices = [np.array([rng.choice(pick) for _ in range(rng.choice([0, 1, 2, 5, 11, 12, 13, 17, 40]))], dtype=np.uint8)
                  for _ in range(rng.randrange(0, 5))]
        want = lm.find(slices)
        assert host_find(slices) == want, [list(map(int, s)) for s in slices]
        seen.add(want[1])
    assert len(seen) >= 3, "several periods, none among them"


@pytest.mark.parametrize("k", range(1, 7))
def test_walk_against_restatement_on_noisy_repeats(k):
    rng = random.Random(3000 + k)
    hit = 0
    for _ in range(25):
        motif = "".join(rng.choice("ACGT") for _ in range(k))
        slices = [rm.noisy_repeat(rng, motif, rng.choice([0, 7, 30, 64, 150])) for _ in range(rng.randrange(1, 6))]
        want = lm.find(slices)
        assert host_find(slices) == want
        hit += want[0] != 0
    assert hit >= 20


# ---- how often the rule finds a motif nobody typed in -----------------------------------------------------------------------------------
RECOVERY_MOTIFS = ["A", "CA", "AT", "CAG", "AAG", "CCG", "GGC", "AAAAG", "TTTTA", "GGCCCC"]


def least_rotation(m):
    return min(m[r:] + m[:r] for r in range(len(m)))


@pytest.mark.parametrize("motif", RECOVERY_MOTIFS)
@pytest.mark.parametrize("n_repeat", [60, 150])
def test_recovery_between_random_flanks(motif, n_repeat):
    """30 slices of 10 random flank bases + a noisy repeat + 10 random flank bases: the motif's smallest rotation comes out, every
    trial (measured beforehand: 200 of 200 for each motif and both lengths).  Loci with little repeat are not asserted: 12 repeat
    bases at depth 3 recover a 5- or 6-mer in 0.10 - 0.31 of the trials ("Locus motifs")."""
    rng = random.Random(7000 + 13 * RECOVERY_MOTIFS.index(motif) + n_repeat)
    flank = lambda: [rng.choice([1, 2, 4, 8]) for _ in range(10)]
    want = rm.literal_word(least_rotation(motif))
    for trial in range(5):
        slices = [np.array(flank() + list(rm.noisy_repeat(rng, motif, n_repeat)) + flank(), dtype=np.uint8) for _ in range(30)]
        got = lm.find(slices)
        assert got[0] == want and got[1] == len(motif), (trial, lm.motif_text(got[0]), got)
        if trial == 0:
            assert host_find(slices) == got


# ---- the file's line -------------------------------------------------------------------------------------------------------------------
def library_row(chrom, start, end, reads, found, catalogue_word, cap=1 << 12):
    L = call.load()
    rec = np.zeros(1, dtype=hipcall.LOCUS_MOTIF_DTYPE)
    rec[0] = found
    buf = C.create_string_buffer(cap)
    n = L.inq_host_format_locus_motif_row(chrom.encode(), start, end, reads, rec.ctypes.data, catalogue_word, buf, cap)
    return n, buf.value.decode()


AGC, AC = rm.literal_word("AGC"), rm.literal_word("AC")
LINE_CASES = [
    ("the catalogue's CAG is a rotation of the found AGC", (AGC, 3, 120, 90, 70), "CAG", "c7\t10\t50\t4\t120\tAGC\t3\t90\t70\tCAG\t1\n"),
    ("the catalogue's motif is reduced to its root first", (AGC, 3, 120, 90, 70), "gcagca", "c7\t10\t50\t4\t120\tAGC\t3\t90\t70\tGCA\t1\n"),
    ("another motif of the same length", (AGC, 3, 120, 90, 70), "CCG", "c7\t10\t50\t4\t120\tAGC\t3\t90\t70\tCCG\t0\n"),
    ("another length", (AC, 4, 30, 18, 5), "CAG", "c7\t10\t50\t4\t30\tAC\t4\t18\t5\tCAG\t0\n"),
    ("none found counts as 0", (0, 3, 7, 3, 0), "CAG", "c7\t10\t50\t4\t7\t.\t3\t3\t0\tCAG\t0\n"),
    ("no catalogue motif that encodes", (AGC, 3, 120, 90, 70), "GCN", "c7\t10\t50\t4\t120\tAGC\t3\t90\t70\t.\t.\n"),
    ("neither", (0, 0, 0, 0, 0), "", "c7\t10\t50\t4\t0\t.\t0\t0\t0\t.\t.\n"),
]


@pytest.mark.parametrize("name,found,catalogue,want", LINE_CASES, ids=[r[0] for r in LINE_CASES])
def test_format_locus_motif_row(name, found, catalogue, want):
    word = hipcall.encode_motif(catalogue)
    assert lm.locus_line("c7", 10, 50, 4, found, word) == want, "the restatement against the hand-written line"
    assert library_row("c7", 10, 50, 4, found, word) == (len(want), want)
    n, text = library_row("c7", 10, 50, 4, found, word, cap=9)
    assert n == len(want) and text == want[:8]


def test_header_line():
    assert lm.LOCUS_MOTIFS_HEADER.split("\t") == ["chrom", "begin", "end", "reads", "bases", "motif", "period", "tandem", "copies", "catalogue",
                                                  "agrees"]


# ---- the record and the symbols --------------------------------------------------------------------------------------------------------
def test_record_layout_and_symbols(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "inquistr_host.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %zu %zu %zu %d\\n", sizeof(inq_locus_motif_t), offsetof(inq_locus_motif_t, word), '
                   "offsetof(inq_locus_motif_t, period), offsetof(inq_locus_motif_t, bases), offsetof(inq_locus_motif_t, tandem), "
                   "offsetof(inq_locus_motif_t, copies), INQ_ABI_VERSION);\n    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout == "40 0 8 16 24 32 5\n"
    assert hipcall.LOCUS_MOTIF_DTYPE.itemsize == 40
    assert [hipcall.LOCUS_MOTIF_DTYPE.fields[f][1] for f in ("word", "period", "bases", "tandem", "copies")] == [0, 8, 16, 24, 32]
    assert call.CallArgsC._fields_[-1][0] == "evidence_path"  # the arguments of a call did not grow
    L = call.load()
    for sym in ("inq_genotype_repeats_locus_motifs", "inq_host_format_locus_motif_row", "inq_host_locus_motif_find"):
        assert hasattr(L, sym) and sym in call.HOST_ABI_SYMBOLS, sym
    D = hipcall.load()
    for sym in ("inq_call_flush_locus_motifs", "inq_locus_motifs_find"):
        assert hasattr(D, sym) and sym in hipcall.ABI_SYMBOLS, sym
    assert D.inq_abi_version() == 5
    # every entry that takes a context refuses none: no device is touched, nothing is written
    assert D.inq_locus_motifs_find(None, None, 0, None, 0, None, 0, None, None, None) == -1
    assert D.inq_call_flush_locus_motifs(None, None, 0, None, None, None, None, None, None, None, None) == -1
    assert L.inq_host_locus_motif_find(None, None, 0, None) == 1
    one = np.array([4], dtype=np.uint32)
    out = np.zeros(1, dtype=hipcall.LOCUS_MOTIF_DTYPE)
    assert L.inq_host_locus_motif_find(None, one.ctypes.data, 1, out.ctypes.data) == 1
    assert L.inq_host_format_locus_motif_row(None, 0, 0, 0, out.ctypes.data, 0, None, 0) == 0


# ---- the command line ------------------------------------------------------------------------------------------------------------------
def _env():
    e = dict(os.environ)
    e.pop("INQ_SERVER", None)
    return e


def _run(args, env=None):
    return subprocess.run([call.CLI_PATH] + args, capture_output=True, text=True, env=env or _env(), timeout=120)


def test_cli_locus_motifs_flags(tmp_path):
    bam, bed, _loci, _recs, _ties = make_tie_case(tmp_path)
    out = tmp_path / "l.tsv"
    env = _env()
    env["INQ_SERVER"] = str(tmp_path / "no.sock")  # refused before any server is looked for: the socket does not exist
    r = _run(["call", bam, "-R", bed, "--locus-motifs", str(out)], env)
    assert r.returncode == 2, r.stderr
    assert r.stdout == "" and "--locus-motifs" in r.stderr and "INQ_SERVER" in r.stderr and "does not write the locus-motifs file" in r.stderr
    assert not out.exists()
    r = _run(["call", bam, "-R", bed, "--locus-motifs"])
    assert r.returncode == 2 and "--locus-motifs" in r.stderr
    r = _run(["call", "--help"])
    assert r.returncode == 0 and "--locus-motifs <FILE>" in r.stdout and "`auto`" in r.stdout
    r = _run(["cohort", "-R", bed, "--locus-motifs", str(out), "--out-dir", str(tmp_path), bam])
    assert r.returncode == 2 and "--locus-motifs" in r.stderr and not out.exists()


def test_neither_motif_nor_column_four_is_still_status_1(tmp_path):
    """--read-motifs over a BED of three columns without --motif: status 1 and its message, as before; --locus-motifs beside it changes
    nothing about that"""
    bam, bed, _loci, _recs, _ties = make_tie_case(tmp_path)
    assert len(open(bed).readline().split("\t")) == 3
    m, l = tmp_path / "m.tsv", tmp_path / "l.tsv"
    for extra in ([], ["--locus-motifs", str(l)], ["--devices", "0,0", "--locus-motifs", str(l)]):
        r = _run(["call", bam, "-R", bed, "-u", "--read-motifs", str(m)] + extra)
        assert r.returncode == 1, r.stderr
        assert r.stdout == ""
        assert "the read-motifs file needs a motif for every target: column 4 of the BED, or --motif <STR> (needed with -r)" in r.stderr
    r = _run(["call", bam, "-R", bed, "-u", "--read-motifs", str(m), "--motif", "AUTO"])  # only `auto` itself is the word
    assert r.returncode == 1 and r.stdout == "" and "AUTO" in r.stderr


def test_auto_and_the_file_alone_need_no_column_four(tmp_path):
    """`--motif auto` and `--locus-motifs` alone pass the motif check on a BED of three columns and on a region string: the call ends as
    the plain call does on this machine (status 0 with a GPU; without one the same status and message), never with the column-4 message"""
    bam, bed, loci, _recs, _ties = make_tie_case(tmp_path)
    m, l = tmp_path / "m.tsv", tmp_path / "l.tsv"
    region = f"{loci[0][0]}:{loci[0][1]}-{loci[0][2]}"
    for where in (["-R", bed], ["-r", region], ["-R", bed, "--devices", "0,0"]):
        plain = _run(["call", bam, "-u"] + where)
        for flags in (["--read-motifs", str(m), "--motif", "auto"], ["--locus-motifs", str(l)],
                      ["--read-motifs", str(m), "--motif", "auto", "--locus-motifs", str(l)]):
            r = _run(["call", bam, "-u"] + where + flags)
            assert r.returncode == plain.returncode and r.stdout == plain.stdout, r.stderr
            assert "column 4" not in r.stderr
            if r.returncode != 0:
                assert r.stderr == plain.stderr


def test_auto_on_the_reference_bed_passes_the_motif_check(tmp_path):
    from tools import bamio

    bam = str(tmp_path / "plumbing.bam")
    w = bamio.BamWriter(bam, [("chr7", 159345973)])
    w.add("r", 0, 0, 154778000, 60, [("M", 2000)], [("HP", "C", 1)])
    w.close()
    bed = os.path.join(GOLDEN, "reference_test.bed")
    assert len(open(bed).readline().rstrip("\n").split("\t")) == 3
    plain = _run(["call", bam, "-R", bed])
    r = _run(["call", bam, "-R", bed, "--motif", "auto", "--read-motifs", str(tmp_path / "m.tsv"), "--locus-motifs", str(tmp_path / "l.tsv")])
    assert r.returncode == plain.returncode and r.stdout == plain.stdout and "column 4" not in r.stderr


def test_unwritable_locus_motifs_path(tmp_path):
    bam, bed, _loci, _recs, _ties = make_tie_case(tmp_path)
    bad = str(tmp_path / "missing" / "l.tsv")
    for extra in ([], ["--devices", "0,0"]):
        r = _run(["call", bam, "-R", bed, "-u", "--locus-motifs", bad] + extra)
        assert r.returncode == 1, r.stderr
        assert r.stdout == "" and bad in r.stderr and "locus-motifs file" in r.stderr
    out = tmp_path / "o.inq"
    with open(out, "w") as f, pytest.raises(call.CallError) as e:
        call.genotype_repeats(bam, None, bed, 5, 3, 1, True, None, None, out=f, locus_motifs=bad)
    assert e.value.status == 1 and bad in e.value.message and "locus-motifs file" in e.value.message
