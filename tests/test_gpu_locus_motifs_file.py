"""The motif each locus's reads repeat at flush time (inq_call_flush_locus_motifs: locus_motifs.hip launched behind the slices' records
and in front of the motif kernel, which reads the words it wrote) and end to end: `inquistr call --motif auto --read-motifs` and
`--locus-motifs` through both front ends, phased and unphased, -t 1 and 4, several devices - against the plain-Python restatement on the
records the BAM was written from."""
import os
import subprocess

import numpy as np
import pytest

from inquistr_amd import batch as B
from inquistr_amd import call, hipcall
from tests import gen
from tests import locus_motif_case as lm
from tests import read_motif_case as rm
from tests import read_seq_case as rs
from tests.read_seq_case import file_seq_reads
from tests.test_gpu_read_seqs import _append, _spans
from tests.test_host_frontend import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = hipcall.Context(0)
    assert c.backend.startswith("hip:gfx950")
    yield c
    c.close()


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """one BAM for every test; the restated reads, computed once per mode"""
    tmp = tmp_path_factory.mktemp("locus_motifs_file")
    bam, bed, loci, recs, col4 = rm.make_motif_case(tmp, 97, n_loci=30)
    bed3 = str(tmp / "three.bed")
    with open(bed3, "w") as f:
        for c, s, e, _t in loci:
            f.write(f"{c}\t{s}\t{e}\n")
    return tmp, bam, bed, bed3, loci, [hipcall.encode_motif(t) for t in col4], {u: file_seq_reads(loci, recs, u, 5) for u in (False, True)}


@pytest.mark.parametrize("unphased", [False, True])
def test_flush_with_locus_motifs(ctx, case, unphased):
    _tmp, bam, bed, _bed3, _loci, target_words, _ = case
    spans = _spans(bam, bed, unphased, 8_000)
    n_spans = len(spans)
    assert n_spans >= 2, "several spans in one batch"
    words = np.array([target_words[int(i)] for s in spans for i in s["locus_index"]], dtype=np.uint64)
    assert (words == 0).any() and (words != 0).any()
    ctx.call_discard()
    assert _append(ctx, spans, unphased)[0] == [0] * n_spans
    n_loci = ctx.deferred_loci
    out = ctx.call_flush_locus_motifs(words)
    rc, p1, p2, ties, _ms, flags, ev, off, rec, org, raw, name_total, sq, packed, seq_total, mt, found = out
    assert rc == 0 and found.dtype == hipcall.LOCUS_MOTIF_DTYPE and len(found) == n_loci and len(mt) == len(rec) == int(off[-1]) > 20
    # the restatement on the written records: record kk of locus j is a kept pair of j, its slice the window's
    written = [r for s in spans for r in rs.span_seq_records(s)]
    starts = np.concatenate([s["locus_start"] for s in spans])
    ends = np.concatenate([s["locus_end"] for s in spans])
    slices = []
    for j in range(n_loci):
        for kk in range(int(off[j]), int(off[j + 1])):
            wds, pos, l_seq, codes_ = written[int(rec["read"][kk])]
            q, n = rs.window(wds, pos, l_seq, int(starts[j]), int(ends[j]))
            slices.append(codes_[q : q + n])
    want = lm.records_of(slices, off)
    assert found.tobytes() == want.tobytes(), [(j, tuple(found[j]), tuple(want[j])) for j in range(n_loci) if found[j] != want[j]][:5]
    assert (want["word"] != 0).sum() > 5 and (want["bases"] == 0).any() and len(set(int(p) for p in want["period"])) >= 3
    # the read-motif records are those of every kept record under the words in use: the given one, else the found one
    use = lm.words_in_use(words, want["word"])
    assert any(g == 0 and u != 0 for g, u in zip(words, use)), "a locus without a given motif whose reads repeat one"
    rec_words = [int(use[j]) for j in range(n_loci) for _ in range(int(off[j]), int(off[j + 1]))]
    assert mt.tobytes() == rm.records_of(slices, rec_words).tobytes()
    # ... and the kernel alone, fed with what inq_read_seqs_fetch returned
    alone, alone_use = ctx.locus_motifs_find(sq, packed, off, words)
    assert alone.tobytes() == found.tobytes() and np.array_equal(alone_use, use)

    # no given word at all: every locus is measured with what was found
    _append(ctx, spans, unphased)
    auto = ctx.call_flush_locus_motifs(None)
    assert auto[0] == 0 and auto[16].tobytes() == want.tobytes()
    auto_words = [int(want["word"][j]) for j in range(n_loci) for _ in range(int(off[j]), int(off[j + 1]))]
    assert auto[15].tobytes() == rm.records_of(slices, auto_words).tobytes()
    rc2, few = ctx.read_motifs_fetch(3, check=False)
    assert rc2 == 0 and few.tobytes() == auto[15][:3].tobytes()

    # found NULL is exactly inq_call_flush_motifs
    _append(ctx, spans, unphased)
    a = ctx.call_flush_locus_motifs(words, found=False)
    _append(ctx, spans, unphased)
    b = ctx.call_flush_motifs(words)
    assert a[16] is None and a[0] == b[0] == 0
    for x, y in zip(a[:16], b):
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and (gen.same_f64(x, y) if x.dtype == np.float64 else x.tobytes() == y.tobytes())
        elif not isinstance(x, float):  # (ms_call is a time)
            assert x == y or bytes(x) == bytes(y)
    assert a[15].tobytes() == rm.records_of(slices, [int(words[j]) for j in range(n_loci) for _ in range(int(off[j]), int(off[j + 1]))]).tobytes()

    # with found, the bases are required; a batch appended without sequences has none - and stays
    assert _append(ctx, spans, unphased, seqs=False)[0] == [0] * n_spans
    n = ctx.deferred_loci
    assert ctx.call_flush_locus_motifs(None, check=False)[0] == B.INQ_ERR_ARG and ctx.deferred_loci == n
    ctx.call_discard()
    p1_ = np.zeros(1)
    res = hipcall.InqResultC(p1_.ctypes.data, p1_.ctypes.data, None, None, 0)
    one = np.zeros(2, dtype=np.uint64)
    fd = np.zeros(1, dtype=hipcall.LOCUS_MOTIF_DTYPE)
    assert ctx._L.inq_call_flush_locus_motifs(ctx._h, hipcall.C.byref(res), 0, None, None, None, one.ctypes.data, one.ctypes.data, None, None,
                                              fd.ctypes.data) == B.INQ_ERR_ARG, "found without seq_bytes"


def _cli(args, env):
    e = dict(os.environ)
    e.pop("INQ_SERVER", None)
    e.update(env)
    return subprocess.run([call.CLI_PATH] + args, capture_output=True, text=True, env=e, timeout=300)


_BYTES = {}  # (unphased, threads, which file) -> its text: both front ends and --devices give the same bytes


@pytest.mark.parametrize("frontend", ["host", "device"])
@pytest.mark.parametrize("unphased", [False, True])
def test_end_to_end(case, frontend, unphased):
    tmp, bam, bed, bed3, loci, words, by_mode = case
    reads = by_mode[unphased]
    out = tmp / f"{frontend}{int(unphased)}"
    out.mkdir()
    found_words = [f[0] for f in lm.found_of(reads)]
    n_found = sum(w != 0 for w in found_words)
    assert 3 < n_found < len(loci) and any(w == 0 and f != 0 for w, f in zip(words, found_words))
    u = ["-u"] if unphased else []
    env = {"INQ_FRONTEND": frontend}
    for threads in (1, 4):
        want_auto = rm.motifs_text(loci, reads, found_words, unphased, threads)
        want_loci = lm.locus_motifs_text(loci, reads, words, threads)
        want_loci3 = lm.locus_motifs_text(loci, reads, [0] * len(loci), threads)
        n_zero = sum(line.endswith("\t0") for line in want_loci.splitlines())
        assert n_zero > 0 and "\t1\n" in want_loci and "\t.\n" in want_loci and "\tAGC\t" in want_auto and "\t.\t.\t.\t.\t.\t.\n" in want_auto
        p = _cli(["call", bam, "-R", bed3, "-t", str(threads)] + u, env)
        assert p.returncode == 0, p.stderr
        # the README's command line: a BED of three columns, both files
        m, l = out / f"m{threads}.tsv", out / f"l{threads}.tsv"
        r = _cli(["call", bam, "-R", bed3, "-t", str(threads), "--motif", "auto", "--read-motifs", str(m), "--locus-motifs", str(l)] + u, env)
        assert r.returncode == 0, r.stderr
        assert r.stdout == p.stdout and r.stderr.count("\n") == p.stderr.count("\n"), "the .inq of the plain call; no catalogue, nothing to count"
        assert m.read_text() == want_auto, f"--motif auto, {frontend}, -t {threads}"
        assert l.read_text() == want_loci3, f"--locus-motifs, three columns, {frontend}, -t {threads}"
        # a catalogue in column 4: `auto` does not read it for the runs, the locus-motifs file compares with it
        r = _cli(["call", bam, "-R", bed, "-t", str(threads), "--motif", "auto", "--read-motifs", str(m), "--locus-motifs", str(l)] + u, env)
        assert r.returncode == 0, r.stderr
        assert r.stdout == p.stdout and m.read_text() == want_auto and l.read_text() == want_loci
        assert r.stderr.count(f"{n_zero} of {len(loci)} targets") == 1 and r.stderr.count("\n") == p.stderr.count("\n") + 1
        # the locus-motifs file alone, and beside a read-motifs file under column 4, which stays what it was
        r = _cli(["call", bam, "-R", bed, "-t", str(threads), "--locus-motifs", str(l), "--read-motifs", str(m)] + u, env)
        assert r.returncode == 0 and r.stdout == p.stdout and l.read_text() == want_loci, r.stderr
        assert m.read_text() == rm.motifs_text(loci, reads, words, unphased, threads)
        lib = out / f"lib{threads}.tsv"
        with open(out / f"lib{threads}.inq", "w") as f:
            call.genotype_repeats(bam, None, bed, 5, 3, threads, unphased, None, None, out=f, frontend=frontend, locus_motifs=str(lib))
        assert lib.read_text() == want_loci and (out / f"lib{threads}.inq").read_text() == p.stdout
        assert _BYTES.setdefault((unphased, threads, "m"), want_auto) == want_auto and _BYTES.setdefault((unphased, threads, "l"), want_loci) == want_loci
    dm, dl = out / "dm.tsv", out / "dl.tsv"
    r = _cli(["call", bam, "-R", bed, "-t", "4", "--devices", "0,0", "--motif=auto", f"--read-motifs={dm}", f"--locus-motifs={dl}"] + u, env)
    assert r.returncode == 0, r.stderr
    assert dm.read_text() == rm.motifs_text(loci, reads, found_words, unphased, 4), "--devices 0,0"
    assert dl.read_text() == lm.locus_motifs_text(loci, reads, words, 4), "--devices 0,0"


def test_one_motif_for_every_target_is_the_catalogue(case):
    tmp, bam, bed, _bed3, loci, _words, by_mode = case
    cag = hipcall.encode_motif("CAG")
    l = tmp / "one.tsv"
    r = _cli(["call", bam, "-R", bed, "--motif", "gcagca", "--locus-motifs", str(l)], {})
    assert r.returncode == 0, r.stderr
    assert l.read_text() == lm.locus_motifs_text(loci, by_mode[False], [hipcall.encode_motif("GCA")] * len(loci), 1) and "\tGCA\t1\n" in l.read_text()
    i = max(range(len(loci)), key=lambda k: len(by_mode[False][k]))
    chrom, s, e, _t = loci[i]
    m = tmp / "region.tsv"
    r = _cli(["call", bam, "-r", f"{chrom}:{s}-{e}", "--motif", "auto", "--read-motifs", str(m), "--locus-motifs", str(l)], {})
    assert r.returncode == 0, r.stderr
    word = lm.found_of([by_mode[False][i]])[0][0]
    assert m.read_text() == rm.motifs_text([loci[i]], [by_mode[False][i]], [word], False, 1) and word != 0 and cag
    assert l.read_text() == lm.locus_motifs_text([loci[i]], [by_mode[False][i]], [0], 1)


def test_auto_on_the_reference_bed(tmp_path):
    from tools import bamio

    bam = str(tmp_path / "plumbing.bam")
    w = bamio.BamWriter(bam, [("chr7", 159345973)])
    w.add("r", 0, 0, 154778000, 60, [("M", 2000)], [("HP", "C", 1)])
    w.close()
    bed = os.path.join(GOLDEN, "reference_test.bed")
    m, l = tmp_path / "m.tsv", tmp_path / "l.tsv"
    p = _cli(["call", bam, "-R", bed], {})
    r = _cli(["call", bam, "-R", bed, "--motif", "auto", "--read-motifs", str(m), "--locus-motifs", str(l)], {})
    assert p.returncode == 0 and r.returncode == 0, r.stderr
    assert r.stdout == p.stdout and m.read_text().startswith(rm.MOTIFS_HEADER + "\n")
    assert l.read_text().startswith(lm.LOCUS_MOTIFS_HEADER + "\nchr7\t154778571\t154779363\t") and l.read_text().endswith("\t.\t.\n")
