"""`inquistr call --read-motifs` end to end: both front ends, phased and unphased, -t 1 and 3, the library entry and the CLI, several
devices - against a plain-Python restatement on the records the BAM was written from, and line for line beside the read-seqs file."""
import os
import subprocess

import pytest

from inquistr_amd import call, hipcall
from tests import read_motif_case as rm
from tests.read_seq_case import file_seq_reads

pytestmark = pytest.mark.gpu


def _cli(args, env):
    e = dict(os.environ)
    e.pop("INQ_SERVER", None)
    e.update(env)
    return subprocess.run([call.CLI_PATH] + args, capture_output=True, text=True, env=e, timeout=300)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """one BAM for every combination; the restated reads, computed once per mode"""
    tmp = tmp_path_factory.mktemp("read_motifs_file")
    bam, bed, loci, recs, col4 = rm.make_motif_case(tmp, 95, n_loci=30)
    return tmp, bam, bed, loci, [hipcall.encode_motif(t) for t in col4], {u: file_seq_reads(loci, recs, u, 5) for u in (False, True)}


_BYTES = {}  # (unphased, threads) -> the file's text: both front ends and --devices give the same bytes


@pytest.mark.parametrize("frontend", ["host", "device"])
@pytest.mark.parametrize("unphased", [False, True])
def test_end_to_end(case, frontend, unphased):
    tmp, bam, bed, loci, words, by_mode = case
    reads = by_mode[unphased]
    out = tmp / f"{frontend}{int(unphased)}"
    out.mkdir()
    kept = [x for c in reads for x in c]
    n_bad = sum(w == 0 for w in words)
    assert 0 < n_bad < len(words) and any(not c for c in reads), "targets without a motif; a target with no kept read"
    assert any(len(x[5]) > 20_000 for x in kept) and any(len(x[5]) == 0 for x in kept), "a soft clip of tens of kilobases; an empty slice"
    u = ["-u"] if unphased else []
    env = {"INQ_FRONTEND": frontend}
    for threads in (1, 3):
        want = rm.motifs_text(loci, reads, words, unphased, threads)
        assert want.startswith(rm.MOTIFS_HEADER + "\n") and want.count("\n") == 1 + len(kept)
        assert "\t.\t.\t.\t.\t.\t.\n" in want and "\tCAG\t" in want and "\tACGTACGTACGTAAA\t" in want
        plain, with_m = out / f"plain{threads}.inq", out / f"m{threads}.inq"
        seqs, motifs = out / f"seqs{threads}.tsv", out / f"motifs{threads}.tsv"
        with open(plain, "w") as f:
            call.genotype_repeats(bam, None, bed, 5, 3, threads, unphased, None, None, out=f, frontend=frontend)
        with open(with_m, "w") as f:
            call.genotype_repeats(bam, None, bed, 5, 3, threads, unphased, None, None, out=f, frontend=frontend, read_seqs=str(seqs),
                                  read_motifs=str(motifs))
        text = motifs.read_text()
        assert text == want, f"library, {frontend}, -t {threads}"
        assert with_m.read_bytes() == plain.read_bytes(), "the .inq is that of the plain call"
        a, b = text.splitlines(), seqs.read_text().splitlines()  # line k of one file is line k of the other
        assert len(a) == len(b) and all(x.split("\t")[:9] == y.split("\t")[:9] for x, y in zip(a[1:], b[1:]))
        assert _BYTES.setdefault((unphased, threads), text) == text, "both front ends give the same bytes"
        # the file alone, through the CLI: stdout is byte for byte that of a plain call; the targets without a motif are counted once
        p = _cli(["call", bam, "-R", bed, "-t", str(threads)] + u, env)
        assert p.returncode == 0, p.stderr
        cli_motifs = out / f"cli{threads}.tsv"
        r = _cli(["call", bam, "-R", bed, "-t", str(threads), "--read-motifs", str(cli_motifs)] + u, env)
        assert r.returncode == 0, r.stderr
        assert r.stdout == p.stdout == plain.read_text()
        assert r.stderr.count(f"{n_bad} of {len(words)} targets") == 1 and r.stderr.count("\n") == p.stderr.count("\n") + 1
        assert cli_motifs.read_text() == want, f"CLI, {frontend}, -t {threads}"
    dev = out / "devices.tsv"
    r = _cli(["call", bam, "-R", bed, "-t", "3", "--devices", "0,0", f"--read-motifs={dev}"] + u, env)
    assert r.returncode == 0, r.stderr
    assert r.stdout == (out / "plain3.inq").read_text()
    assert dev.read_text() == rm.motifs_text(loci, reads, words, unphased, 3), "--devices 0,0"


def test_one_motif_for_a_region(case):
    """--motif is the motif of every target; it is needed with -r and overrides column 4"""
    tmp, bam, bed, loci, _words, by_mode = case
    cag = hipcall.encode_motif("CAG")
    i = max(range(len(loci)), key=lambda k: len(by_mode[False][k]))
    chrom, s, e, _t = loci[i]
    out = tmp / "region.tsv"
    r = _cli(["call", bam, "-r", f"{chrom}:{s}-{e}", "--read-motifs", str(out)], {})
    assert r.returncode == 1 and r.stdout == "" and "column 4" in r.stderr
    r = _cli(["call", bam, "-r", f"{chrom}:{s}-{e}", "--read-motifs", str(out), "--motif", "cagcag"], {})
    assert r.returncode == 0, r.stderr
    assert out.read_text() == rm.motifs_text([loci[i]], [by_mode[False][i]], [cag], False, 1) and len(by_mode[False][i]) > 3
    for frontend in ("host", "device"):
        r = _cli(["call", bam, "-R", bed, "--read-motifs", str(out), "--motif=CAG"], {"INQ_FRONTEND": frontend})
        assert r.returncode == 0 and "targets" not in r.stderr, r.stderr
        assert out.read_text() == rm.motifs_text(loci, by_mode[False], [cag] * len(loci), False, 1)
