"""`inquistr call --read-seqs` end to end: both front ends, phased and unphased, -t 1 and 4, the library entry and the CLI, several
devices - against a plain-Python restatement on the records the BAM was written from, and against the read table of the same call."""
import os
import subprocess

import pytest

from inquistr_amd import call
from tests.read_seq_case import SEQS_HEADER, file_seq_reads, make_seq_case, seqs_text
from tests.test_tie_report import row_order

pytestmark = pytest.mark.gpu


def _cli(args, env):
    e = dict(os.environ)
    e.pop("INQ_SERVER", None)
    e.update(env)
    return subprocess.run([call.CLI_PATH] + args, capture_output=True, text=True, env=e, timeout=300)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """one BAM for every combination; the restated reads, computed once per mode"""
    tmp = tmp_path_factory.mktemp("read_seqs")
    bam, bed, loci, recs = make_seq_case(tmp, 91, n_loci=30)
    return tmp, bam, bed, loci, {u: file_seq_reads(loci, recs, u, 5) for u in (False, True)}


_BYTES = {}  # (unphased, threads) -> the file's text: both front ends and --devices give the same bytes


@pytest.mark.parametrize("frontend", ["host", "device"])
@pytest.mark.parametrize("unphased", [False, True])
def test_end_to_end(case, frontend, unphased):
    tmp, bam, bed, loci, by_mode = case
    reads = by_mode[unphased]
    out = tmp / f"{frontend}{int(unphased)}"
    out.mkdir()
    # what the case must hold for the file to say anything
    kept = [x for c in reads for x in c]
    assert any(x[0] == "Clip" and len(x[5]) > x[1] > 0 for x in kept), "a Clip whose slice contains the clip"
    assert any(len(x[5]) == 0 for x in kept), "an empty slice"
    by_name = {}
    for x in kept:
        by_name.setdefault(x[3], set()).add((x[4], bytes(x[5])))
    assert any(len(v) > 1 for v in by_name.values()), "a read kept by two loci with different slices"
    assert any(not c for c in reads), "a target with no kept read"
    assert row_order(loci, 4) != row_order(loci, 1)
    u = ["-u"] if unphased else []
    for threads in (1, 4):
        want = seqs_text(loci, reads, unphased, threads)
        assert want.startswith(SEQS_HEADER + "\n") and want.count("\n") == 1 + len(kept)
        plain, with_s = out / f"plain{threads}.inq", out / f"s{threads}.inq"
        files = {k: out / f"{k}{threads}.tsv" for k in ("rc", "ev", "tf", "table", "seqs", "rc0", "ev0", "tf0", "table0")}
        with open(plain, "w") as f:
            call.genotype_repeats(bam, None, bed, 5, 3, threads, unphased, None, None, out=f, frontend=frontend, ties=str(files["tf0"]),
                                  evidence=str(files["ev0"]), read_calls=str(files["rc0"]), read_table=str(files["table0"]))
        with open(with_s, "w") as f:
            call.genotype_repeats(bam, None, bed, 5, 3, threads, unphased, None, None, out=f, frontend=frontend, ties=str(files["tf"]),
                                  evidence=str(files["ev"]), read_calls=str(files["rc"]), read_table=str(files["table"]),
                                  read_seqs=str(files["seqs"]))
        text = files["seqs"].read_text()
        assert text == want, f"library, {frontend}, -t {threads}"
        # the .inq and the other four files are those of the call without the file
        assert with_s.read_bytes() == plain.read_bytes()
        for k in ("rc", "ev", "tf", "table"):
            assert files[k].read_bytes() == files[k + "0"].read_bytes(), k
        # line k of one file is line k of the other: columns 1 - 7 agree
        a, b = text.splitlines(), files["table"].read_text().splitlines()
        assert len(a) == len(b) and all(x.split("\t")[:7] == y.split("\t")[:7] for x, y in zip(a, b))
        assert _BYTES.setdefault((unphased, threads), text) == text, "both front ends give the same bytes"
        # the file alone, through the CLI: stdout and stderr are those of the call without the flag
        env = {"INQ_FRONTEND": frontend}
        p = _cli(["call", bam, "-R", bed, "-t", str(threads)] + u, env)
        assert p.returncode == 0, p.stderr
        cli_seqs = out / f"cli{threads}.tsv"
        r = _cli(["call", bam, "-R", bed, "-t", str(threads), "--read-seqs", str(cli_seqs)] + u, env)
        assert r.returncode == 0, r.stderr
        assert r.stdout == p.stdout and r.stderr == p.stderr and r.stdout == plain.read_text()
        assert cli_seqs.read_text() == want, f"CLI, {frontend}, -t {threads}"
    dev_seqs, dev_table = out / "devices.tsv", out / "devices_table.tsv"
    r = _cli(["call", bam, "-R", bed, "-t", "4", "--devices", "0,0", f"--read-seqs={dev_seqs}", "--read-table", str(dev_table)] + u,
             {"INQ_FRONTEND": frontend})
    assert r.returncode == 0, r.stderr
    assert r.stdout == (out / "plain4.inq").read_text()
    assert dev_seqs.read_text() == seqs_text(loci, reads, unphased, 4), "--devices 0,0"
    assert dev_table.read_bytes() == (out / "table04.tsv").read_bytes()
