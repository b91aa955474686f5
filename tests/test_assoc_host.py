"""`inquistr assoc` above the C ABI, without a GPU: the loud failure, every input error (exit status 101), how the phenotype file picks
the analysed samples, and the new entries' place in the two ABIs.  Moving the text readers of `outlier` into a header `assoc` shares must
not change `outlier`: its output on the reference's own .inq fixtures is held to what the commit before printed (recorded on an
MI355X in tests/golden/outlier_parent_output.json; that test needs the device)."""
import ctypes as C
import gzip
import json
import os
import re
import subprocess

import numpy as np
import pytest

from inquistr_amd import call, hipcall

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CLI = os.path.join(ROOT, "inquistr_amd", "lib", "inquistr")
NAMES = [f"S{i}" for i in range(8)]


def _have_gpu():
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.fixture()
def files(tmp_path):
    """8 samples x 5 loci; the phenotype file lists S0 .. S6 (S3 with an unparseable covariate) and a sample the cohort lacks"""
    rng = np.random.default_rng(3)
    head = "chromosome\tbegin\tend\t" + "\t".join(f"{n}_H{h}" for n in NAMES for h in (1, 2))
    rows = [f"chr{1 + i % 2}\t{100 * i}\t{100 * i + 20}\t" + "\t".join(str(int(v)) for v in rng.integers(5, 20, 16)) for i in range(5)]
    comb = tmp_path / "c.tsv"
    comb.write_text(head + "\n" + "\n".join(rows) + "\n")
    ph = tmp_path / "p.tsv"
    ph.write_text("individual\tgrp\tage\tw\n" + "".join(f"{n}\t{'Y' if i % 2 else 'N'}\t{30 + i}\t{'NA' if i == 3 else i * 1.5}\n"
                                                       for i, n in enumerate(NAMES[:7])) + "ZZ\tY\t1\t1\n")
    return comb, ph, head, rows


def _cli(*args):
    return subprocess.run([CLI, "assoc"] + [str(a) for a in args], capture_output=True, text=True)


@pytest.mark.skipif(_have_gpu(), reason="checks the no-GPU failure mode")
def test_fails_loudly_without_a_gpu(files):
    comb, ph, _, _ = files
    r = _cli(comb, "--phenocovar", ph, "--phenotype", "grp", "--outcome", "binary", "--binary-order", "N,Y")
    assert r.returncode == 1 and "no CPU fallback" in r.stderr and r.stdout == ""
    with pytest.raises(call.CallError) as e:
        call.assoc(comb, ph, "age", "continuous")
    assert e.value.status == 1 and "no CPU fallback" in e.value.message


def test_wrong_input_is_exit_101(files, tmp_path):
    comb, ph, head, rows = files
    base = ["--phenocovar", ph, "--phenotype", "grp", "--outcome", "binary", "--binary-order", "N,Y"]

    def is_101(r, text):
        return r.returncode == 101 and "panicked" in r.stderr and text in r.stderr and r.stdout == ""

    assert is_101(_cli(tmp_path / "missing.tsv", *base), "Combined file does not exist!")
    assert is_101(_cli(comb, "--phenocovar", tmp_path / "missing.tsv", "--phenotype", "grp", "--outcome", "continuous"), "Metadata file does not exist!")
    assert is_101(_cli(comb, "--phenocovar", ph, "--phenotype", "grp", "--outcome", "binary"), "--binary-order is missing")
    assert is_101(_cli(comb, "--phenocovar", ph, "--phenotype", "grp", "--outcome", "binary", "--binary-order", "N"), "two different values")
    assert is_101(_cli(comb, "--phenocovar", ph, "--phenotype", "nope", "--outcome", "continuous"), "phenotype variable nope is not a column")
    assert is_101(_cli(comb, *base, "--covariates", "age,height"), "covariate height is not a column")
    assert is_101(_cli(comb, "--phenocovar", ph, "--phenotype", "grp", "--outcome", "continuous"), "Not enough samples")  # N / Y are no numbers
    assert is_101(_cli(comb, "--phenocovar", ph, "--phenotype", "grp", "--outcome", "binary", "--binary-order", "N,Q"), "Not enough samples") is False  # N alone: 4 samples
    assert is_101(_cli(comb, "--phenocovar", ph, "--phenotype", "grp", "--outcome", "binary", "--binary-order", "P,Q"), "Not enough samples")
    assert is_101(_cli(comb, *base, "--chr", "chr1", "--chr-begin", "5"), "go together")
    bad = tmp_path / "bad.tsv"
    bad.write_text(head + "\n" + rows[0] + "\n" + rows[1].replace("\t", "\tx", 4).replace("\tx", "\t", 3) + "\n")
    assert is_101(_cli(bad, *base), "Failed to parse number")  # a number that does not parse
    short = tmp_path / "short.tsv"
    short.write_text(head + "\n" + rows[0] + "\nchr1\t5\n")
    assert is_101(_cli(short, *base), "fewer than three fields")
    odd = tmp_path / "odd.tsv"
    odd.write_text(head + "\tS9_H1\n" + rows[0] + "\t3\n")
    assert is_101(_cli(odd, *base), "H1 / H2 pairs")
    empty = tmp_path / "empty.tsv"
    empty.write_text("")
    assert is_101(_cli(empty, *base), "empty combined file")
    with pytest.raises(call.CallError) as e:
        call.assoc(tmp_path / "missing.tsv", ph, "grp", "binary", "N,Y")
    assert e.value.status == 101
    # what the command line itself refuses is the usage error 2, as for the other commands
    assert _cli(comb, "--phenocovar", ph, "--phenotype", "grp").returncode == 2
    assert _cli(comb, *base, "--outcome", "ordinal").returncode == 2 and _cli(comb, *base, "--missing-cutoff", "abc").returncode == 2
    r = subprocess.run([CLI, "bogus"], capture_output=True, text=True)
    assert r.returncode == 2 and "`assoc`" in r.stderr


def test_phenotype_file_picks_the_samples(files, tmp_path):
    comb, ph, head, rows = files
    # the column is found by its name; S7 is in the cohort only, ZZ in the phenotype file only
    names, y, cov = call.assoc_samples(comb, ph, "grp", "binary", "N,Y")
    assert names == NAMES[:7] and y.tolist() == [0, 1, 0, 1, 0, 1, 0] and cov.shape == (0, 7)
    names, y, cov = call.assoc_samples(comb, ph, "grp", "binary", ["Y", "N"], ["age"])
    assert names == NAMES[:7] and y.tolist() == [1, 0, 1, 0, 1, 0, 1] and cov.tolist() == [[30, 31, 32, 33, 34, 35, 36]]
    # an unparseable covariate drops its sample for every locus
    names, y, cov = call.assoc_samples(comb, ph, "grp", "binary", "N,Y", "age,w")
    assert names == ["S0", "S1", "S2", "S4", "S5", "S6"] and y.tolist() == [0, 1, 0, 0, 1, 0]
    assert cov.tolist() == [[30, 31, 32, 34, 35, 36], [0, 1.5, 3, 6, 7.5, 9]]
    # a continuous outcome takes the samples whose phenotype is a number; a third group leaves the binary analysis
    names, y, _ = call.assoc_samples(comb, ph, "w", "continuous")
    assert names == ["S0", "S1", "S2", "S4", "S5", "S6"] and y.tolist() == [0, 1.5, 3, 6, 7.5, 9]
    ph3 = tmp_path / "p3.tsv"
    ph3.write_text("id\tage\tgrp\nS7\t1\tcase\nS0\t2\tcontrol\nS5\t3\tother\nS2\t4\tcase\nS0\t9\tcase\n")
    names, y, cov = call.assoc_samples(comb, ph3, "grp", "binary", "control,case", "age")
    assert names == ["S0", "S2", "S7"] and y.tolist() == [0, 1, 1] and cov.tolist() == [[2, 4, 1]]  # cohort order; a sample's first line counts
    gz = tmp_path / "c.tsv.gz"
    with gzip.open(gz, "wt") as f:
        f.write(comb.read_text())
    assert call.assoc_samples(gz, ph, "grp", "binary", "N,Y")[0] == NAMES[:7]
    with pytest.raises(call.CallError) as e:
        call.assoc_samples(comb, ph, "nope", "continuous")
    assert e.value.status == 101


def test_new_entries_in_both_abis():
    D, L = hipcall.load(), call.load()
    assert "inq_assoc_rows" in hipcall.ABI_SYMBOLS and hasattr(D, "inq_assoc_rows") and D.inq_assoc_rows.argtypes is not None
    assert len(D.inq_assoc_rows.argtypes) == 11 and D.inq_abi_version() == 5
    for sym in ("inq_assoc", "inq_assoc_samples"):
        assert hasattr(L, sym) and sym in call.HOST_ABI_SYMBOLS, sym
    # the row's size and offsets are fixed in the header's comment
    hdr = open(os.path.join(ROOT, "include", "inquistr_hip.h")).read()
    m = re.search(r"inq_assoc_row_t is (\d+) bytes: ([^.]*)\.", hdr)
    assert m and int(m.group(1)) == 88 == C.sizeof(hipcall.AssocRowC) == hipcall.ASSOC_ROW_DTYPE.itemsize
    stated = {name: int(off) for name, off in re.findall(r"([a-z_0-9]+) (\d+)", m.group(2).replace("\n", " ").replace("*", " "))}
    assert stated == {f: getattr(hipcall.AssocRowC, f).offset for f, _ in hipcall.AssocRowC._fields_}
    assert stated == {f: hipcall.ASSOC_ROW_DTYPE.fields[f][1] for f in hipcall.ASSOC_ROW_DTYPE.names}
    for name, val in (("INQ_ASSOC_BINARY", 0), ("INQ_ASSOC_CONTINUOUS", 1), ("INQ_ASSOC_MAX", 0), ("INQ_ASSOC_MIN", 1), ("INQ_ASSOC_MEAN", 2)):
        assert re.search(rf"#define {name} {val}\b", hdr), name
    for val, name in enumerate(hipcall.ASSOC_STATUS):
        assert re.search(rf"#define INQ_ASSOC_ROW_{name} {val}\b", hdr), name
    assert C.sizeof(call.AssocArgsC) == 6 * 8 + 2 * 8 + 8 + 4 * 4


@pytest.mark.gpu
def test_outlier_prints_what_the_commit_before_printed():
    """`inquistr outlier --minsize 0 -z 1.0` with both methods on the reference's file1 .. file3.inq, plain and gzip: exit status,
    standard output and the message, byte for byte"""
    rec = json.load(open(os.path.join(GOLDEN, "outlier_parent_output.json")))
    assert len(rec) == 12
    for key, want in rec.items():
        name, method = key.split(":")
        r = subprocess.run([CLI, "outlier", os.path.join(GOLDEN, name), "--method", method, "--minsize", "0", "-z", "1.0"], capture_output=True, text=True)
        assert (r.returncode, r.stdout, r.stderr) == (want["status"], want["stdout"], want["stderr"]), key
