"""`inquistr assoc --firth` from the command line on a 40-sample cohort of 24 ordinary loci and one whose long alleles occur in one
group only.  Without the flag, and with `--firth no`, the command prints what it printed before.  With `--firth fallback` the
separated locus alone is fitted by Firth's penalised likelihood: its line says `firth`, has a finite odds ratio and comes first;
every other line is its old line with `glm` appended.  The text is held byte for byte to what tests/assoc_restatement.render_text
makes of the rows inq_assoc_rows_firth returns for the same samples (those rows are held to the restatement by
tests/test_gpu_firth.py), as tests/test_gpu_assoc_cli.py holds the ordinary command's."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from inquistr_amd import call, hipcall
from tests import assoc_cases as ac
from tests import assoc_restatement as ar
from tests import firth_restatement as fr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "inquistr_amd", "lib", "inquistr")
NS, NL, SEPARATED = 40, 25, 11
BASE = ["--phenotype", "grp", "--outcome", "binary", "--binary-order", "N,Y", "--covariates", "age"]


def fmt(v):
    buf = C.create_string_buffer(400)
    call.load().inq_host_format_f64(float(v), buf, 400)
    return buf.value.decode()


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    d = tmp_path_factory.mktemp("firth")
    rng = np.random.default_rng(77)
    names = [f"P{i:02d}" for i in range(NS)]
    y = (rng.random(NS) < 0.45).astype(float)
    y[0], y[1] = 0.0, 1.0
    age = rng.integers(20, 80, NS).astype(float)
    (d / "pheno.tsv").write_text("individual\tgrp\tage\n" + "".join(f"{n}\t{'Y' if v else 'N'}\t{int(a)}\n" for n, v, a in zip(names, y, age)))
    values = np.array([ac.ordinary_row(rng, y, "binary") for _ in range(NL)])
    sep = 12.0 + rng.integers(0, 3, (NS, 2))
    sep[y != 0.0] += 9.0  # every patient's alleles are longer than every control's
    values[SEPARATED] = sep.reshape(-1)
    values[3] = 14.0  # a constant locus: tested by neither fit
    cell = lambda v: "NaN" if np.isnan(v) else (str(int(v)) if float(v).is_integer() else repr(float(v)))
    coords = [(f"chr{1 + r % 3}", 1000 * r, 1000 * r + 40) for r in range(NL)]
    lines = ["chromosome\tbegin\tend\t" + "\t".join(f"{n}_H{h}" for n in names for h in (1, 2))]
    lines += [f"{c}\t{b}\t{e}\t" + "\t".join(cell(x) for x in values[r]) for r, (c, b, e) in enumerate(coords)]
    (d / "cohort.tsv").write_text("\n".join(lines) + "\n")
    return dict(dir=d, path=d / "cohort.tsv", pheno=d / "pheno.tsv", values=values, y=y, cov=age[None, :], ids=[f"{c}:{b}_{e}" for c, b, e in coords])


def cli(cohort, *extra):
    r = subprocess.run([CLI, "assoc", str(cohort["path"]), "--phenocovar", str(cohort["pheno"]), *BASE, *extra], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r


def rendered(rows, firth, ids, all_rows):
    """the text of the command with --firth given: the rows with an OK Firth fit take beta, se and p from it"""
    use = firth["status"] == fr.OK
    shown = rows.copy()
    for f in ("beta", "se", "p"):
        shown[f][use] = firth[f][use]
    lines = ar.render_text(shown, ids, "binary", "grp", ["age"], ["N", "Y"], all_rows, fmt).split("\n")
    method = {i: "firth" if u else "glm" for i, u in zip(ids, use)}
    return "\n".join([lines[0] + "\tmethod"] + [l + "\t" + method[l.split("\t")[0]] for l in lines[1:-1]]) + "\n"


def test_no_flag_and_firth_no_print_the_same_bytes(cohort):
    for extra in ([], ["--all-rows"]):
        a, b = cli(cohort, *extra), cli(cohort, *extra, "--firth", "no")
        assert a.stdout == b.stdout and a.stderr == b.stderr and a.stdout.count("\n") > 20
        assert "method" not in a.stdout


@pytest.mark.parametrize("when", ["fallback", "always"])
def test_text_with_the_flag(cohort, when):
    with hipcall.Context(0) as ctx:
        rows, firth = ctx.assoc_rows_firth(cohort["values"], cohort["y"], cohort["cov"], "max", 0.8, when)
    sep_id = cohort["ids"][SEPARATED]
    assert rows["status"][SEPARATED] == ar.NOT_CONVERGED or rows["se"][SEPARATED] > 100
    assert firth["status"][SEPARATED] == fr.OK and rows["status"][3] == ar.CONSTANT and firth["status"][3] == fr.NOT_FITTED
    for all_rows in (False, True):
        extra = ["--all-rows"] if all_rows else []
        old = cli(cohort, *extra).stdout
        r = cli(cohort, *extra, "--firth", when)
        assert r.stdout == rendered(rows, firth, cohort["ids"], all_rows)
        assert f"fitted by Firth {int((firth['status'] == fr.OK).sum())}" in r.stderr
        new, was = r.stdout.split("\n")[:-1], {l.split("\t")[0]: l for l in old.split("\n")[:-1]}
        assert new[0] == was["VariantID"] + "\tmethod" and len(new) == len(was)
        # the separated locus: last among the tested loci before (p near 1), first now, with a finite odds ratio
        tested = [l.split("\t")[0] for l in old.split("\n")[1:-1] if not all_rows or l.split("\t")[-1] in ("OK", "NOT_CONVERGED")]
        assert tested[-1] == sep_id and new[1].split("\t")[0] == sep_id and new[1].endswith("\tfirth")
        cells = new[1].split("\t")
        assert all(math.isfinite(float(v)) for v in cells[1:6]) and 1.0 < float(cells[1]) < 1e4 and float(cells[5]) < 1e-6
        assert float(was[sep_id].split("\t")[5]) > 0.9
        ps = [float(l.split("\t")[5]) for l in new[1:] if not all_rows or l.split("\t")[-2] in ("OK", "NOT_CONVERGED")]
        assert ps == sorted(ps)
        for l in new[2:]:
            if when == "fallback":
                assert l == was[l.split("\t")[0]] + "\tglm"
            else:  # every tested locus is fitted again; the others keep their line
                assert l.endswith("\tfirth") or l == was[l.split("\t")[0]] + "\tglm"
        if when == "always":
            assert sum(l.endswith("\tfirth") for l in new) == int((firth["status"] == fr.OK).sum()) >= NL - 2
    # the Python mirror and `python -m inquistr_amd` print the same bytes
    out = cohort["dir"] / "mirror.txt"
    with open(out, "w") as f:
        call.assoc(cohort["path"], cohort["pheno"], "grp", "binary", "N,Y", "age", out=f, firth=when)
    assert out.read_text() == rendered(rows, firth, cohort["ids"], False)
    m = subprocess.run([sys.executable, "-m", "inquistr_amd", "assoc", str(cohort["path"]), "--phenocovar", str(cohort["pheno"]), *BASE, "--firth", when],
                       capture_output=True, text=True, cwd=ROOT)
    assert m.returncode == 0 and m.stdout == out.read_text()
