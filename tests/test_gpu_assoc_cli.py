"""`inquistr assoc` from the command line on a 40-sample, 60-locus cohort, plain and gzip: binary with and without a covariate, and
continuous.  The text is held in two steps.  (1) Byte for byte it is what tests/assoc_restatement.render_text makes of the rows
inq_assoc_rows returns for the same samples: header, columns, row order, every digit.  (2) Those rows are the restatement's within the
tolerance of tests/test_gpu_assoc.py, and so is the text: rendered from the restatement's rows it has the same header, the same loci in
the same order, the same counts and names, and numbers that differ by no more than that tolerance allows (a printed number is the
shortest decimal that reads back as the f64, so a difference in the last bit is a different text: the digits cannot be held
exactly to a CPU computation that sums in another order)."""
import ctypes as C
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from inquistr_amd import call, hipcall
from tests import assoc_cases as ac
from tests import assoc_restatement as ar

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "inquistr_amd", "lib", "inquistr")
NS, NL = 40, 60
CONFIGS = {
    "binary": dict(phenotype="grp", outcome="binary", binary_order="N,Y", covariates=None),
    "binary_cov": dict(phenotype="grp", outcome="binary", binary_order="N,Y", covariates="age"),
    "continuous": dict(phenotype="bmi", outcome="continuous", binary_order=None, covariates="age"),
}


def fmt(v):
    buf = C.create_string_buffer(400)
    call.load().inq_host_format_f64(float(v), buf, 400)
    return buf.value.decode()


def cell(v):
    return "NaN" if np.isnan(v) else (str(int(v)) if float(v).is_integer() else repr(float(v)))


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    d = tmp_path_factory.mktemp("assoc")
    rng = np.random.default_rng(2024)
    names = [f"P{i:02d}" for i in range(NS)]
    grp = np.array(["Y" if v else "N" for v in rng.random(NS) < 0.45])
    grp[0], grp[1], grp[5] = "N", "Y", "X"  # P05 is in a third group
    age = rng.integers(20, 80, NS).astype(float)
    bmi = np.round(rng.normal(25, 4, NS), 2)
    listed = [i for i in range(NS) if i != 9]  # P09 is not in the phenotype file
    ph = d / "pheno.tsv"
    ph.write_text("individual\tgrp\tage\tbmi\n" + "".join(f"{names[i]}\t{grp[i]}\t{cell(age[i])}\t{'NA' if i == 12 else bmi[i]}\n" for i in listed))
    ybin = (grp == "Y").astype(float)
    use = np.array([i for i in listed if grp[i] in "NY"])
    rows = []
    for r in range(NL):
        for _ in range(60):  # drawn again until the row ends outside the convergence band in both binary analyses (tests/assoc_cases.py)
            h = np.full(2 * NS, np.nan, dtype=np.float32)
            lean = ybin if r % 2 else (bmi - bmi.mean()) / bmi.std()
            v = ac.ordinary_row(rng, lean, "binary")
            h[:] = v
            if r in (7, 31):
                h[:] = 14.0  # constant
            if r == 19:
                h[:] = np.nan
            if r == 44:
                h[rng.choice(2 * NS, 60, replace=False)] = np.nan
            sel = np.stack([2 * use, 2 * use + 1], axis=1).reshape(-1)
            crits = [ar.fit_row(h[sel][0::2], h[sel][1::2], ybin[use], cov, "binary")[1] for cov in (None, age[use][None, :])]
            if not any(ac.in_band(c) for c in crits):
                break
        rows.append(h)
    values = np.array(rows)
    coords = [(f"chr{1 + r % 3}", 1000 * r, 1000 * r + 40) for r in range(NL)]
    lines = ["chromosome\tbegin\tend\t" + "\t".join(f"{n}_H{h}" for n in names for h in (1, 2))]
    lines += [f"{c}\t{b}\t{e}\t" + "\t".join(cell(x) for x in values[r]) for r, (c, b, e) in enumerate(coords)]
    plain, gz = d / "cohort.tsv", d / "cohort.tsv.gz"
    plain.write_text("\n".join(lines) + "\n")
    with gzip.open(gz, "wt") as f:
        f.write("\n".join(lines) + "\n")
    return dict(dir=d, plain=plain, gz=gz, pheno=ph, names=names, values=values, coords=coords, lines=lines)


def cli(*args):
    r = subprocess.run([CLI, "assoc"] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r


def flags(cfg):
    out = ["--phenotype", cfg["phenotype"], "--outcome", cfg["outcome"]]
    if cfg["binary_order"]:
        out += ["--binary-order", cfg["binary_order"]]
    if cfg["covariates"]:
        out += ["--covariates", cfg["covariates"]]
    return out


def same_text_within(a, b, tol):
    la, lb = a.split("\n"), b.split("\n")
    assert la[0] == lb[0] and len(la) == len(lb)
    for x, y in zip(la[1:], lb[1:]):
        fx, fy = x.split("\t"), y.split("\t")
        assert len(fx) == len(fy)
        for u, v in zip(fx, fy):
            if u != v:
                assert ar.rel_diff([float(u)], [float(v)]) <= tol, (x, y)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_text_of_the_command(cohort, name):
    cfg = CONFIGS[name]
    names, y, cov = call.assoc_samples(cohort["plain"], cohort["pheno"], cfg["phenotype"], cfg["outcome"], cfg["binary_order"], cfg["covariates"])
    assert len(names) == 38  # binary: without P09 and P05; continuous: without P09 and P12
    idx = np.array([cohort["names"].index(n) for n in names])
    sel = np.stack([2 * idx, 2 * idx + 1], axis=1).reshape(-1)
    case = ac.Case(cohort["values"][:, sel], y, cov, cfg["outcome"], "max")
    with hipcall.Context(0) as ctx:
        got = ctx.assoc_rows(case.values, y, cov, cfg["outcome"], "max", 0.8)
    ac.compare(case, got)
    ids = [f"{c}:{b}_{e}" for c, b, e in cohort["coords"]]
    covs = cfg["covariates"].split(",") if cfg["covariates"] else []
    order = cfg["binary_order"].split(",") if cfg["binary_order"] else None
    for all_rows in (False, True):
        want = ar.render_text(got, ids, cfg["outcome"], cfg["phenotype"], covs, order, all_rows, fmt)
        extra = ["--all-rows"] if all_rows else []
        for path in (cohort["plain"], cohort["gz"]):
            r = cli(path, "--phenocovar", cohort["pheno"], *flags(cfg), *extra)
            assert r.stdout == want, path.name
            assert f"{NL} loci, {len(names)} samples" in r.stderr and "LOW_CALL_RATE 2" in r.stderr and "CONSTANT 2" in r.stderr
        # the Python mirror prints the same bytes
        out = cohort["dir"] / "mirror.txt"
        with open(out, "w") as f:
            call.assoc(cohort["plain"], cohort["pheno"], cfg["phenotype"], cfg["outcome"], cfg["binary_order"], cfg["covariates"], all_rows=all_rows, out=f)
        assert out.read_text() == want
        m = subprocess.run([sys.executable, "-m", "inquistr_amd", "assoc", str(cohort["plain"]), "--phenocovar", str(cohort["pheno"]), *flags(cfg), *extra],
                           capture_output=True, text=True, cwd=ROOT)
        assert m.returncode == 0 and m.stdout == want
        # ... and it is the restatement's text: exp() of at most |diff x beta| and |beta| + 1.96 se multiplies a relative error by that much
        ok = np.isin(case.want["status"], (ar.OK, ar.NOT_CONVERGED))
        reach = np.nanmax(np.abs(case.want["beta"][ok]) * (1.0 + np.abs(case.want["max_x"][ok] - case.want["min_x"][ok])) + 1.96 * case.want["se"][ok])
        same_text_within(want, ar.render_text(case.want, ids, cfg["outcome"], cfg["phenotype"], covs, order, all_rows, fmt), case.tol * max(1.0, reach))
        body = want.split("\n")[1:-1]
        if all_rows:  # every locus exactly once
            assert sorted(l.split("\t")[0] for l in body) == sorted(ids) and body[-1].split("\t")[-1] in ar.STATUS_NAMES
        else:
            assert len(body) == int(ok.sum()) == NL - 4
            ps = [float(l.split("\t")[5]) for l in body]
            assert ps == sorted(ps)


def test_chromosome_and_interval_select_what_filtering_the_input_does(cohort):
    cfg = CONFIGS["binary_cov"]
    head, rows = cohort["lines"][0], cohort["lines"][1:]

    def filtered(keep, name):
        p = cohort["dir"] / name
        p.write_text("\n".join([head] + [l for l, c in zip(rows, cohort["coords"]) if keep(c)]) + "\n")
        return p

    base = ["--phenocovar", cohort["pheno"], *flags(cfg), "--all-rows"]
    a = cli(cohort["gz"], *base, "--chr", "chr2").stdout
    b = cli(filtered(lambda c: c[0] == "chr2", "chr2.tsv"), *base).stdout
    assert a == b and len(a.split("\n")) == 20 + 2
    a = cli(cohort["plain"], *base, "--chr", "chr1", "--chr-begin", "3000", "--chr-end", "30040").stdout  # both ends inclusive
    b = cli(filtered(lambda c: c[0] == "chr1" and c[1] >= 3000 and c[2] <= 30040, "interval.tsv"), *base).stdout
    assert a == b and len(a.split("\n")) == 10 + 2
    assert cli(cohort["plain"], *base, "--chr", "chr9").stdout.count("\n") == 1  # no locus: the header alone
