"""Firth's penalised logistic regression on the GPU through the C ABI (inq_assoc_rows_firth) against the restatement
(tests/firth_restatement.py, pinned without a GPU by tests/test_firth_restatement.py), on the shapes of tests/test_gpu_assoc.py.

Exact: statuses, which rows are fitted, the bytes of rows[] (those of inq_assoc_rows) and both iteration counts - those except on
rows where the last or the last-but-one criterion of either fit lies within 1 % of 1e-9, at most 2 % of a case (asserted when the
case is built, tests/firth_cases.py).  beta, se, chi2, log(p) and both l* are held, per case, to 10 x the largest relative
disagreement of the restatement's QR route and its Cholesky route on that same input, never below 64 * 2^-52: the rule of
tests/test_gpu_assoc.py, the factor covering the wave's order of summation, which is neither route's.  Every test prints the share
of the tolerance it used.  compare() also holds every fitted row to a tolerance of its own against a long-double fit of the same
iteration, chi2 at the scale of l* (tests/assoc_reference.py), and p to the host's erfc of the device's own chi2."""
import json
import math
import os

import numpy as np
import pytest

from inquistr_amd import hipcall
from tests import assoc_cases as ac
from tests import assoc_restatement as ar
from tests import firth_cases as fc
from tests import firth_restatement as fr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    c = hipcall.Context(0)
    yield c
    c.close()


def check(ctx, c, whens=fc.WHENS):
    ordinary = ctx.assoc_rows(c.values, c.y, c.cov, "binary", c.mode, c.cutoff)
    out = {}
    for when in whens:
        rows, firth = ctx.assoc_rows_firth(c.values, c.y, c.cov, c.mode, c.cutoff, when)
        fc.compare(c, when, rows, firth, ordinary)
        out[when] = firth
    return out


@pytest.mark.parametrize("ns", [3, 63, 64, 65, 127, 128, 129, 300])
def test_sample_counts_at_lane_and_stride_boundaries(ctx, ns):
    """one sample short of, at and one past one and two steps of a wave; k and the mode go round with ns"""
    check(ctx, fc.case(ns, 24, ns, [0, 1, 6][ns % 3], ac.MODES[ns % 3]))


@pytest.mark.parametrize("n_rows", [1, 3, 4, 5, 257])
def test_row_counts_around_a_workgroup(ctx, n_rows):
    """four rows to a workgroup: a part of one, exactly one, one row more, and 64 workgroups and a row"""
    check(ctx, fc.case(1000 + n_rows, n_rows, 65, 1, "max"))


@pytest.mark.parametrize("k", [0, 1, 2, 3, 4, 5, 6])
def test_every_column_count(ctx, k):
    """one kernel instantiation per p = 2 + k: all seven, the mode going round"""
    check(ctx, fc.case(2000 + k, 16, 129, k, ac.MODES[k % 3]))


@pytest.mark.parametrize("n_rows", [7, 8, 9, 17])
def test_tiles(ctx, n_rows):
    """rows go up tile by tile ("assoc_tile_rows" = 8 here): the same bytes as in one piece, in both outputs"""
    c = fc.case(3000 + n_rows, n_rows, 70, 2, "mean")
    whole = ctx.assoc_rows_firth(c.values, c.y, c.cov, c.mode, c.cutoff, "always")
    ctx.set_option("assoc_tile_rows", 8)
    try:
        tiled = ctx.assoc_rows_firth(c.values, c.y, c.cov, c.mode, c.cutoff, "always")
    finally:
        ctx.set_option("assoc_tile_rows", 0)
    assert tiled[0].tobytes() == whole[0].tobytes() and tiled[1].tobytes() == whole[1].tobytes()
    fc.compare(c, "always", tiled[0], tiled[1], ctx.assoc_rows(c.values, c.y, c.cov, "binary", c.mode, c.cutoff))


@pytest.mark.parametrize("mode", ac.MODES)
def test_constructed_rows(ctx, mode):
    """assoc_cases.special_case's rows: NaNs in lane 0, in lane 63, in the last sample, in one haplotype only; separation, which
    now ends OK with a finite estimate; every filter, whose rows are never fitted.  Under FALLBACK the fitted set is the
    restatement's (compare() asserts it): the separated rows and no ordinary one."""
    c = fc.special_case(mode)
    at = {n: i for i, n in enumerate(ac.SPECIAL_NAMES)}
    got = check(ctx, c)
    o = c.R.ordinary["status"]
    for when in fc.WHENS:
        f = got[when]
        for name in ("separated", "quasi_separated"):
            r = f[at[name]]
            assert r["status"] == fr.OK and math.isfinite(r["beta"]) and r["se"] < 10.0 and r["p"] < 1e-20, (name, r)
        for name in ("nan_everywhere", "low_call_rate", "constant", "one_group"):
            assert o[at[name]] not in (ar.OK, ar.NOT_CONVERGED) and f["status"][at[name]] == fr.NOT_FITTED, name
            assert np.isnan(f["beta"][at[name]]) and np.isnan(f["p"][at[name]]) and f["n_iter_full"][at[name]] == 0
    assert o[at["separated"]] == ar.NOT_CONVERGED and c.R.min_mu[at["quasi_separated"]] < 1e-7
    fitted = got["fallback"]["status"] != fr.NOT_FITTED
    assert fitted[at["separated"]] and fitted[at["quasi_separated"]] and not fitted[at["nan_lane0"]] and fitted.sum() < 10
    always = got["always"]["status"] != fr.NOT_FITTED
    assert always[at["nan_lane0"]] and always[at["nan_lane63"]] and always[at["nan_last"]] and always[at["nan_one_haplotype"]]
    # the bound is an option: with 0.5 every fitted row's smallest min(mu, 1 - mu) is below it, and FALLBACK fits what ALWAYS fits
    ctx.set_option("assoc_firth_mu_ppb", 500_000_000)
    try:
        _, wide = ctx.assoc_rows_firth(c.values, c.y, c.cov, c.mode, c.cutoff, "fallback")
    finally:
        ctx.set_option("assoc_firth_mu_ppb", 1000)
    assert wide.tobytes() == got["always"].tobytes()


def test_too_few_samples_is_not_fitted(ctx):
    """TOO_FEW, the one filter special_case has no row for: 3 samples against p = 3"""
    rng = np.random.default_rng(5)
    v = rng.integers(5, 20, (4, 6)).astype(np.float32)
    rows, firth = ctx.assoc_rows_firth(v, np.array([0.0, 1.0, 1.0]), np.array([[0.5, 0.1, 0.9]]), "max", 0.8, "always")
    assert (rows["status"] == ar.TOO_FEW).all() and (firth["status"] == fr.NOT_FITTED).all() and np.isnan(firth["chi2"]).all()


def test_a_collinear_covariate_is_singular(ctx):
    c = fc.collinear_case()
    assert c.R.ordinary["status"][0] in (ar.OK, ar.NOT_CONVERGED) and c.R.chol["status"][0] == fr.SINGULAR
    assert (c.R.chol["status"][1:] == fr.OK).all()
    got = check(ctx, c, ("always",))["always"]
    assert got["status"][0] == fr.SINGULAR and np.isnan(got["beta"][0]) and np.isnan(got["pll_full"][0]) and got["n_iter_full"][0] == 0
    # a covariate that IS x stops the ordinary fit, and Firth's is not tried
    a = ac.collinear_case("binary", 0.0)
    rows, firth = ctx.assoc_rows_firth(a.values, a.y, a.cov, "max", 0.8, "always")
    assert rows["status"][0] == ar.SINGULAR and firth["status"][0] == fr.NOT_FITTED and (firth["status"][1:] == fr.OK).all()


def test_hand_derived_vectors(ctx):
    """The 2 x 2 closed form (tests/golden/kat_firth.json), zero cells included.  The iteration stops when a step is below 1e-9
    standard errors and each step is a fixed fraction r of the one before, so r / (1 - r) of the last step is left: beta is held to
    1e-7 standard errors (r up to 0.99), the standard error, a smooth function of beta, to 1e-7 of itself; the bounds of
    tests/test_firth_restatement.py"""
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "kat_firth.json")))
    for t in kat["tables"]["cases"]:
        a, b, c, d = t["a"], t["b"], t["c"], t["d"]
        x = np.array([1.0] * a + [1.0] * b + [0.0] * c + [0.0] * d)
        y = np.array([1.0] * a + [0.0] * b + [1.0] * c + [0.0] * d)
        _, firth = ctx.assoc_rows_firth(np.repeat(x, 2)[None, :].astype(np.float32), y, None, "mean", 0.8, "always")
        got = firth[0]
        beta = math.log((a + 0.5) * (d + 0.5) / ((b + 0.5) * (c + 0.5)))
        p1, p0 = (a + 0.5) / (a + b + 1), (c + 0.5) / (c + d + 1)
        se = math.sqrt(1 / ((a + b) * p1 * (1 - p1)) + 1 / ((c + d) * p0 * (1 - p0)))
        assert got["status"] == fr.OK and abs(got["beta"] - beta) < 1e-7 * se and abs(got["se"] - se) < 1e-7 * se, (t, got)
        assert got["p"] == math.erfc(math.sqrt(got["chi2"] / 2)) or abs(got["p"] - math.erfc(math.sqrt(got["chi2"] / 2))) < 1e-14 * got["p"]
        if (a, b, c, d) == (1, 1, 1, 1):
            assert got["beta"] == 0.0 and got["chi2"] < 1e-12 and got["n_iter_full"] == 0


def test_arguments(ctx):
    L, h = ctx._L, ctx._h
    rows = np.zeros(4, dtype=hipcall.ASSOC_ROW_DTYPE)
    firth = np.zeros(4, dtype=hipcall.ASSOC_FIRTH_ROW_DTYPE)
    v = np.zeros((4, 8), dtype=np.float32)
    y = np.array([0.0, 1.0, 0.0, 1.0])
    cov = np.zeros((7, 4))
    call = lambda n_rows, ns, yy, k, mode, cut, when: L.inq_assoc_rows_firth(h, v.ctypes.data, n_rows, ns, yy.ctypes.data, cov.ctypes.data, k, mode, cut,
                                                                             when, rows.ctypes.data, firth.ctypes.data)
    assert call(0, 4, y, 0, 0, 0.8, 1) == 0  # no rows: nothing to do
    assert call(4, 4, y, 0, 0, 0.8, 0) == -1 and call(4, 4, y, 0, 0, 0.8, 3) == -1 and call(0, 4, y, 0, 0, 0.8, -1) == -1  # a bad `when`
    assert call(4, 4, y, 7, 0, 0.8, 1) == -1 and call(4, 65536, y, 0, 0, 0.8, 1) == -1  # the limits, before any launch
    assert call(4, 4, y, 0, 3, 0.8, 2) == -1 and call(4, 4, y, 0, 0, float("nan"), 2) == -1
    assert call(4, 4, np.array([0.0, 1.0, 2.0, 1.0]), 0, 0, 0.8, 2) == -1  # the outcome is binary: 0 or 1
    assert L.inq_assoc_rows_firth(h, v.ctypes.data, 4, 4, y.ctypes.data, None, 0, 0, 0.8, 1, rows.ctypes.data, None) == -1
    assert L.inq_assoc_rows_firth(h, None, 4, 4, y.ctypes.data, None, 0, 0, 0.8, 1, rows.ctypes.data, firth.ctypes.data) == -1
    assert ctx._L.inq_ctx_set_option(h, b"assoc_firth_mu_ppb", -1) == hipcall.INQ_ERR_ARG
    assert call(4, 4, y, 0, 0, 0.8, 2) == 0 and (firth["status"] == fr.NOT_FITTED).all()  # all zeros: every row is CONSTANT
