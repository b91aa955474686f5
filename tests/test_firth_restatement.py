"""Pins the restatement of Firth's penalised logistic regression (tests/firth_restatement.py), both of its routes, without a GPU:
to the 2 x 2 closed form (tests/golden/kat_firth.json), to scipy.optimize maximising the penalised likelihood as an independent
route, to scipy's chi-square tail, to the invariances the model has, and the fallback rule to rows built for each of its branches.
No logistf exists where this runs, so parity with it is unpinned."""
import json
import math
import os

import numpy as np
import pytest
from scipy import optimize, stats

from tests import assoc_cases as ac
from tests import assoc_restatement as ar
from tests import firth_cases as fc
from tests import firth_restatement as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "kat_firth.json")))
ROUTES = ("chol", "qr")


def _table(t):
    a, b, c, d = t["a"], t["b"], t["c"], t["d"]
    x = np.array([1.0] * a + [1.0] * b + [0.0] * c + [0.0] * d)
    y = np.array([1.0] * a + [0.0] * b + [1.0] * c + [0.0] * d)
    return (a, b, c, d), x, y


@pytest.mark.parametrize("route", ROUTES)
def test_two_by_two_tables(route):
    """beta = log((a + 1/2)(d + 1/2) / ((b + 1/2)(c + 1/2))), zero cells included, and the standard error at the fitted
    probabilities.  The iteration stops when a step is below 1e-9 standard errors; convergence is linear, each step a fixed fraction
    r of the one before, so r / (1 - r) of the last step is left: beta is held to 1e-7 standard errors (r up to 0.99), the standard
    error, a smooth function of beta, to 1e-7 of itself."""
    for t in KAT["tables"]["cases"]:
        (a, b, c, d), x, y = _table(t)
        row, fits = fr.fit_row(x, x, y, None, "max", route)
        beta = math.log((a + 0.5) * (d + 0.5) / ((b + 0.5) * (c + 0.5)))
        p1, p0 = (a + 0.5) / (a + b + 1), (c + 0.5) / (c + d + 1)
        se = math.sqrt(1 / ((a + b) * p1 * (1 - p1)) + 1 / ((c + d) * p0 * (1 - p0)))
        assert row["status"] == fr.OK and fits[0]["crits"][-1] < 1e-9 and row["n_iter_full"] <= 30
        assert abs(row["beta"] - beta) < 1e-7 * se and abs(row["se"] - se) < 1e-7 * se, (t, row)
        # the null fit: one pi for everybody, the hat values still those of both columns and summing to 2, so the intercept's
        # modified score (a + c) - n pi + 2 (1/2 - pi) = 0 gives pi = (a + c + 1) / (n + 2)
        n, pn = a + b + c + d, (a + c + 1) / (a + b + c + d + 2)
        ll0 = (a + c) * math.log(pn) + (b + d) * math.log(1 - pn)
        I0 = np.array([[n, a + b], [a + b, a + b]]) * pn * (1 - pn)
        assert abs(row["pll_null"] - (ll0 + 0.5 * math.log(np.linalg.det(I0)))) < 1e-12 * abs(row["pll_null"]) + 1e-12
        if (a, b, c, d) == (1, 1, 1, 1):
            assert abs(row["beta"]) < 1e-14 and row["chi2"] < 1e-12 and row["p"] > 1 - 1e-6


def _pll(X, y, beta):
    pi = 1.0 / (1.0 + np.exp(-(X @ beta)))
    w = pi * (1.0 - pi)
    return float((y * np.log(pi) + (1 - y) * np.log(1 - pi)).sum() + 0.5 * np.linalg.slogdet(X.T @ (w[:, None] * X))[1])


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("k", [0, 1, 3])
def test_against_scipy_optimize(route, k):
    """scipy maximises l* itself, over all coefficients and over all but x's: the fixed points of both fits, by a route that shares
    nothing with the restatement's steps (no hat values, no modified score).  BFGS ends with a gradient below 1e-9; the curvature
    of l* is about the information, so its beta is within about 1e-9 standard errors ... held to 1e-6 of one, l* (flat there) to
    1e-9 absolute."""
    c = fc.case(40 + k, 6, 40, k, "max")
    for i in range(6):
        v = c.values[i]
        ys, X, Xc = fr.columns(v[0::2], v[1::2], c.y, c.cov, "max")
        sd = np.concatenate([[1.0], Xc[:, 1:].std(axis=0)])
        Z = Xc / sd  # unit columns for the optimiser; l* moves by the constant sum log sd
        shift = float(np.log(sd).sum())
        row, fits = fr.fit_row(v[0::2], v[1::2], c.y, c.cov, "max", route)
        assert row["status"] == fr.OK
        full = optimize.minimize(lambda b: -_pll(Z, ys, b), np.zeros(2 + k), method="BFGS", options={"gtol": 1e-10})
        null = optimize.minimize(lambda b: -_pll(Z, ys, np.concatenate([b, [0.0]])), np.zeros(1 + k), method="BFGS", options={"gtol": 1e-10})
        assert abs(full.x[-1] / sd[-1] - row["beta"]) < 1e-6 * row["se"], (i, full.x[-1] / sd[-1], row["beta"])
        assert abs(-full.fun + shift - row["pll_full"]) < 1e-9 and abs(-null.fun + shift - row["pll_null"]) < 1e-9
        assert abs(2 * (null.fun - full.fun) - row["chi2"]) < 1e-8
        # the standard error is the inverse information's corner there
        pi = 1.0 / (1.0 + np.exp(-(Z @ full.x)))
        inv = np.linalg.inv(Z.T @ ((pi * (1 - pi))[:, None] * Z))
        assert abs(math.sqrt(inv[-1, -1]) / sd[-1] - row["se"]) < 1e-6 * row["se"]


def test_p_is_the_chi_square_tail():
    for chi2 in (0.0, 1e-12, 0.01, 1.0, 3.841458820694124, 30.0, 148.0, 1400.0):
        p, q = math.erfc(math.sqrt(chi2 * 0.5)), stats.chi2.sf(chi2, 1)
        assert abs(p - q) <= 1e-13 * q, (chi2, p, q)
    c = fc.special_case("max")
    fitted = c.R.chol["status"] == fr.OK
    assert fitted.sum() > 100
    q = stats.chi2.sf(c.R.chol["chi2"][fitted], 1)
    assert np.all(np.abs(c.R.chol["p"][fitted] - q) <= 1e-13 * q)


@pytest.mark.parametrize("route", ROUTES)
def test_shifting_and_scaling_x_changes_neither_chi2_nor_beta_over_se(route):
    """x -> 4 x + 1000 (exact in f32 for these lengths): beta and se divide by 4, chi2 and the iteration counts stay.  Held to 1e-9:
    the shift costs the uncentred route three digits of its thirteen"""
    c = fc.case(7, 8, 50, 1, "max")
    for i in range(8):
        v = c.values[i]
        a, _ = fr.fit_row(v[0::2], v[1::2], c.y, c.cov, "max", route)
        b, _ = fr.fit_row(4 * v[0::2] + 1000, 4 * v[1::2] + 1000, c.y, c.cov, "max", route)
        assert a["status"] == b["status"] == fr.OK and (a["n_iter_full"], a["n_iter_null"]) == (b["n_iter_full"], b["n_iter_null"])
        assert abs(a["beta"] / a["se"] - b["beta"] / b["se"]) <= 1e-9 * abs(a["beta"] / a["se"]) + 1e-12
        assert abs(a["beta"] - 4 * b["beta"]) <= 1e-9 * abs(a["beta"]) + 1e-12
        assert abs(a["chi2"] - b["chi2"]) <= 1e-9 * a["chi2"] + 1e-10


def test_the_two_routes_agree():
    """on every decision and every count (Case asserts it), and to a few hundred ulp on the ordinary rows' numbers"""
    c = fc.case(2003, 16, 129, 3, "max")
    assert (c.R.chol["status"] == fr.OK).all() and not c.skip.any()
    assert fr.disagreement(c.R.chol, c.R.qr) < 1e-9


def test_fallback_rule_on_rows_built_for_each_branch():
    c = fc.special_case("max")
    at = {n: i for i, n in enumerate(ac.SPECIAL_NAMES)}
    o, m = c.R.ordinary["status"], c.R.min_mu
    fb, al = c.R.fitted("fallback"), c.R.fitted("always")
    # NOT_CONVERGED: fitted whatever mu is
    assert o[at["separated"]] == ar.NOT_CONVERGED and fb[at["separated"]] and al[at["separated"]]
    # stopped on the deviance with a fitted probability below the bound: OK, and fitted
    assert o[at["quasi_separated"]] == ar.OK and c.R.ordinary["se"][at["quasi_separated"]] > 100 and m[at["quasi_separated"]] < 1e-6
    assert fb[at["quasi_separated"]]
    # an ordinary row: OK, mu well inside, ALWAYS only
    assert o[at["two_values"]] == ar.OK and m[at["two_values"]] > 1e-3 and al[at["two_values"]] and not fb[at["two_values"]]
    # stopped by a filter, or SINGULAR: never
    for name in ("nan_everywhere", "low_call_rate", "constant", "one_group", "inf_h1", "inf_both"):
        assert o[at[name]] in (ar.LOW_CALL_RATE, ar.CONSTANT, ar.ONE_GROUP, ar.SINGULAR) and not al[at[name]] and not fb[at[name]], name
        assert c.R.chol["status"][at[name]] == fr.NOT_FITTED and math.isnan(m[at[name]])
    assert fb.sum() == 2 and al.sum() == (np.isin(o, (ar.OK, ar.NOT_CONVERGED))).sum()
    # the bound moves the set: at 0.5 every fitted row is below it
    assert np.array_equal(c.R.fitted("fallback", 0.5), al)
    assert fr.selected("fallback", ar.OK, 9e-7) and not fr.selected("fallback", ar.OK, 1e-6) and not fr.selected("always", ar.TOO_FEW, 0.0)
    # what separation does to the two fits: the ordinary one's estimate runs away, Firth's stays
    for name in ("separated", "quasi_separated"):
        r = c.R.chol[at[name]]
        assert r["status"] == fr.OK and r["se"] < 10 and abs(r["beta"]) < 10 and r["p"] < 1e-20
