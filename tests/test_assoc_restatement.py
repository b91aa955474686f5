"""Pins the restatement of `inquistr assoc` (tests/assoc_restatement.py), both of its routes, without a GPU: to vectors worked out
by hand (tests/golden/kat_assoc.json) and to scipy as an independent route.  No R exists where this runs, so parity with R's
glm() itself is unpinned."""
import json
import math
import os

import numpy as np
import pytest
from scipy import optimize, stats

from tests import assoc_cases as ac
from tests import assoc_restatement as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "kat_assoc.json")))
ROUTES = ("chol", "qr")


def _f(v):
    return math.nan if v == "NaN" else float(v)


@pytest.mark.parametrize("route", ROUTES)
def test_two_by_two_tables(route):
    """beta = log(ad / bc), se = sqrt(1/a + 1/b + 1/c + 1/d).  The iteration stops once the deviance moves by less than 1e-8 of
    itself; Newton's steps square the error, so beta is then within about 1e-8 of its limit (held to 1e-6).  The standard error is
    taken at the weights of the last weighted least squares, as glm.fit returns them: those belong to the iterate before, which is
    within about sqrt(1e-8) = 1e-4 of the limit, and so is the standard error (held to 1e-4, p to 1e-3)."""
    for t in KAT["tables"]["cases"]:
        a, b, c, d = t["a"], t["b"], t["c"], t["d"]
        x = np.array([1.0] * a + [1.0] * b + [0.0] * c + [0.0] * d)
        y = np.array([1.0] * a + [0.0] * b + [1.0] * c + [0.0] * d)
        row, crit = ar.fit_row(x, x, y, None, "binary", "max", 0.8, route)
        beta, se = math.log(a * d / (b * c)), math.sqrt(1 / a + 1 / b + 1 / c + 1 / d)
        assert row["status"] == ar.OK and crit < 1e-8 and 2 <= row["n_iter"] <= 8
        assert abs(row["beta"] - beta) < 1e-6 * max(1.0, abs(beta)) and abs(row["se"] - se) < 1e-4 * se
        assert abs(row["p"] - math.erfc(abs(beta / se) / math.sqrt(2))) < 1e-3 * row["p"]
        assert (row["n"], row["n_g1"], row["n_g2"]) == (a + b + c + d, b + d, a + c)
        assert row["mean_g2"] == a / (a + c) and row["mean_g1"] == b / (b + d) and (row["min_x"], row["max_x"]) == (0.0, 1.0)


@pytest.mark.parametrize("route", ROUTES)
def test_five_point_least_squares(route):
    o = KAT["ols"]
    x = np.array(o["x"], dtype=np.float64)
    row, _ = ar.fit_row(x, x, np.array(o["y"]), None, "continuous", "min", 0.8, route)
    assert row["status"] == ar.OK and row["n"] == 5 and row["n_iter"] == 0
    for f, v in (("beta", o["beta"]), ("se", o["se"]), ("stat", o["t"]), ("p", o["p"])):
        assert abs(row[f] - v) <= 1e-9 * abs(v), (f, row[f], v)  # the hand arithmetic's own rounding
    assert (row["mean_all"], row["min_x"], row["max_x"]) == (o["mean"], o["min"], o["max"])


def test_predictor_rules():
    for t in KAT["predictor"]["cases"]:
        for mode in ac.MODES:
            got = ar.predictor([_f(t["h1"])], [_f(t["h2"])], mode)[0]
            want = _f(t[mode])
            assert (math.isnan(got) and math.isnan(want)) or got == want, (t, mode)


def test_student_t_against_scipy():
    """the continued fraction against scipy's t distribution, held to 1e-11 relative: the coefficient 1 / B(df / 2, 1 / 2) is a product
    of df / 2 <= 32 766 rounded factors (a random walk of about 180 ulp at worst), the fraction a few hundred more"""
    for df in (1, 2, 3, 7, 30, 266, 1000, 65533):
        for t in (1e-8, 0.01, 0.5, 1.0, 2.0, 5.0, 12.0, 40.0):
            p, q = ar.student_t_two_sided(t, df), 2.0 * stats.t.sf(t, df)
            assert abs(p - q) <= 1e-11 * q, (df, t, p, q)
    assert ar.student_t_two_sided(0.0, 5) == 1.0 and ar.student_t_two_sided(math.inf, 5) == 0.0 and math.isnan(ar.student_t_two_sided(math.nan, 5))


@pytest.mark.parametrize("route", ROUTES)
def test_least_squares_against_linregress(route):
    c = ac.case(11, 40, 128, 0, "continuous", "max")
    rows = c.want if route == "chol" else c.alt
    for i in range(40):
        x = ar.predictor(c.values[i, 0::2], c.values[i, 1::2], "max")
        keep = ~np.isnan(x)
        r = stats.linregress(x[keep], c.y[keep])
        # linregress works from the correlation coefficient; 1e-9 covers its own cancellation at |r| near 0
        assert rows["status"][i] == ar.OK and rows["n"][i] == keep.sum()
        assert abs(rows["beta"][i] - r.slope) <= 1e-9 * abs(r.slope) and abs(rows["se"][i] - r.stderr) <= 1e-9 * r.stderr
        assert abs(rows["p"][i] - r.pvalue) <= 1e-7 * r.pvalue


def _mle(X, y):
    """the logistic maximum-likelihood fit by BFGS, and the inverse Fisher information there"""
    Xc = X.copy()
    Xc[:, 1:] -= Xc[:, 1:].mean(axis=0)
    sd = Xc[:, 1:].std(axis=0)
    Xc[:, 1:] /= sd

    def nll(b):
        eta = Xc @ b
        return float(np.sum(np.logaddexp(0.0, eta) - y * eta))

    def grad(b):
        return Xc.T @ (1.0 / (1.0 + np.exp(-(Xc @ b))) - y)

    r = optimize.minimize(nll, np.zeros(X.shape[1]), jac=grad, method="BFGS", options={"gtol": 1e-10, "maxiter": 2000})
    mu = 1.0 / (1.0 + np.exp(-(Xc @ r.x)))
    cov = np.linalg.inv(Xc.T @ ((mu * (1 - mu))[:, None] * Xc))
    return r.x[1] / sd[0], math.sqrt(cov[1, 1]) / sd[0]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("k", [0, 1, 6])
def test_logistic_and_least_squares_against_scipy_on_200_loci(route, k):
    """200 random loci at p = 2, 3, 8.  BFGS ends where its gradient is below 1e-10, IRLS where the deviance stops moving by 1e-8 of
    itself (beta within about 1e-8, its standard error within about 1e-4, see above): beta is held to 1e-5 of the standard error,
    the standard error to 1e-4, log(p) to 1e-3 (p moves by z^2 = 2 |log p| times what z moves by)."""
    for outcome in ("binary", "continuous"):
        c = ac.case(500 + k, 200, 150, k, outcome, "max")
        rows = c.want if route == "chol" else c.alt
        tested = 0
        for i in range(0, 200, 1 if outcome == "continuous" else 4):  # (every fourth locus through BFGS: it is slow)
            if rows["status"][i] != ar.OK:
                continue
            x = ar.predictor(c.values[i, 0::2], c.values[i, 1::2], "max")
            keep = ~np.isnan(x)
            X = np.column_stack([np.ones(keep.sum()), x[keep]] + [cc[keep] for cc in c.cov])
            if outcome == "binary":
                beta, se = _mle(X, c.y[keep])
                p = 2.0 * stats.norm.sf(abs(beta / se))
            else:
                b, res, _, _ = np.linalg.lstsq(X, c.y[keep], rcond=None)
                df = keep.sum() - X.shape[1]
                se = math.sqrt(float(res[0]) / df * np.linalg.inv(X.T @ X)[1, 1])
                beta, p = b[1], 2.0 * stats.t.sf(abs(b[1] / se), df)
            assert abs(rows["beta"][i] - beta) <= 1e-5 * se, (i, rows["beta"][i], beta, se)
            assert abs(rows["se"][i] - se) <= 1e-4 * se, (i, rows["se"][i], se)
            assert abs(math.log(rows["p"][i]) - math.log(p)) <= 1e-3 * max(1.0, abs(math.log(p))), (i, rows["p"][i], p)
            tested += 1
        assert tested >= 40


def test_every_status_is_reached_and_the_routes_agree():
    """each status by a constructed row (tests/assoc_cases.py); Case() itself asserts that the two routes give the same statuses and
    that at most 2 % of a case's rows end within a factor 100 of the convergence threshold"""
    seen = set()
    for outcome in ("binary", "continuous"):
        for mode in ac.MODES:
            c = ac.special_case(outcome, mode)
            at = {n: i for i, n in enumerate(ac.SPECIAL_NAMES)}
            st = c.want["status"]
            seen.update(int(s) for s in st)
            assert st[at["nan_everywhere"]] == ar.LOW_CALL_RATE and st[at["constant"]] == ar.CONSTANT
            assert st[at["inf_h1"]] == (ar.OK if mode == "min" else ar.SINGULAR)
            assert np.array_equal(c.want["n_iter"], c.alt["n_iter"])
            if outcome == "binary":
                # complete separation: the deviance falls by 1 / e a step and 25 steps do not bring its change under 1e-8 of it
                assert st[at["one_group"]] == ar.ONE_GROUP and st[at["separated"]] == ar.NOT_CONVERGED and c.want["n_iter"][at["separated"]] == 25
                # quasi-complete: whichever way the 25-step rule decides, both routes decide the same, and the standard error is huge
                q = at["quasi_separated"]
                assert st[q] in (ar.OK, ar.NOT_CONVERGED) and c.alt["status"][q] == st[q] and c.want["se"][q] > 100.0
    for outcome in ("binary", "continuous"):
        for noise in (0.0, 1e-9):
            assert ac.collinear_case(outcome, noise).want["status"][0] == ar.SINGULAR
    y = np.array([0.0, 1.0, 0.0, 1.0])
    row, _ = ar.fit_row([1, 2, 3, 4], [1, 2, 3, 4], y, np.ones((2, 4)), "binary")
    seen.add(row["status"])
    assert row["status"] == ar.TOO_FEW  # N = 4 = p
    assert seen == set(range(7))


def test_centring_keeps_lengths_near_10000_conditioned():
    """the same row shifted by 10 000: beta and its standard error do not move (the shift is a reparametrisation)"""
    rng = np.random.default_rng(5)
    y = (rng.random(200) < 0.5).astype(np.float64)
    x = rng.integers(0, 3, 200) + y * (rng.random(200) < 0.5)
    for outcome, yy in (("binary", y), ("continuous", x * 0.3 + rng.normal(size=200))):
        a, _ = ar.fit_row(x, x, yy, None, outcome, "max", 0.8, "chol")
        b, _ = ar.fit_row(x + 10000.0, x + 10000.0, yy, None, outcome, "max", 0.8, "chol")
        assert a["status"] == b["status"] == ar.OK and a["n_iter"] == b["n_iter"]
        assert abs(a["beta"] - b["beta"]) <= 1e-11 * abs(a["beta"]) and abs(a["se"] - b["se"]) <= 1e-11 * a["se"]
