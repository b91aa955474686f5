"""Pins tests/assoc_reference.py without a GPU: the long-double reference to the closed forms of tests/golden and to a 40-digit mpmath
run of the same iterations, its decisions to the f64 restatement's on every case the GPU tests use; the per-row rule of
assoc_cases.compare / firth_cases.compare with the wave-order route in the device's place on every such case; and the host's
p-value functions, which the GPU tests hold the device's to, against mpmath."""
import json
import math
import os

import mpmath
import numpy as np
import pytest

from tests import assoc_cases as ac
from tests import assoc_reference as rf
from tests import assoc_restatement as ar
from tests import firth_cases as fc
from tests import firth_restatement as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


def _table(t):
    a, b, c, d = t["a"], t["b"], t["c"], t["d"]
    x = np.array([1.0] * a + [1.0] * b + [0.0] * c + [0.0] * d)
    y = np.array([1.0] * a + [0.0] * b + [1.0] * c + [0.0] * d)
    return (a, b, c, d), x, y


@pytest.mark.parametrize("arith", [rf.REFERENCE, rf.WAVE], ids=lambda a: a.name)
def test_closed_forms(arith):
    """the bounds of tests/test_assoc_restatement.py and tests/test_firth_restatement.py, where they are derived"""
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "kat_assoc.json")))
    for t in kat["tables"]["cases"]:
        (a, b, c, d), x, y = _table(t)
        row, _ = rf.fit_row(arith, x, x, y, None, "binary", "mean")
        beta, se = math.log(a * d / (b * c)), math.sqrt(1 / a + 1 / b + 1 / c + 1 / d)
        assert row["status"] == ar.OK and abs(row["beta"] - beta) < 1e-6 * max(1.0, abs(beta)) and abs(row["se"] - se) < 1e-4 * se
        assert (row["n"], row["n_g1"], row["n_g2"]) == (a + b + c + d, b + d, a + c)
        assert row["mean_g2"] == arith.dtype(a) / (a + c) and row["mean_g1"] == arith.dtype(b) / (b + d)
    o = kat["ols"]
    row, _ = rf.fit_row(arith, o["x"], o["x"], np.array(o["y"]), None, "continuous", "max")
    assert row["status"] == ar.OK and row["n"] == 5 and row["n_iter"] == 0
    for f, v in (("beta", o["beta"]), ("se", o["se"]), ("stat", o["t"]), ("p", o["p"])):
        assert abs(float(row[f]) - v) <= 1e-9 * abs(v), (f, row[f], v)
    assert (row["mean_all"], row["min_x"], row["max_x"]) == (o["mean"], o["min"], o["max"])
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "kat_firth.json")))
    for t in kat["tables"]["cases"]:
        (a, b, c, d), x, y = _table(t)
        row = rf.firth_fit_row(arith, x, x, y, None, "max")
        beta = math.log((a + 0.5) * (d + 0.5) / ((b + 0.5) * (c + 0.5)))
        p1, p0 = (a + 0.5) / (a + b + 1), (c + 0.5) / (c + d + 1)
        se = math.sqrt(1 / ((a + b) * p1 * (1 - p1)) + 1 / ((c + d) * p0 * (1 - p0)))
        assert row["status"] == fr.OK and abs(row["beta"] - beta) < 1e-7 * se and abs(row["se"] - se) < 1e-7 * se, (t, row)
        n, pn = a + b + c + d, (a + c + 1) / (a + b + c + d + 2)  # the null fit's closed form, as test_firth_restatement has it
        ll0 = (a + c) * math.log(pn) + (b + d) * math.log(1 - pn)
        I0 = np.array([[n, a + b], [a + b, a + b]]) * pn * (1 - pn)
        assert abs(float(row["pll_null"]) - (ll0 + 0.5 * math.log(np.linalg.det(I0)))) < 1e-12 * abs(float(row["pll_null"])) + 1e-12
        if (a, b, c, d) == (1, 1, 1, 1):
            assert abs(row["beta"]) < 1e-14 and row["chi2"] < 1e-12


def test_the_wave_sum_is_the_kernels_order():
    """lane l adds its samples in ascending order, the butterfly pairs lanes xor 1, 2, ... 32; a sample that is left out keeps its lane"""
    rng = np.random.default_rng(3)
    for ns in (1, 63, 64, 65, 200):
        idx = np.nonzero(rng.random(ns) < 0.8)[0] if ns > 1 else np.array([0])
        a = rng.normal(size=(len(idx), 3)) * 10.0 ** rng.integers(-8, 8, (len(idx), 3))
        lanes = [np.zeros(3) for _ in range(64)]
        for i, row in zip(idx.tolist(), a):
            lanes[i % 64] = lanes[i % 64] + row
        d = 1
        while d < 64:
            lanes = [lanes[l] + lanes[l ^ d] for l in range(64)]
            d *= 2
        assert all(np.array_equal(lanes[0], lanes[l]) for l in range(64))  # the same bits in every lane
        assert np.array_equal(rf.wave_sum(a, idx), lanes[0])
        assert np.array_equal(rf.wave_sum(a[:, 0], idx), lanes[0][0])


# ---- the same iterations in mpmath at 40 digits ------------------------------------------------------------------------------------

def _mp_chol(M):
    p = len(M)
    L = [[mpmath.mpf(0)] * p for _ in range(p)]
    for j in range(p):
        L[j][j] = mpmath.sqrt(M[j][j] - sum(L[j][k] ** 2 for k in range(j)))
        for i in range(j + 1, p):
            L[i][j] = (M[i][j] - sum(L[i][k] * L[j][k] for k in range(j))) / L[j][j]
    return L


def _mp_forward(L, r):
    v = []
    for i in range(len(r)):
        v.append((r[i] - sum(L[i][k] * v[k] for k in range(i))) / L[i][i])
    return v


def _mp_backward(L, v):
    v = list(v)
    for i in range(len(v) - 1, -1, -1):
        v[i] = (v[i] - sum(L[k][i] * v[k] for k in range(i + 1, len(v)))) / L[i][i]
    return v


def _mp_columns(x, cov, x_last):
    mp = mpmath.mpf
    n = len(x)
    centre = lambda c: [mp(float(v)) - sum(mp(float(u)) for u in c) / n for v in c]
    cols = [centre(c) for c in cov]
    cols = cols + [centre(x)] if x_last else [centre(x)] + cols
    return [[mp(1)] + [c[i] for c in cols] for i in range(n)]  # rows


def _mp_gram(X, w):
    p = len(X[0])
    return [[sum(wi * r[i] * r[j] for wi, r in zip(w, X)) for j in range(p)] for i in range(p)]


def _mp_ordinary(x, y, cov, binary):
    """-> beta_x, se, n_iter"""
    mp = mpmath.mpf
    X = _mp_columns(x, cov, False)
    n, p = len(X), len(X[0])
    y = [mp(float(v)) for v in y]
    e1 = [mp(int(j == 1)) for j in range(p)]
    if not binary:
        L = _mp_chol(_mp_gram(X, [mp(1)] * n))
        beta = _mp_backward(L, _mp_forward(L, [sum(r[j] * yi for r, yi in zip(X, y)) for j in range(p)]))
        rss = sum((yi - sum(b * v for b, v in zip(beta, r))) ** 2 for r, yi in zip(X, y))
        return beta[1], mpmath.sqrt(rss / (n - p) * _mp_backward(L, _mp_forward(L, e1))[1]), 0
    eps = mp(2) ** -52
    beta, dev_old = None, mp(0)
    for t in range(ar.MAX_ITER + 1):
        if t == 0:
            mu = [(yi + mp(0.5)) * mp(0.5) for yi in y]
            eta = [mpmath.log(m / (1 - m)) for m in mu]
        else:
            eta = [sum(b * v for b, v in zip(beta, r)) for r in X]
            mu = [min(max(1 / (1 + mpmath.exp(-e)), eps), 1 - eps) for e in eta]
        dev = sum(-2 * mpmath.log(m if yi != 0 else 1 - m) for m, yi in zip(mu, y))
        if t >= 1 and (abs(dev - dev_old) / (abs(dev) + mp(0.1)) < mp(ar.CONVERGED) or t == ar.MAX_ITER):
            return beta[1], mpmath.sqrt(inv_xx), t
        dev_old = dev
        w = [m * (1 - m) for m in mu]
        z = [e + (yi - m) / wi for e, yi, m, wi in zip(eta, y, mu, w)]
        L = _mp_chol(_mp_gram(X, w))
        beta = _mp_backward(L, _mp_forward(L, [sum(wi * r[j] * zi for wi, r, zi in zip(w, X, z)) for j in range(p)]))
        inv_xx = _mp_backward(L, _mp_forward(L, e1))[1]


def _mp_firth(x, y, cov, null):
    """-> beta_x, se, l*, n_iter"""
    mp = mpmath.mpf
    X = _mp_columns(x, cov, True)
    n, p = len(X), len(X[0])
    y = [mp(float(v)) for v in y]
    eps = mp(2) ** -52
    beta = [mp(0)] * p
    for t in range(fr.MAX_ITER + 1):
        pi = [min(max(1 / (1 + mpmath.exp(-sum(b * v for b, v in zip(beta, r)))), eps), 1 - eps) for r in X]
        w = [q * (1 - q) for q in pi]
        M = _mp_gram(X, w)
        L = _mp_chol(M)
        pll = sum(mpmath.log(q if yi != 0 else 1 - q) for q, yi in zip(pi, y)) + sum(mpmath.log(L[j][j]) for j in range(p))
        h = [wi * sum(u * u for u in _mp_forward(L, r)) for wi, r in zip(w, X)]
        U = [sum(((yi - q) + hi * (mp(0.5) - q)) * r[j] for yi, q, hi, r in zip(y, pi, h, X)) for j in range(p)]
        v = _mp_forward(L, U)
        if null:
            v[p - 1] = mp(0)
        delta = _mp_backward(L, v)
        big = max(abs(d) for d in delta)
        if max(abs(d) * mpmath.sqrt(M[j][j]) for j, d in enumerate(delta)) < mp(fr.CONVERGED) or t == fr.MAX_ITER:
            return beta[p - 1], 1 / L[p - 1][p - 1], pll, t
        scale = mp(fr.MAX_STEP) / big if big > fr.MAX_STEP else mp(1)
        beta = [b + d * scale for b, d in zip(beta, delta)]


def _mp_rows(seed):
    """12 samples, one covariate, no missing value; x with an effect so that beta is no small difference"""
    rng = np.random.default_rng(seed)
    yb = np.array([0.0, 1.0] * 6)
    rng.shuffle(yb)
    yc = np.round(rng.normal(50.0, 10.0, 12), 3)
    cov = np.round(rng.normal(0.0, 1.0, (1, 12)), 4)
    noise = rng.integers(-3, 4, 12).astype(np.float64)
    return yb, yc, cov, 20.0 + noise + 2.0 * yb, 20.0 + noise + np.round((yc - 50.0) / 5.0)


def _rel(got, want):
    return float(abs(mpmath.mpf(float(got)) + mpmath.mpf(float(LD(got) - LD(float(got)))) - want) / abs(want))


@pytest.mark.parametrize("seed", [11, 12])
def test_the_reference_against_mpmath(seed):
    """Six rows in all, two per model: beta, se and both l* within 1e-17 relative of the same iteration at 40 digits, the step
    counts equal.  (A long double goes into mpmath exactly as its f64 head plus the rest.)"""
    yb, yc, cov, xb, xc = _mp_rows(seed)
    with mpmath.workdps(40):
        row, _ = rf.fit_row(rf.REFERENCE, xb, xb, yb, cov, "binary", "max")
        beta, se, steps = _mp_ordinary(xb, yb, cov, True)
        assert row["status"] == ar.OK and row["n_iter"] == steps
        print(f"binary: beta {_rel(row['beta'], beta):.1e} se {_rel(row['se'], se):.1e} steps {steps}")
        assert _rel(row["beta"], beta) <= 1e-17 and _rel(row["se"], se) <= 1e-17
        row, _ = rf.fit_row(rf.REFERENCE, xc, xc, yc, cov, "continuous", "max")
        beta, se, _ = _mp_ordinary(xc, yc, cov, False)
        print(f"continuous: beta {_rel(row['beta'], beta):.1e} se {_rel(row['se'], se):.1e}")
        assert row["status"] == ar.OK and _rel(row["beta"], beta) <= 1e-17 and _rel(row["se"], se) <= 1e-17
        row = rf.firth_fit_row(rf.REFERENCE, xb, xb, yb, cov, "max")
        beta, se, pll_full, steps_full = _mp_firth(xb, yb, cov, False)
        _, _, pll_null, steps_null = _mp_firth(xb, yb, cov, True)
        assert row["status"] == fr.OK and (row["n_iter_full"], row["n_iter_null"]) == (steps_full, steps_null)
        each = [_rel(row["beta"], beta), _rel(row["se"], se), _rel(row["pll_full"], pll_full), _rel(row["pll_null"], pll_null)]
        print("firth: beta %.1e se %.1e l*_full %.1e l*_null %.1e" % tuple(each), "steps", steps_full, steps_null)
        assert max(each) <= 1e-17


# ---- every case the GPU tests use ----------------------------------------------------------------------------------------------

def _ordinary_cases():
    for o in ("binary", "continuous"):
        for ns in (2, 3, 63, 64, 65, 127, 128, 129, 300):
            yield f"ns {ns} {o}", ac.case(ns, 24, ns, [0, 1, 6][ns % 3], o, ac.MODES[ns % 3])
        for n_rows in (1, 3, 4, 5, 257):
            yield f"rows {n_rows} {o}", ac.case(1000 + n_rows, n_rows, 65, 1, o, "max")
        for mode in ac.MODES:
            for k in range(7):
                yield f"k {k} {mode} {o}", ac.case(2000 + k, 16, 129, k, o, mode)
            yield f"special {mode} {o}", ac.special_case(o, mode)
        for n_rows in (7, 8, 9, 17):
            yield f"tiles {n_rows} {o}", ac.case(3000 + n_rows, n_rows, 70, 2, o, "mean")
        for noise in (0.0, 1e-9):
            yield f"collinear {noise} {o}", ac.collinear_case(o, noise)
    yield from ac.edge_cases()


def _firth_cases():
    for ns in (3, 63, 64, 65, 127, 128, 129, 300):
        yield f"ns {ns}", fc.case(ns, 24, ns, [0, 1, 6][ns % 3], ac.MODES[ns % 3]), fc.WHENS
    for n_rows in (1, 3, 4, 5, 257):
        yield f"rows {n_rows}", fc.case(1000 + n_rows, n_rows, 65, 1, "max"), fc.WHENS
    for k in range(7):
        yield f"k {k}", fc.case(2000 + k, 16, 129, k, ac.MODES[k % 3]), fc.WHENS
    for n_rows in (7, 8, 9, 17):
        yield f"tiles {n_rows}", fc.case(3000 + n_rows, n_rows, 70, 2, "mean"), ("always",)
    for mode in ac.MODES:
        yield f"special {mode}", fc.special_case(mode), fc.WHENS
    yield "collinear", fc.collinear_case(), ("always",)
    yield from fc.edge_cases()


def test_the_rule_with_the_wave_order_route_on_every_ordinary_case(capsys):
    """On every case of tests/test_gpu_assoc.py and tests/test_gpu_assoc_edges.py: the reference decides as route "chol" does and
    stops at its step outside the band; the wave-order route does too, passes the per-row rule and the p check; and the rows the
    per-row rule was made for are held as tightly as it promises."""
    worst, lines = (0.0, ""), []
    for name, c in _ordinary_cases():
        hold = ~c.skip
        for f in ("status", "n", "n_g1", "n_g2"):
            assert np.array_equal(c.ref[f], c.want[f]), (name, f)
        assert np.array_equal(c.ref["n_iter"][hold], c.want["n_iter"][hold]), name
        wave = rf.assoc_rows(rf.WAVE, c.values, c.y, c.cov, c.outcome, c.mode, c.cutoff)
        assert np.array_equal(wave["status"], c.want["status"]) and np.array_equal(wave["n_iter"][hold], c.want["n_iter"][hold]), name
        share = ac.compare_rows(c, wave, "wave-order route")
        ac.compare_p(c, wave, "wave-order route")
        tol = c.tol_row[0][c.fitted]
        lines.append(f"{name}: one tolerance {c.tol:.1e}, per row {tol.min() if len(tol) else 0:.1e} .. {tol.max() if len(tol) else 0:.1e}, "
                     f"wave-order route's worst share {share:.3f}")
        worst = max(worst, (share, name))
    print("\n".join(lines))
    print("worst share of a row's tolerance, wave-order route:", worst)
    # the ns = 3 binary boundary case: one tolerance of 10 before, every row now below 1e-11
    c = ac.case(3, 24, 3, 0, "binary", "max")
    assert c.tol >= 1.0 and c.tol_row[0][c.fitted].max() < 1e-11
    # the rows test_constructed_rows exists for, next to quasi-separated row 9
    at = {n: i for i, n in enumerate(ac.SPECIAL_NAMES)}
    for o in ("binary", "continuous"):
        for mode in ac.MODES:
            c = ac.special_case(o, mode)
            for n in ("nan_lane0", "nan_lane63", "nan_last", "nan_one_haplotype"):
                assert c.fitted[at[n]] and c.tol_row[0][at[n]] < 1e-11, (o, mode, n, c.tol_row[0][at[n]])


def test_the_rule_with_the_wave_order_route_on_every_firth_case():
    """the same for tests/test_gpu_firth.py and tests/test_gpu_firth_edges.py"""
    worst, lines = (0.0, ""), []
    for name, c, whens in _firth_cases():
        hold = ~c.skip
        assert np.array_equal(c.ref["status"], c.R.chol["status"]), name
        wave = rf.firth_rows(rf.WAVE, c.values, c.y, c.cov, c.mode, c.cutoff)
        assert np.array_equal(wave["status"], c.R.chol["status"]), name
        for f in ("n_iter_full", "n_iter_null"):
            assert np.array_equal(c.ref[f][hold], c.R.chol[f][hold]) and np.array_equal(wave[f][hold], c.R.chol[f][hold]), (name, f)
        for when in whens:
            fitted = c.R.fitted(when)
            got = {f: np.where(fitted, v, math.nan) if v.dtype.kind == "f" else v for f, v in wave.items()}
            share = fc.compare_rows(c, when, got, "wave-order route")
            fc.compare_p(c, when, got, "wave-order route")
            tol = c.tol_row(when)[0][fitted]
            lines.append(f"{name} {when}: one tolerance {c.tol(when)[0]:.1e}, per row {tol.min() if len(tol) else 0:.1e} .. "
                         f"{tol.max() if len(tol) else 0:.1e}, wave-order route's worst share {share:.3f}")
            worst = max(worst, (share, f"{name} {when}"))
    print("\n".join(lines))
    print("worst share of a row's tolerance, wave-order route:", worst)


# ---- the p-value functions -------------------------------------------------------------------------------------------------------

P_DF = (1, 2, 3, 7, 30, 61, 126, 298, 4096, 65533)


def test_p_functions_against_mpmath():
    """assoc_restatement.student_t_two_sided against mpmath's regularised incomplete beta and math.erfc against mpmath's, at 40
    digits, on df x the |t| of assoc_cases.t_targets: the largest errors in units of 2^-52 max(1, |log p|) are the constants the
    GPU tests' allowance is made of, Student's t by bands of df.  Where the true value is below 2^-1022 the host's must be too."""
    worst_t, worst_z, skipped, points = {top: (0.0, None) for top, _ in rf.P_UNITS_T}, 0.0, 0, 0
    with mpmath.workdps(40):
        tiny = mpmath.mpf(2) ** -1022
        for df in P_DF:
            for t in ac.t_targets(df):
                points += 1
                try:
                    x = mpmath.mpf(df) / (mpmath.mpf(df) + mpmath.mpf(t) ** 2)
                    want = mpmath.betainc(mpmath.mpf(df) / 2, mpmath.mpf(1) / 2, 0, x, regularized=True)
                except mpmath.libmp.NoConvergence:
                    skipped += 1
                    continue
                got = ar.student_t_two_sided(t, df)
                if want < tiny:
                    assert 0.0 <= got < 2.0 ** -1022, (df, t, got)
                    continue
                u = float(abs(mpmath.mpf(got) - want) / want / (mpmath.mpf(2) ** -52 * max(1, abs(mpmath.log(want)))))
                band = next(top for top, _ in rf.P_UNITS_T if df <= top)
                if u > worst_t[band][0]:
                    worst_t[band] = (u, (df, t))
        for z in sorted({t for df in P_DF for t in ac.t_targets(df)}):
            want = mpmath.erfc(mpmath.mpf(z) / mpmath.sqrt(2))
            got = math.erfc(z / math.sqrt(2.0))
            if want < tiny:
                assert 0.0 <= got < 2.0 ** -1022, (z, got)
                continue
            worst_z = max(worst_z, float(abs(mpmath.mpf(got) - want) / want / (mpmath.mpf(2) ** -52 * max(1, abs(mpmath.log(want))))))
    for top, (u, at) in worst_t.items():
        print(f"student_t_two_sided, df up to {top}: {u:.1f} units at (df, t) = {at}")
    print(f"erfc: {worst_z:.2f} units; {skipped} of {points} points skipped")
    assert skipped < 0.02 * points and worst_z <= rf.P_UNITS_ERFC
    for top, units in rf.P_UNITS_T:
        assert 0.5 * units < worst_t[top][0] <= units, (top, worst_t[top])  # the constant is this measurement, not a roomy guess
    assert [rf.p_units_t(df) for df in (1, 298, 299, 4096, 4097, 65533)] == [37.0, 37.0, 44.0, 44.0, 7527.0, 7527.0]
