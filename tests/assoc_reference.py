"""The model of `inquistr assoc` (include/inquistr_hip.h) a third time, generic in the number type and in the order
of summation: the ordinary logistic fit, least squares, and Firth's full and null fit with their l*.  Everything but those two is
as tests/assoc_restatement.py's and tests/firth_restatement.py's route "chol" (and the kernels) have it: the x rule, the row filters,
the centring, the start values, the mu clamp at 2^-52, the stopping rules, x as the last column for Firth, and an explicit Cholesky.

Two instances:

REFERENCE   np.longdouble (x87 extended, eps 1.1e-19) with plain sums.  What the f64 routes and the device are measured against:
            its own rounding is three and a half digits below theirs.  tests/test_assoc_reference.py pins it to the closed forms
            and to a 40-digit mpmath run of the same iteration.
WAVE        np.float64 with every sum taken as the kernels take it: lane l adds samples l, l + 64, ... in ascending order (a sample
            without an x adds nothing but keeps its lane), then the butterfly xor 1, 2, ... 32.  It stands in for the device where
            there is none and is never part of a tolerance.  (The compiler may contract the kernels' a += b * c; this route cannot.)

The p-values of both are the f64 functions of tests/assoc_restatement.py at the f64-rounded statistic: rounding a statistic t to f64
moves log p by t^2 2^-53, 2^-52 of log p itself, and what those functions are worth is measured on its own (P_UNITS_ERFC, P_UNITS_T below).

The per-row rule (row errors, tolerances) that assoc_cases.compare and firth_cases.compare apply lives here too."""
import math

import numpy as np

from tests import assoc_restatement as ar
from tests import firth_restatement as fr

assert np.finfo(np.longdouble).nmant >= 63, (
    "tests/assoc_reference.py needs an extended-precision np.longdouble (64-bit significand, x87): here it has "
    f"{np.finfo(np.longdouble).nmant + 1} bits, no more than the f64 it is to judge")

LD = np.longdouble
FLOOR = 64 * 2.0 ** -52
P_MIN_NORMAL = 2.0 ** -1022
_LANES = np.arange(64)


def plain_sum(a, idx):
    """column sums of a [n, ...]; idx (the samples' places in the row) is not used"""
    return np.asarray(a).sum(axis=0)


def wave_sum(a, idx):
    """column sums of a [n, ...] in the kernels' order; idx: each entry's sample index, ascending"""
    a = np.asarray(a)
    steps = int(idx[-1]) // 64 + 1 if len(idx) else 0
    pad = np.zeros((steps, 64) + a.shape[1:], a.dtype)
    pad[idx // 64, idx % 64] = a
    acc = np.zeros((64,) + a.shape[1:], a.dtype)
    for s in range(steps):
        acc = acc + pad[s]
    d = 1
    while d < 64:
        acc = acc + acc[_LANES ^ d]
        d *= 2
    return acc[0]


class Arith:
    def __init__(self, name, dtype, sum_):
        self.name, self.dtype, self.sum = name, dtype, sum_


REFERENCE = Arith("long double", np.longdouble, plain_sum)
WAVE = Arith("wave order", np.float64, wave_sum)


def _cholesky(T, M, tol):
    """in place, lower triangle -> factor; False where a pivot is not above tol (the factor is then unusable)"""
    p = len(M)
    ok = True
    for j in range(p):
        d = M[j, j]
        for k in range(j):
            d = d - M[j, k] * M[j, k]
        ok = ok and bool(d > tol)
        M[j, j] = np.sqrt(d)
        for i in range(j + 1, p):
            s = M[i, j]
            for k in range(j):
                s = s - M[i, k] * M[j, k]
            M[i, j] = s / M[j, j]
    return ok


def _forward(T, L, r):
    v = np.zeros(len(r), T)
    for i in range(len(r)):
        s = r[i]
        for k in range(i):
            s = s - L[i, k] * v[k]
        v[i] = s / L[i, i]
    return v


def _backward(T, L, v):
    v = v.copy()
    for i in range(len(v) - 1, -1, -1):
        s = v[i]
        for k in range(i + 1, len(v)):
            s = s - L[k, i] * v[k]
        v[i] = s / L[i, i]
    return v


def _sums(A, cols, w, idx, z=None):
    """M = sum w xc xc' (lower triangle filled) and, with z, r = sum w xc z, the products taken as the kernels take them"""
    T, p = A.dtype, len(cols)
    wx = [w * c for c in cols]
    terms = [wx[i] * cols[j] for i in range(p) for j in range(i + 1)]
    if z is not None:
        terms += [wx[i] * z for i in range(p)]
    s = A.sum(np.stack(terms, axis=1), idx)
    M = np.zeros((p, p), T)
    at = 0
    for i in range(p):
        for j in range(i + 1):
            M[i, j] = s[at]
            at += 1
    return M, (s[at:] if z is not None else None)


def _eta(cols, beta):
    eta = beta[0] + beta[1] * cols[1]
    for j in range(2, len(cols)):
        eta = eta + beta[j] * cols[j]
    return eta


def _kept(A, h1, h2, y, cov, mode):
    """the kept samples' places, x, y, covariates in the instance's type; ns, p"""
    T = A.dtype
    y = np.asarray(y, dtype=np.float64)
    ns = len(y)
    cov = np.zeros((0, ns)) if cov is None else np.asarray(cov, dtype=np.float64).reshape(-1, ns)
    x = ar.predictor(h1, h2, mode)
    keep = ~np.isnan(x)
    idx = np.nonzero(keep)[0]
    return idx, x[keep].astype(T), y[keep].astype(T), cov[:, keep].astype(T), ns, 2 + len(cov)


def _centred(A, idx, xs, cs):
    """x and the covariates, each less its mean over the kept samples"""
    n = A.dtype(len(xs))
    return xs - A.sum(xs, idx) / n, [c - A.sum(c, idx) / n for c in cs]


def fit_row(A, h1, h2, y, cov, outcome="binary", mode="max", missing_cutoff=0.8):
    """One locus, the ordinary fit: (row as a dict of the fields of inq_assoc_row_t, the numbers in A's type; last criterion)"""
    T = A.dtype
    idx, xs, ys, cs, ns, p = _kept(A, h1, h2, y, cov, mode)
    n = len(xs)
    nan = T(math.nan)
    row = dict(beta=nan, se=nan, stat=nan, p=math.nan, mean_all=nan, mean_g1=nan, mean_g2=nan, min_x=nan, max_x=nan, n=n, n_g1=0, n_g2=0,
               status=ar.OK, n_iter=0)
    binary = outcome == "binary"
    with np.errstate(all="ignore"):
        sx = T(0)
        if n:
            sx = A.sum(xs, idx)
            row["mean_all"], row["min_x"], row["max_x"] = sx / T(n), xs.min(), xs.max()
        if binary:
            g2 = ys != 0
            row["n_g1"], row["n_g2"] = int((~g2).sum()), int(g2.sum())
            if row["n_g1"]:
                row["mean_g1"] = A.sum(np.where(g2, T(0), xs), idx) / T(row["n_g1"])
            if row["n_g2"]:
                row["mean_g2"] = A.sum(np.where(g2, xs, T(0)), idx) / T(row["n_g2"])
        if ns == 0 or not n / ns >= missing_cutoff:
            row["status"] = ar.LOW_CALL_RATE
        elif not row["min_x"] != row["max_x"]:
            row["status"] = ar.CONSTANT
        elif binary and (not row["n_g1"] or not row["n_g2"]):
            row["status"] = ar.ONE_GROUP
        elif n <= p:
            row["status"] = ar.TOO_FEW
        elif not abs(sx) < math.inf:
            row["status"] = ar.SINGULAR
        if row["status"] != ar.OK:
            return row, math.nan

        xc, cc = _centred(A, idx, xs, cs)
        cols = [np.ones(n, T), xc] + cc

        def wls(w, z):
            M, r = _sums(A, cols, w, idx, z)
            if not _cholesky(T, M, ar.RANK_TOL * M.diagonal().max()):
                return None
            e = np.zeros(p, T)
            e[1] = 1
            return _backward(T, M, _forward(T, M, r)), _backward(T, M, _forward(T, M, e))[1]

        crit = math.nan
        if binary:
            eps = T(2) ** -52
            beta, inv_xx, dev_old = None, nan, T(0)
            for t in range(ar.MAX_ITER + 1):
                if t == 0:
                    mu = (ys + 0.5) * 0.5
                    eta = np.log(mu / (1 - mu))
                else:
                    eta = _eta(cols, beta)
                    mu = np.clip(1 / (1 + np.exp(-eta)), eps, 1 - eps)
                dev = A.sum(-2 * np.log(np.where(ys != 0, mu, 1 - mu)), idx)
                if t >= 1:
                    row["n_iter"] = t
                    if not abs(dev) < math.inf:
                        row["status"] = ar.NOT_CONVERGED
                        break
                    crit = float(abs(dev - dev_old) / (abs(dev) + 0.1))
                    if abs(dev - dev_old) / (abs(dev) + 0.1) < ar.CONVERGED:
                        break
                    if t == ar.MAX_ITER:
                        row["status"] = ar.NOT_CONVERGED
                        break
                dev_old = dev
                w = mu * (1 - mu)
                got = wls(w, eta + (ys - mu) / w)
                if got is None:
                    row["status"], row["n_iter"] = ar.SINGULAR, 0
                    return row, math.nan
                beta, inv_xx = got
            row["beta"], row["se"] = beta[1], np.sqrt(inv_xx)
            row["stat"] = row["beta"] / row["se"]
            s = float(row["stat"])
            row["p"] = math.erfc(abs(s) * 0.70710678118654752440) if s == s else math.nan
        else:
            got = wls(np.ones(n, T), ys)
            if got is None:
                row["status"] = ar.SINGULAR
                return row, math.nan
            beta, inv_xx = got
            res = ys - _eta(cols, beta)
            df = n - p
            row["beta"] = beta[1]
            row["se"] = np.sqrt(A.sum(res * res, idx) / T(df) * inv_xx)
            row["stat"] = row["beta"] / row["se"]
            row["p"] = ar.student_t_two_sided(float(row["stat"]), df)
    return row, crit


def _firth_fit(A, ys, cols, idx, null):
    """one of Firth's two fits: dict(status, beta_x, se, pll, n_iter, crits: the criterion of every evaluation)"""
    T, p = A.dtype, len(cols)
    eps = T(2) ** -52
    beta = np.zeros(p, T)
    out = dict(status=fr.OK, beta=T(0), se=T(math.nan), pll=T(math.nan), n_iter=0, crits=[])
    for t in range(fr.MAX_ITER + 1):
        eta = _eta(cols, beta)
        pi = np.clip(1 / (1 + np.exp(-eta)), eps, 1 - eps)
        w = pi * (1 - pi)
        M, _ = _sums(A, cols, w, idx)
        diag = M.diagonal().copy()
        if not _cholesky(T, M, ar.RANK_TOL * diag.max()):
            out["status"] = fr.SINGULAR
            return out
        logdet = T(0)
        for j in range(p):
            logdet = logdet + np.log(M[j, j])
        u = []  # the forward substitution L u = xc of every sample at once
        for i in range(p):
            s = cols[i]
            for k in range(i):
                s = s - M[i, k] * u[k]
            u.append(s / M[i, i])
        h = u[0] * u[0]
        for j in range(1, p):
            h = h + u[j] * u[j]
        h = h * w
        sc = (ys - pi) + h * (0.5 - pi)
        s = A.sum(np.stack([sc * c for c in cols] + [np.log(np.where(ys != 0, pi, 1 - pi))], axis=1), idx)
        U, ll = s[:p], s[p]
        pll = ll + logdet
        out.update(beta=beta[p - 1], se=1 / M[p - 1, p - 1], pll=pll, n_iter=t)
        if not abs(pll) < math.inf:
            out["status"] = fr.NOT_CONVERGED
            return out
        v = _forward(T, M, U)
        if null:
            v[p - 1] = 0
        delta = _backward(T, M, v)
        crit = big = T(0)
        for j in range(p):
            d = abs(delta[j])
            c = d * np.sqrt(diag[j])
            big = d if d > big else big
            crit = c if c > crit else crit
        out["crits"].append(float(crit))
        if crit < fr.CONVERGED:
            return out
        if t == fr.MAX_ITER:
            out["status"] = fr.NOT_CONVERGED
            return out
        beta = beta + delta * (fr.MAX_STEP / big if big > fr.MAX_STEP else 1)
    return out


def firth_fit_row(A, h1, h2, y, cov, mode="max", fits=None):
    """Both of Firth's fits of one locus that is fitted: the row as a dict of the fields of inq_assoc_firth_row_t; the fits
    themselves are appended to `fits` where one is given"""
    T = A.dtype
    idx, xs, ys, cs, ns, p = _kept(A, h1, h2, y, cov, mode)
    nan = T(math.nan)
    row = dict(beta=nan, se=nan, chi2=nan, p=math.nan, pll_full=nan, pll_null=nan, n_iter_full=0, n_iter_null=0, status=fr.OK)
    with np.errstate(all="ignore"):
        xc, cc = _centred(A, idx, xs, cs)
        cols = [np.ones(len(xs), T)] + cc + [xc]
        full = _firth_fit(A, ys, cols, idx, False)
        null = _firth_fit(A, ys, cols, idx, True) if full["status"] != fr.SINGULAR else None
        if fits is not None:
            fits += [f for f in (full, null) if f is not None]
        if null is None or null["status"] == fr.SINGULAR:
            row["status"] = fr.SINGULAR
            return row
        d = 2 * (full["pll"] - null["pll"])
        chi2 = d if d > 0 else T(0)
        row.update(beta=full["beta"], se=full["se"], chi2=chi2, p=math.erfc(math.sqrt(float(chi2) * 0.5)), pll_full=full["pll"],
                   pll_null=null["pll"], n_iter_full=full["n_iter"], n_iter_null=null["n_iter"],
                   status=fr.NOT_CONVERGED if fr.NOT_CONVERGED in (full["status"], null["status"]) else fr.OK)
    return row


NUMBERS = ("beta", "se", "stat", "mean_all", "mean_g1", "mean_g2", "min_x", "max_x")
FIRTH_NUMBERS = ("beta", "se", "chi2", "pll_full", "pll_null")


def _table(rows, numbers, T):
    out = {}
    for f in rows[0] if rows else ():
        out[f] = np.array([r[f] for r in rows], dtype=T if f in numbers else np.float64 if f == "p" else np.int64)
    return out


def assoc_rows(A, values, y, cov=None, outcome="binary", mode="max", missing_cutoff=0.8):
    """values f32 [n_rows, 2 * n_samples] -> the rows as a dict of arrays by field, the numbers in A's type"""
    values = np.asarray(values, dtype=np.float32)
    return _table([fit_row(A, v[0::2], v[1::2], y, cov, outcome, mode, missing_cutoff)[0] for v in values], NUMBERS, A.dtype)


def firth_rows(A, values, y, cov=None, mode="max", missing_cutoff=0.8):
    """Firth's rows of every row whose ordinary status (by A's own ordinary fit) is OK or NOT_CONVERGED, the others NOT_FITTED"""
    values = np.asarray(values, dtype=np.float32)
    nan = A.dtype(math.nan)
    rows = []
    for v in values:
        o, _ = fit_row(A, v[0::2], v[1::2], y, cov, "binary", mode, missing_cutoff)
        if o["status"] in (ar.OK, ar.NOT_CONVERGED):
            rows.append(firth_fit_row(A, v[0::2], v[1::2], y, cov, mode))
        else:
            rows.append(dict(beta=nan, se=nan, chi2=nan, p=math.nan, pll_full=nan, pll_null=nan, n_iter_full=0, n_iter_null=0,
                             status=fr.NOT_FITTED))
    return _table(rows, FIRTH_NUMBERS, A.dtype)


# ---- the per-row rule -------------------------------------------------------------------------------------------------------------

def _scaled(got, ref, scale):
    """|got - ref| / scale per row in long double; equal values (NaN with NaN, inf with inf) count 0, anything else not finite inf"""
    got, ref = np.asarray(got, dtype=LD), np.asarray(ref, dtype=LD)
    with np.errstate(all="ignore"):
        same = (got == ref) | (np.isnan(got) & np.isnan(ref))
        e = np.abs(got - ref) / scale
        return np.where(same, 0.0, np.where(np.isfinite(e), e, math.inf)).astype(np.float64)


def _log_p_error(got_p, ref_p, least=1):
    """|log p - log p_ref| / max(1, |log p_ref|, least); where p_ref is denormal or 0 the p-value is held by check_p alone"""
    with np.errstate(all="ignore"):
        lg, lr = np.log(np.asarray(got_p, dtype=LD)), np.log(np.asarray(ref_p, dtype=LD))
        e = _scaled(lg, lr, np.maximum(np.maximum(1, np.abs(lr)), least))
    return np.where(np.asarray(ref_p) < P_MIN_NORMAL, 0.0, e)


def row_errors(got, ref, fitted):
    """The ordinary fit's error per row against the reference's rows: beta in units of se_ref, se and the means relative, stat
    against max(1, |stat_ref|), log p against max(1, |log p_ref|); a row's error is the largest of them, 0 where it is not fitted"""
    with np.errstate(all="ignore"):
        se, stat = np.asarray(ref["se"], dtype=LD), np.asarray(ref["stat"], dtype=LD)
        each = [_scaled(got["beta"], ref["beta"], se), _scaled(got["se"], se, np.abs(se)), _scaled(got["stat"], stat, np.maximum(1, np.abs(stat))),
                _log_p_error(got["p"], ref["p"])]
        each += [_scaled(got[f], ref[f], np.abs(np.asarray(ref[f], dtype=LD))) for f in ("mean_all", "mean_g1", "mean_g2")]
    return np.where(fitted, np.max(each, axis=0), 0.0)


def firth_row_errors(got, ref, fitted):
    """Firth's: beta in units of se_ref, se and both l* relative, chi2 against max(chi2_ref, |l*_full_ref|) (one rounding of an l*
    moves chi2 by 2 eps |l*| whoever computes it), log p against max(1, |log p_ref|)"""
    with np.errstate(all="ignore"):
        se, chi2, pf = (np.asarray(ref[f], dtype=LD) for f in ("se", "chi2", "pll_full"))
        each = [_scaled(got["beta"], ref["beta"], se), _scaled(got["se"], se, np.abs(se)), _scaled(got["chi2"], chi2, np.maximum(chi2, np.abs(pf))),
                _scaled(got["pll_full"], pf, np.abs(pf)), _scaled(got["pll_null"], ref["pll_null"], np.abs(np.asarray(ref["pll_null"], dtype=LD)))]
        # log p = log erfc(sqrt(chi2 / 2)) inherits chi2's error, which is held at the scale |l*|: towards chi2 = 0 its slope in
        # chi2 is 1 / sqrt(2 pi chi2), without bound, so |l*| times that slope joins the scale (a row whose chi2 the device may
        # clamp to 0 is otherwise held at log p = 0 to what no rounding of l* leaves); check_p holds p to chi2_dev everywhere
        each.append(_log_p_error(got["p"], ref["p"], np.abs(pf) / np.sqrt(2 * LD(math.pi) * chi2)))
    return np.where(fitted, np.max(each, axis=0), 0.0)


def tolerances(e_chol, e_qr, fitted):
    """tol_row = 10 x max(e_row, e_typ, 64 * 2^-52): e_row the larger of the two f64 routes' errors on that row against the
    reference, e_typ the 90th percentile of e_row over the case's fitted rows.  -> (tol_row, e_row, e_typ)"""
    e_row = np.maximum(e_chol, e_qr)
    e_typ = float(np.percentile(e_row[fitted], 90)) if fitted.any() else 0.0
    return 10.0 * np.maximum(np.maximum(e_row, e_typ), FLOOR), e_row, e_typ


def worst_share(err, tol, fitted):
    """(largest err / tol over the fitted rows, its row), (0, -1) where there is none"""
    if not fitted.any():
        return 0.0, -1
    share = np.where(fitted, err / tol, 0.0)
    i = int(np.argmax(share))
    return float(share[i]), i


# ---- the p-value as a function of the statistic -------------------------------------------------------------------------------

# The largest error of the host's two functions against mpmath at 40 digits, in units of 2^-52 max(1, |log p|) of p, over the grid
# of tests/test_assoc_reference.py::test_p_functions_against_mpmath, which asserts them (rounded up; measured 1.41 for erfc and,
# for Student's t, 36.5 up to df = 298, 43.5 at df = 4096, 7526.5 at df = 65533).  math.erfc is good to its last bits.
# assoc_restatement.student_t_two_sided, the kernel's algorithm line for line, loses digits as df grows, so its constant goes by
# bands of df, each band measured at its upper end (and, up to 298, at eight df below it).  At df = 65533, |t| = 1.767 - just
# on the side of the switch (a + 1) / (a + b + 2) where the fraction in x is taken, a = df / 2 - p is 4.3e-12 off (the 7526 units)
# and the continued fraction itself 6.1e-12.  That is not the stopping rule: the same f64 loop run for 800 steps without a stop is
# 4.9e-12 off there (and 1.7e-12 instead of 5e-13 at t = 3, 1.1e-12 instead of 1.7e-13 at t = 5: worse), while the recurrence in
# 40 digits has its factors within 1e-13 of 1 by the step where f64 stops.  The fraction's value is about 1.7e4 there, and the
# error is rounding gathered inside the f64 recurrence of d and c on the way to it.  On the other side of the switch (8 steps)
# the fraction is good to 3e-16 and what is left is the coefficient's recurrence, 2e-14 off at df = 65533.
P_UNITS_ERFC = 2.0
P_UNITS_T = ((298, 37.0), (4096, 44.0), (65535, 7527.0))  # (largest df of the band, units)


def p_units_t(df):
    """the Student t's constant for df degrees of freedom: that of the first band that holds df"""
    return next(u for top, u in P_UNITS_T if df <= top)


def p_allowed(units):
    """what a device p may differ by from the host's function of the same statistic: 10 x max(64, the function's own error)"""
    return 10.0 * max(64.0, units)


def p_units(p_got, p_host):
    """|p_got - p_host| / p_host in units of 2^-52 max(1, |log p_host|)"""
    return abs(p_got - p_host) / p_host / (2.0 ** -52 * max(1.0, abs(math.log(p_host))))


def check_p(p_dev, p_host, what, allowed):
    """p_dev against the host's value of the same function at the device's own statistic: within `allowed` units (one number, or
    one per row), or, where the host's is denormal or 0 (math libraries may flush there), anywhere in [0, 2^-1022).  -> (the
    largest share of its allowance a row used, the most units a row used)"""
    worst = units = 0.0
    each = np.broadcast_to(np.asarray(allowed, dtype=np.float64), np.shape(p_dev)).tolist()
    for i, (g, h) in enumerate(zip(np.asarray(p_dev, dtype=np.float64).tolist(), np.asarray(p_host, dtype=np.float64).tolist())):
        if h != h:
            assert g != g, (what, i, g, h)
        elif h < P_MIN_NORMAL:
            assert 0.0 <= g < P_MIN_NORMAL, (what, i, g, h)
        else:
            u = p_units(g, h)
            assert u <= each[i], (what, i, g, h, u, each[i])
            worst, units = max(worst, u / each[i]), max(units, u)
    return worst, units
