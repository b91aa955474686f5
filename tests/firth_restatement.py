"""Firth's penalised logistic regression as inq_assoc_rows_firth fits it (include/inquistr_hip.h), in plain numpy f64,
one locus at a time, beside tests/assoc_restatement.py, whose ordinary fit decides which rows are fitted.

Written twice, as that file is.  Route "chol" is what the kernel does: columns [1, covariates..., x] centred on their means over the
kept samples, I = X'WX factored by a Cholesky whose pivots carry the rank test, hat values by a forward substitution with the
factor.  Route "qr" keeps the columns UNCENTRED and takes everything from a QR factorisation of sqrt(W) X: the hat values are the
squared row norms of Q, log det I = 2 sum log |R_jj| (centring has determinant 1), the pivots are R_jj^2.  Centring is a linear
reparametrisation: beta_x, its standard error and l* do not see it; the step limit and the convergence criterion are stated in the
centred coordinates, so route "qr" carries its step over before it measures it.

No logistf exists where this runs, so parity with it is unpinned; tests/test_firth_restatement.py pins both routes to the 2 x 2
closed form and to scipy.optimize."""
import math

import numpy as np

from tests import assoc_restatement as ar

OK, NOT_FITTED, SINGULAR, NOT_CONVERGED = range(4)
STATUS_NAMES = ("OK", "NOT_FITTED", "SINGULAR", "NOT_CONVERGED")
MAX_ITER = 100
CONVERGED = 1e-9
MAX_STEP = 5.0
MU_BOUND = 1e-6
CRIT_BAND = 0.01  # n_iter is not held where a fit's last or last-but-one criterion lies within 1 % of CONVERGED

ROW_DTYPE = np.dtype([("beta", "<f8"), ("se", "<f8"), ("chi2", "<f8"), ("p", "<f8"), ("pll_full", "<f8"), ("pll_null", "<f8"),
                      ("n_iter_full", "u1"), ("n_iter_null", "u1"), ("status", "u1"), ("pad", "u1", (5,))])
FIT_FIELDS = ("beta", "se", "chi2", "pll_full", "pll_null")


def columns(h1, h2, y, cov, mode):
    """the kept samples' y, X = [1, cov..., x] uncentred and the same centred on the column means"""
    y = np.asarray(y, dtype=np.float64)
    ns = len(y)
    cov = np.zeros((0, ns)) if cov is None else np.asarray(cov, dtype=np.float64).reshape(-1, ns)
    x = ar.predictor(h1, h2, mode)
    keep = ~np.isnan(x)
    n = int(keep.sum())
    X = np.column_stack([np.ones(n)] + [c[keep] for c in cov] + [x[keep]])
    Xc = X.copy()
    Xc[:, 1:] -= Xc[:, 1:].sum(axis=0) / n
    return y[keep], X, Xc


def _cholesky(M, tol):
    p = len(M)
    L = np.zeros((p, p))
    for j in range(p):
        d = M[j, j] - L[j, :j] @ L[j, :j]
        if not d > tol:
            return None
        L[j, j] = math.sqrt(d)
        for i in range(j + 1, p):
            L[i, j] = (M[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    return L


def _forward(L, r):
    v = np.zeros(len(r))
    for i in range(len(r)):
        v[i] = (r[i] - L[i, :i] @ v[:i]) / L[i, i]
    return v


def _backward(L, v):
    v = v.copy()
    for i in range(len(v) - 1, -1, -1):
        v[i] = (v[i] - L[i + 1:, i] @ v[i + 1:]) / L[i, i]
    return v


def evaluate(route, ys, X, Xc, beta, null):
    """At beta (route "chol": of the centred columns, "qr": of the uncentred ones): None where a pivot fails, else
    (l*, delta in the route's own coordinates, delta in the centred ones, diagonal of the centred I, se of beta_x)."""
    p = X.shape[1]
    design = Xc if route == "chol" else X
    with np.errstate(all="ignore"):
        eta = design @ beta
        pi = np.clip(1.0 / (1.0 + np.exp(-eta)), ar.MU_EPS, 1.0 - ar.MU_EPS)
        w = pi * (1.0 - pi)
        # l* is stationary at the fit, so what the routes' different beta do to it is nothing: its rounding is that of the terms and
        # of their sum, and chi2 is a difference of two of them.  Each route takes the terms by its own formula and the sum in its own
        # order (the clamped samples apart), or the two would agree on l* bit for bit and say nothing about it
        terms = np.log(np.where(ys != 0.0, pi, 1.0 - pi))
        if route == "chol":
            ll = float(terms.sum())
        else:
            inside = (pi > ar.MU_EPS) & (pi < 1.0 - ar.MU_EPS)
            terms = np.where(inside, -np.log1p(np.exp(np.where(ys != 0.0, -eta, eta))), terms)  # log pi = -log(1 + exp(-eta))
            ll = float(np.cumsum(terms)[-1])
        diag = (w[:, None] * Xc * Xc).sum(axis=0)
        tol = ar.RANK_TOL * diag.max()
        if route == "chol":
            M = Xc.T @ (w[:, None] * Xc)
            diag = M.diagonal().copy()
            L = _cholesky(M, ar.RANK_TOL * diag.max())
            if L is None:
                return None
            half_logdet = float(np.log(L.diagonal()).sum())
            u = np.array([_forward(L, row) for row in Xc])
            h = w * (u * u).sum(axis=1)
            U = Xc.T @ ((ys - pi) + h * (0.5 - pi))
            v = _forward(L, U)
            if null:
                v[p - 1] = 0.0
            delta = _backward(L, v)
            return ll + half_logdet, delta, delta, diag, 1.0 / L[p - 1, p - 1]
        Q, R = np.linalg.qr(np.sqrt(w)[:, None] * X)
        if not np.all(R.diagonal() ** 2 > tol):
            return None
        half_logdet = float(np.log(np.abs(R.diagonal())).sum())
        h = (Q * Q).sum(axis=1)
        U = X.T @ ((ys - pi) + h * (0.5 - pi))
        f = p - 1 if null else p
        delta = np.zeros(p)
        delta[:f] = np.linalg.solve(R[:f, :f], np.linalg.solve(R[:f, :f].T, U[:f]))
        centred = delta.copy()
        centred[0] += (X[:, 1:].sum(axis=0) / len(X)) @ delta[1:]
        Rinv = np.linalg.solve(R, np.eye(p))
        return ll + half_logdet, delta, centred, diag, math.sqrt(float(Rinv[p - 1] @ Rinv[p - 1]))


def fit(route, ys, X, Xc, null):
    """One fit: dict(status, beta (route's coordinates), se, pll, n_iter, crits: the criterion of every evaluation)"""
    p = X.shape[1]
    beta = np.zeros(p)
    out = dict(status=OK, beta=beta, se=math.nan, pll=math.nan, n_iter=0, crits=[])
    for t in range(MAX_ITER + 1):
        ev = evaluate(route, ys, X, Xc, beta, null)
        if ev is None:
            out["status"] = SINGULAR
            return out
        pll, delta, centred, diag, se = ev
        out.update(beta=beta, se=se, pll=pll, n_iter=t)
        if not abs(pll) < math.inf:
            out["status"] = NOT_CONVERGED
            return out
        crit = big = 0.0
        with np.errstate(all="ignore"):
            for j in range(p):
                d = abs(float(centred[j]))
                c = d * math.sqrt(diag[j])
                big = d if d > big else big
                crit = c if c > crit else crit
        out["crits"].append(crit)
        if crit < CONVERGED:
            return out
        if t == MAX_ITER:
            out["status"] = NOT_CONVERGED
            return out
        beta = beta + delta * (MAX_STEP / big if big > MAX_STEP else 1.0)
    return out


def in_band(fits):
    """does the last or the last-but-one criterion of one of the fits lie within CRIT_BAND of CONVERGED"""
    return any(abs(c / CONVERGED - 1.0) <= CRIT_BAND for f in fits for c in f["crits"][-2:])


def fit_row(h1, h2, y, cov, mode="max", route="chol"):
    """Both fits of one locus that is fitted: (row as a dict of the fields of inq_assoc_firth_row_t, [full fit, null fit])"""
    ys, X, Xc = columns(h1, h2, y, cov, mode)
    nan = math.nan
    row = dict(beta=nan, se=nan, chi2=nan, p=nan, pll_full=nan, pll_null=nan, n_iter_full=0, n_iter_null=0, status=OK)
    full = fit(route, ys, X, Xc, False)
    if full["status"] == SINGULAR:
        row["status"] = SINGULAR
        return row, [full]
    null = fit(route, ys, X, Xc, True)
    if null["status"] == SINGULAR:
        row["status"] = SINGULAR
        return row, [full, null]
    d = 2.0 * (full["pll"] - null["pll"])
    chi2 = d if d > 0.0 else 0.0
    row.update(beta=float(full["beta"][-1]), se=full["se"], chi2=chi2, p=math.erfc(math.sqrt(chi2 * 0.5)), pll_full=full["pll"],
               pll_null=null["pll"], n_iter_full=full["n_iter"], n_iter_null=null["n_iter"],
               status=NOT_CONVERGED if NOT_CONVERGED in (full["status"], null["status"]) else OK)
    return row, [full, null]


def ordinary_fit(h1, h2, y, cov, mode="max", missing_cutoff=0.8):
    """The ordinary binary fit's row (assoc_restatement.fit_row, route chol) and, where it is OK or NOT_CONVERGED, the smallest
    min(mu, 1 - mu) over the kept samples at its last pass: glm.fit's iteration once more, keeping what fit_row does not return"""
    row, _ = ar.fit_row(h1, h2, y, cov, "binary", mode, missing_cutoff, "chol")
    if row["status"] not in (ar.OK, ar.NOT_CONVERGED):
        return row, math.nan
    ys, X, Xc = columns(h1, h2, y, cov, mode)
    Xo = np.column_stack([Xc[:, 0], Xc[:, -1]] + [Xc[:, j] for j in range(1, Xc.shape[1] - 1)])  # that fit's order: [1, x, cov...]
    beta, dev_old, t_end = None, 0.0, 0
    with np.errstate(all="ignore"):
        for t in range(ar.MAX_ITER + 1):
            if t == 0:
                mu = (ys + 0.5) * 0.5
                eta = np.log(mu / (1.0 - mu))
            else:
                eta = Xo @ beta
                mu = np.clip(1.0 / (1.0 + np.exp(-eta)), ar.MU_EPS, 1.0 - ar.MU_EPS)
            dev = float((-2.0 * np.log(np.where(ys != 0.0, mu, 1.0 - mu))).sum())
            t_end = t
            if t >= 1 and (not abs(dev) < math.inf or abs(dev - dev_old) / (abs(dev) + 0.1) < ar.CONVERGED or t == ar.MAX_ITER):
                break
            dev_old = dev
            w = mu * (1.0 - mu)
            beta, _ = ar._wls_chol(Xo, w, eta + (ys - mu) / w)
    assert t_end == row["n_iter"], (t_end, row["n_iter"])
    return row, float(np.minimum(mu, 1.0 - mu).min())


def selected(when, status, min_mu, bound=MU_BOUND):
    """is a row with this ordinary status and smallest min(mu, 1 - mu) fitted"""
    if status not in (ar.OK, ar.NOT_CONVERGED):
        return False
    return when == "always" or status == ar.NOT_CONVERGED or bool(min_mu < bound)


class Rows:
    """What the restatement makes of a matrix: ordinary (assoc_restatement.ROW_DTYPE), min_mu, chol / qr: the Firth rows of ALL rows whose
    ordinary status is OK or NOT_CONVERGED by the two routes (the others NOT_FITTED), band: rows whose n_iter is not held"""

    def __init__(self, values, y, cov, mode="max", missing_cutoff=0.8):
        values = np.asarray(values, dtype=np.float32)
        n = len(values)
        self.ordinary = np.zeros(n, dtype=ar.ROW_DTYPE)
        self.min_mu = np.full(n, math.nan)
        self.chol, self.qr = np.zeros(n, dtype=ROW_DTYPE), np.zeros(n, dtype=ROW_DTYPE)
        self.band = np.zeros(n, dtype=bool)
        for i, v in enumerate(values):
            row, self.min_mu[i] = ordinary_fit(v[0::2], v[1::2], y, cov, mode, missing_cutoff)
            for k, val in row.items():
                self.ordinary[k][i] = val
            for dst, route in ((self.chol, "chol"), (self.qr, "qr")):
                if selected("always", row["status"], self.min_mu[i]):
                    r, fits = fit_row(v[0::2], v[1::2], y, cov, mode, route)
                    self.band[i] |= in_band(fits)
                else:
                    r = dict(beta=math.nan, se=math.nan, chi2=math.nan, p=math.nan, pll_full=math.nan, pll_null=math.nan, n_iter_full=0,
                             n_iter_null=0, status=NOT_FITTED)
                for k, val in r.items():
                    dst[k][i] = val

    def fitted(self, when, bound=MU_BOUND):
        return np.array([selected(when, s, m, bound) for s, m in zip(self.ordinary["status"], self.min_mu)], dtype=bool)

    def want(self, when, route="chol", bound=MU_BOUND):
        """the Firth rows under `when`: the rows it leaves out NOT_FITTED"""
        out = (self.chol if route == "chol" else self.qr).copy()
        blank = np.zeros(1, dtype=ROW_DTYPE)
        for f in ("beta", "se", "chi2", "p", "pll_full", "pll_null"):
            blank[f] = math.nan
        blank["status"] = NOT_FITTED
        out[~self.fitted(when, bound)] = blank[0]
        return out


def disagreement(a, b):
    """largest relative disagreement of beta, se, chi2, log p and both l* between two sets of Firth rows"""
    worst = max(ar.rel_diff(a[f], b[f]) for f in FIT_FIELDS)
    return max(worst, ar.rel_diff(ar.log_p(a["p"]), ar.log_p(b["p"])))
