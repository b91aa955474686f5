"""The model of `inquistr assoc` (include/inquistr_hip.h) in plain numpy f64, one locus at a time.

It is written twice.  Route "chol" is what the kernel does: every non-intercept column centred on its mean over the locus's kept
samples, the normal equations X'WX, X'Wz summed up and solved by a Cholesky factorisation whose pivots carry the rank test.  Route
"qr" is what R's glm.fit / lm.fit do: a QR factorisation of sqrt(W) X of the UNCENTRED columns; the squares of R's diagonal are
the same pivots (subtracting a multiple of the intercept column from another column changes no pivot behind the first), held to
the same threshold.  No R exists where this runs, so parity with R is unpinned; tests/test_assoc_restatement.py pins both routes to
hand-derived values and to scipy.

The rows come back as a structured array with the fields of inq_assoc_row_t (hipcall.ASSOC_ROW_DTYPE) and, beside it, each row's
last convergence criterion |dev - dev_old| / (|dev| + 0.1) (NaN where there was none)."""
import math

import numpy as np

OK, LOW_CALL_RATE, CONSTANT, ONE_GROUP, TOO_FEW, SINGULAR, NOT_CONVERGED = range(7)
STATUS_NAMES = ("OK", "LOW_CALL_RATE", "CONSTANT", "ONE_GROUP", "TOO_FEW", "SINGULAR", "NOT_CONVERGED")
MAX_ITER = 25
CONVERGED = 1e-8
MU_EPS = 2.0 ** -52
RANK_TOL = 1e-11
Z95 = 1.959963984540054

ROW_DTYPE = np.dtype([("beta", "<f8"), ("se", "<f8"), ("stat", "<f8"), ("p", "<f8"), ("mean_all", "<f8"), ("mean_g1", "<f8"),
                      ("mean_g2", "<f8"), ("min_x", "<f8"), ("max_x", "<f8"), ("n", "<u4"), ("n_g1", "<u4"), ("n_g2", "<u4"),
                      ("status", "u1"), ("n_iter", "u1"), ("pad", "u1", (2,))])


def predictor(h1, h2, mode):
    """pmax / pmin(H1, H2, na.rm = TRUE) and their mean (prepare_calls of the R script): NaN only where both are."""
    h1, h2 = np.asarray(h1, dtype=np.float64), np.asarray(h2, dtype=np.float64)
    m1, m2 = np.isnan(h1), np.isnan(h2)
    with np.errstate(invalid="ignore"):
        hi = np.where(m1, h2, np.where(m2, h1, np.where(h1 > h2, h1, h2)))
        lo = np.where(m1, h2, np.where(m2, h1, np.where(h1 < h2, h1, h2)))
        return hi if mode == "max" else lo if mode == "min" else (hi + lo) * 0.5


def _tri_solve(L, r):
    """L L' v = r"""
    p = len(r)
    v = np.zeros(p)
    for i in range(p):
        v[i] = (r[i] - L[i, :i] @ v[:i]) / L[i, i]
    for i in range(p - 1, -1, -1):
        v[i] = (v[i] - L[i + 1:, i] @ v[i + 1:]) / L[i, i]
    return v


def _wls_chol(Xc, w, z):
    """beta (of the centred columns) and (X'WX)^-1_xx, or None where a pivot is not above RANK_TOL x the largest diagonal"""
    p = Xc.shape[1]
    M = Xc.T @ (w[:, None] * Xc)
    r = Xc.T @ (w * z)
    tol = RANK_TOL * M.diagonal().max()
    L = np.zeros((p, p))
    for j in range(p):
        d = M[j, j] - L[j, :j] @ L[j, :j]
        if not d > tol:
            return None
        L[j, j] = math.sqrt(d)
        for i in range(j + 1, p):
            L[i, j] = (M[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    e = np.zeros(p)
    e[1] = 1.0
    return _tri_solve(L, r), _tri_solve(L, e)[1]


def _wls_qr(X, Xc, w, z):
    """the same from a QR factorisation of sqrt(W) X, X uncentred; the threshold's diagonal is that of the centred columns"""
    sw = np.sqrt(w)
    Q, R = np.linalg.qr(sw[:, None] * X)
    tol = RANK_TOL * ((w[:, None] * Xc * Xc).sum(axis=0)).max()
    piv = R.diagonal() ** 2
    if not np.all(piv > tol):
        return None
    beta = np.linalg.solve(R, Q.T @ (sw * z))
    Rinv = np.linalg.solve(R, np.eye(len(R)))
    return beta, float(Rinv[1] @ Rinv[1])


def t_coef(df):
    """1 / B(df / 2, 1 / 2) = Gamma((df + 1) / 2) / (Gamma(df / 2) sqrt(pi)) by c[df + 2] = c[df] (df + 1) / df"""
    c = 1.0 / math.pi if df % 2 else 0.5
    for d in range(1 if df % 2 else 2, df, 2):
        c = c * (d + 1) / d
    return c


def _beta_cf(a, b, x):
    tiny, qab, qap, qam = 1e-300, a + b, a + 1.0, a - 1.0
    c, d = 1.0, 1.0 - qab * x / qap
    if abs(d) < tiny:
        d = tiny
    d = 1.0 / d
    h = d
    for m in range(1, 1001):
        m2 = 2.0 * m
        aa = m * (b - m) * x / ((qam + m2) * (a + m2))
        d = 1.0 + aa * d
        if abs(d) < tiny:
            d = tiny
        c = 1.0 + aa / c
        if abs(c) < tiny:
            c = tiny
        d = 1.0 / d
        h *= d * c
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d = 1.0 + aa * d
        if abs(d) < tiny:
            d = tiny
        c = 1.0 + aa / c
        if abs(c) < tiny:
            c = tiny
        d = 1.0 / d
        de = d * c
        h *= de
        if abs(de - 1.0) < 1e-16:
            break
    return h


def student_t_two_sided(t, df):
    """P(|T| >= |t|) = I_x(df / 2, 1 / 2), x = df / (df + t^2): regularised incomplete beta by a Lentz continued fraction"""
    if t != t:
        return t
    t2 = t * t
    if t2 == math.inf:
        return 0.0
    if t2 == 0.0:
        return 1.0
    a, b = 0.5 * df, 0.5
    x, xc = df / (df + t2), t2 / (df + t2)
    front = t_coef(df) * math.exp(-a * math.log1p(t2 / df)) * math.sqrt(xc)
    if x < (a + 1.0) / (a + b + 2.0):
        return front * _beta_cf(a, b, x) / a
    return 1.0 - front * _beta_cf(b, a, xc) / b


def fit_row(h1, h2, y, cov, outcome="binary", mode="max", missing_cutoff=0.8, route="chol"):
    """One locus: (row as a dict of the fields of inq_assoc_row_t, last convergence criterion)."""
    y = np.asarray(y, dtype=np.float64)
    ns = len(y)
    cov = np.zeros((0, ns)) if cov is None else np.asarray(cov, dtype=np.float64).reshape(-1, ns)
    p = 2 + len(cov)
    x = predictor(h1, h2, mode)
    keep = ~np.isnan(x)
    n = int(keep.sum())
    xs, ys, cs = x[keep], y[keep], cov[:, keep]
    nan = math.nan
    row = dict(beta=nan, se=nan, stat=nan, p=nan, mean_all=nan, mean_g1=nan, mean_g2=nan, min_x=nan, max_x=nan, n=n, n_g1=0, n_g2=0,
               status=OK, n_iter=0)
    binary = outcome == "binary"
    with np.errstate(all="ignore"):
        if n:
            row["mean_all"], row["min_x"], row["max_x"] = xs.sum() / n, xs.min(), xs.max()
        if binary:
            g2 = ys != 0.0
            row["n_g1"], row["n_g2"] = int((~g2).sum()), int(g2.sum())
            if row["n_g1"]:
                row["mean_g1"] = xs[~g2].sum() / row["n_g1"]
            if row["n_g2"]:
                row["mean_g2"] = xs[g2].sum() / row["n_g2"]
        if ns == 0 or not n / ns >= missing_cutoff:
            row["status"] = LOW_CALL_RATE
        elif not row["min_x"] != row["max_x"]:
            row["status"] = CONSTANT
        elif binary and (not row["n_g1"] or not row["n_g2"]):
            row["status"] = ONE_GROUP
        elif n <= p:
            row["status"] = TOO_FEW
        elif not abs(xs.sum()) < math.inf:  # an infinite x: its centred column is not finite
            row["status"] = SINGULAR
        if row["status"] != OK:
            return row, nan

        X = np.column_stack([np.ones(n), xs] + [c for c in cs])
        Xc = X.copy()
        Xc[:, 1:] -= Xc[:, 1:].sum(axis=0) / n
        design = Xc if route == "chol" else X
        wls = (lambda w, z: _wls_chol(Xc, w, z)) if route == "chol" else (lambda w, z: _wls_qr(X, Xc, w, z))
        crit = nan
        if binary:
            beta, inv_xx, dev_old = None, nan, 0.0
            for t in range(MAX_ITER + 1):
                if t == 0:
                    mu = (ys + 0.5) * 0.5
                    eta = np.log(mu / (1.0 - mu))
                else:
                    eta = design @ beta
                    mu = np.clip(1.0 / (1.0 + np.exp(-eta)), MU_EPS, 1.0 - MU_EPS)
                dev = float((-2.0 * np.log(np.where(ys != 0.0, mu, 1.0 - mu))).sum())
                if t >= 1:
                    row["n_iter"] = t
                    if not abs(dev) < math.inf:
                        row["status"] = NOT_CONVERGED
                        break
                    crit = abs(dev - dev_old) / (abs(dev) + 0.1)
                    if crit < CONVERGED:
                        break
                    if t == MAX_ITER:
                        row["status"] = NOT_CONVERGED
                        break
                dev_old = dev
                w = mu * (1.0 - mu)
                got = wls(w, eta + (ys - mu) / w)
                if got is None:
                    row["status"], row["n_iter"] = SINGULAR, 0
                    return row, nan
                beta, inv_xx = got
            row["beta"], row["se"] = float(beta[1]), math.sqrt(inv_xx) if inv_xx >= 0 else nan
            row["stat"] = np.float64(row["beta"]) / np.float64(row["se"])
            row["p"] = math.erfc(abs(row["stat"]) * 0.70710678118654752440) if row["stat"] == row["stat"] else nan
        else:
            got = wls(np.ones(n), ys)
            if got is None:
                row["status"] = SINGULAR
                return row, nan
            beta, inv_xx = got
            res = ys - design @ beta
            df = n - p
            row["beta"] = float(beta[1])
            v = float(res @ res) / df * inv_xx
            row["se"] = math.sqrt(v) if v >= 0 else nan
            row["stat"] = float(np.float64(row["beta"]) / np.float64(row["se"]))
            row["p"] = student_t_two_sided(row["stat"], df)
        row["stat"] = float(row["stat"])
    return row, crit


def assoc_rows(values, y, cov=None, outcome="binary", mode="max", missing_cutoff=0.8, route="chol"):
    """values f32 [n_rows, 2 * n_samples] as inq_assoc_rows takes them -> (rows ROW_DTYPE [n_rows], criterion f64 [n_rows])"""
    values = np.asarray(values, dtype=np.float32)
    rows = np.zeros(len(values), dtype=ROW_DTYPE)
    crit = np.full(len(values), math.nan)
    for i, v in enumerate(values):
        r, crit[i] = fit_row(v[0::2], v[1::2], y, cov, outcome, mode, missing_cutoff, route)
        for k, val in r.items():
            rows[k][i] = val
    return rows, crit


def rel_diff(a, b):
    """largest |a - b| / max(|a|, |b|) over two arrays; equal values (NaN with NaN, inf with inf, 0 with 0) count 0, a NaN or an
    infinity on one side only counts inf"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        same = (a == b) | (np.isnan(a) & np.isnan(b))
        d = np.abs(a - b) / np.maximum(np.abs(a), np.abs(b))
        d = np.where(same, 0.0, np.where(np.isfinite(d), d, math.inf))
    return float(d.max()) if d.size else 0.0


def log_p(p):
    with np.errstate(all="ignore"):
        return np.log(np.asarray(p, dtype=np.float64))


FIT_FIELDS = ("beta", "se", "stat", "logp")


def route_disagreement(a, b):
    """largest relative disagreement of beta, se, stat, log(p) and the descriptive means between two sets of rows"""
    worst = 0.0
    for f in ("beta", "se", "stat", "mean_all", "mean_g1", "mean_g2", "min_x", "max_x"):
        worst = max(worst, rel_diff(a[f], b[f]))
    return max(worst, rel_diff(log_p(a["p"]), log_p(b["p"])))


def _exp(v):
    """exp as the C library computes it (the CLI's), inf on overflow"""
    try:
        return math.exp(v)
    except OverflowError:
        return math.inf


def render_text(rows, ids, outcome, phenotype, covariates=(), binary_order=None, all_rows=False, fmt=repr):
    """The text `inquistr assoc` prints for these rows: the tested loci (OK, NOT_CONVERGED) by ascending p, ties in file order, in the
    R script's columns; with all_rows the others behind them with their status name.  fmt: a float's text (inq_host_format_f64)."""
    model = phenotype + "~x" + "".join("+" + c for c in covariates)
    if outcome == "binary":
        a, b = binary_order
        head = ["VariantID", "OR", "OR_L95", "OR_U95", "OR_stdErr", "Pvalue", "N", f"{a}_N", f"{b}_N", "AvgSize", f"{a}_AvgSize",
                f"{b}_AvgSize", f"{b}_{a}_absAvgSizeDiff", f"{b}_{a}_OR_for_absAvgSizeDiff", "model", "binaryOrder"]
    else:
        head = ["VariantID", "Beta", "Beta_L95", "Beta_U95", "Beta_stdErr", "Pvalue", "N", "AvgSize", "MinSize", "MaxSize",
                "Max_Min_absSizeDiff", "Max_Min_Beta_for_absSizeDiff", "model"]
    if all_rows:
        head.append("status")
    tested = [i for i in range(len(rows)) if rows["status"][i] in (OK, NOT_CONVERGED)]
    tested.sort(key=lambda i: (math.isnan(rows["p"][i]), rows["p"][i] if not math.isnan(rows["p"][i]) else 0.0, i))
    order = tested + ([i for i in range(len(rows)) if rows["status"][i] not in (OK, NOT_CONVERGED)] if all_rows else [])
    out = ["\t".join(head)]
    with np.errstate(all="ignore"):
        for i in order:
            r = rows[i]
            beta, se = np.float64(r["beta"]), np.float64(r["se"])
            lo, hi = beta - Z95 * se, beta + Z95 * se
            if outcome == "binary":
                diff = np.abs(np.float64(r["mean_g2"]) - np.float64(r["mean_g1"]))
                cells = [ids[i], fmt(_exp(float(beta))), fmt(_exp(float(lo))), fmt(_exp(float(hi))), fmt(float(se)), fmt(float(r["p"])),
                         str(int(r["n"])), str(int(r["n_g1"])), str(int(r["n_g2"])), fmt(float(r["mean_all"])), fmt(float(r["mean_g1"])),
                         fmt(float(r["mean_g2"])), fmt(float(diff)), fmt(_exp(float(diff * beta))), model, f"{binary_order[0]},{binary_order[1]}"]
            else:
                diff = np.abs(np.float64(r["max_x"]) - np.float64(r["min_x"]))
                cells = [ids[i], fmt(float(beta)), fmt(float(lo)), fmt(float(hi)), fmt(float(se)), fmt(float(r["p"])), str(int(r["n"])),
                         fmt(float(r["mean_all"])), fmt(float(r["min_x"])), fmt(float(r["max_x"])), fmt(float(diff)), fmt(float(diff * beta)), model]
            if all_rows:
                cells.append(STATUS_NAMES[int(r["status"])])
            out.append("\t".join(cells))
    return "\n".join(out) + "\n"
