"""Inputs for the `inquistr assoc` tests, built on the CPU: cohort matrices as inq_assoc_rows takes them, with the restatement's rows of
both routes computed once per case (tests/assoc_restatement.py) and kept.

n_iter and the convergence band.  The kernel and the restatement stop on |dev - dev_old| / (|dev| + 0.1) < 1e-8; a row whose last
criterion lies within a factor 100 of 1e-8 may stop one step apart on the two, so the tests do not hold n_iter on such rows, and at
most 2 % of a case's rows may be such rows.  Newton's steps square the error, so with random rows about a third end in that band:
every ordinary row here is drawn again, by the restatement alone, until it ends outside it.  The constructed rows (separation, whose
criterion falls by 1 / e a step) are few enough to stay under the cap, which case() asserts."""
import functools
import math

import numpy as np

from tests import assoc_reference as rf
from tests import assoc_restatement as ar

FLOOR = 64 * 2.0 ** -52
BAND = (1e-10, 1e-6)
MODES = ("max", "min", "mean")


def in_band(crit):
    return bool(BAND[0] <= crit <= BAND[1])


def design(rng, ns, k, outcome):
    """y and covariates shared by every row: both groups there, a covariate that leans on y"""
    if outcome == "binary":
        y = (rng.random(ns) < 0.45).astype(np.float64)
        if ns >= 2:
            y[0], y[-1] = 0.0, 1.0
    else:
        y = np.round(rng.normal(50.0, 10.0, ns), 3)
    cov = np.round(rng.normal(0.0, 1.0, (k, ns)), 4)
    if k:
        cov[0] = np.round(cov[0] + 0.3 * (y - y.mean()) / (y.std() + 1e-9), 4)
    return y, cov


def ordinary_row(rng, y, outcome, eff=None):
    """H1 / H2 of a locus with a real effect of varying size (or of the size given): a base length, jitter, halves, 4 % missing
    haplotypes"""
    ns = len(y)
    base = float(rng.choice([8, 15, 31, 120, 400]))
    eff = rng.choice([0.0, 0.5, 1.0, 2.0, 4.0]) if eff is None else eff
    lean = (y - y.mean()) / (y.std() + 1e-9) if outcome == "continuous" else y
    h = base + rng.integers(-3, 4, (ns, 2)) + np.round(eff * lean)[:, None] * rng.integers(0, 2, (ns, 2))
    h = h + 0.5 * (rng.random((ns, 2)) < 0.1)
    h[rng.random((ns, 2)) < 0.04] = np.nan
    return h.reshape(-1).astype(np.float32)


class Case:
    """values, y, cov and what the restatement makes of them: want (route chol), alt (route qr), crit, tol, skip (rows in the band)"""

    def __init__(self, values, y, cov, outcome, mode, cutoff=0.8):
        self.values, self.y, self.cov, self.outcome, self.mode, self.cutoff = values, y, cov, outcome, mode, cutoff
        self.want, self.crit = ar.assoc_rows(values, y, cov, outcome, mode, cutoff, "chol")
        self.alt, _ = ar.assoc_rows(values, y, cov, outcome, mode, cutoff, "qr")
        # the two routes agree on every decision; where they do not the input sits on a threshold and is no test input
        assert np.array_equal(self.want["status"], self.alt["status"]), (self.want["status"].tolist(), self.alt["status"].tolist())
        self.disagreement = ar.route_disagreement(self.want, self.alt)
        self.tol = max(10.0 * self.disagreement, FLOOR)
        self.skip = np.array([in_band(c) for c in self.crit], dtype=bool)
        assert self.skip.sum() <= 0.02 * len(values), (int(self.skip.sum()), len(values))

    @functools.cached_property
    def fitted(self):
        return np.isin(self.want["status"], (ar.OK, ar.NOT_CONVERGED))

    @functools.cached_property
    def ref(self):
        """the long-double reference's rows (tests/assoc_reference.py), computed when first asked for"""
        return rf.assoc_rows(rf.REFERENCE, self.values, self.y, self.cov, self.outcome, self.mode, self.cutoff)

    @functools.cached_property
    def tol_row(self):
        """(tol_row, e_row, e_typ) of assoc_reference.tolerances from the two f64 routes' errors against the reference"""
        return rf.tolerances(rf.row_errors(self.want, self.ref, self.fitted), rf.row_errors(self.alt, self.ref, self.fitted), self.fitted)


def random_values(rng, n_rows, y, cov, outcome, mode, cutoff=0.8):
    rows = []
    for _ in range(n_rows):
        for _ in range(40):
            v = ordinary_row(rng, y, outcome)
            if outcome != "binary":
                break
            _, crit = ar.fit_row(v[0::2], v[1::2], y, cov, outcome, mode, cutoff, "chol")
            if not in_band(crit):
                break
        rows.append(v)
    return np.array(rows, dtype=np.float32).reshape(n_rows, 2 * len(y))


@functools.lru_cache(maxsize=None)
def case(seed, n_rows, ns, k, outcome, mode):
    rng = np.random.default_rng(seed)
    y, cov = design(rng, ns, k, outcome)
    return Case(random_values(rng, n_rows, y, cov, outcome, mode), y, cov, outcome, mode)


SPECIAL_NS = 130  # three steps of a wave: samples 0 .. 63, 64 .. 127, 128 and 129
SPECIAL_NAMES = ("nan_lane0", "nan_lane63", "nan_last", "nan_one_haplotype", "nan_everywhere", "constant", "two_values", "one_group",
                 "separated", "quasi_separated", "near_10000", "inf_h1", "low_call_rate", "inf_both")


@functools.lru_cache(maxsize=None)
def special_case(outcome, mode):
    """The constructed rows (SPECIAL_NAMES, in this order) in front of 100 ordinary ones, at a call-rate cutoff of 0.3 so that a group
    wiped out by NaNs is what stops its row"""
    rng = np.random.default_rng(1234)
    ns = SPECIAL_NS
    y, cov = design(rng, ns, 1, outcome)
    if outcome == "binary":
        y[:] = 0.0
        y[rng.choice(ns, 40, replace=False)] = 1.0  # 31 % in group 2: without them the call rate is still 0.69
    hi = y > np.median(y) if outcome == "continuous" else y != 0.0
    rows = {}

    def fresh():
        return ordinary_row(rng, y, outcome).astype(np.float64).reshape(ns, 2)

    for name, at in (("nan_lane0", 0), ("nan_lane63", 63), ("nan_last", ns - 1)):
        h = fresh()
        h[at] = np.nan
        rows[name] = h
    h = fresh()
    h[::3, 0] = np.nan
    h[1::3, 1] = np.nan
    rows["nan_one_haplotype"] = h
    rows["nan_everywhere"] = np.full((ns, 2), np.nan)
    rows["constant"] = np.full((ns, 2), 17.0)
    h = np.full((ns, 2), 17.0)
    h[rng.random(ns) < 0.4] = 19.0
    rows["two_values"] = h
    h = fresh()
    h[hi] = np.nan
    rows["one_group"] = h
    h = 10.0 + rng.integers(0, 4, (ns, 2)).astype(np.float64)
    h[hi] += 8.0
    rows["separated"] = h
    h = 10.0 + rng.integers(0, 4, (ns, 2)).astype(np.float64)
    h[hi] += 3.0  # the groups meet at 13
    h[np.argmax(hi)] = 13.0
    h[np.argmin(hi)] = 13.0
    rows["quasi_separated"] = h
    h = 10000.0 + rng.integers(0, 2, (ns, 2)).astype(np.float64) + (hi & (rng.random(ns) < 0.5))[:, None]
    rows["near_10000"] = h
    h = fresh()
    h[5, 0] = np.inf
    rows["inf_h1"] = h
    h = fresh()
    h[rng.choice(ns, 100, replace=False)] = np.nan  # 30 of 130 left: 0.23 < 0.3
    rows["low_call_rate"] = h
    h = fresh()
    h[7] = (np.inf, -np.inf)
    rows["inf_both"] = h
    special = np.array([rows[n].reshape(-1) for n in SPECIAL_NAMES], dtype=np.float32)
    ordinary = random_values(rng, 100, y, cov, outcome, mode, 0.3)
    return Case(np.concatenate([special, ordinary]), y, cov, outcome, mode, 0.3)


@functools.lru_cache(maxsize=None)
def collinear_case(outcome, noise):
    """One covariate that IS row 0's x (noise 0) or that plus noise of 1e-9: row 0 is rank deficient, the rows behind it are not"""
    rng = np.random.default_rng(77)
    ns = 90
    y, _ = design(rng, ns, 0, outcome)
    values = random_values(rng, 12, y, np.zeros((0, ns)), outcome, "max")
    values[0] = np.nan_to_num(values[0], nan=20.0)
    cov = ar.predictor(values[0, 0::2], values[0, 1::2], "max")[None, :].copy()
    if noise:
        cov += noise * rng.normal(size=ns)
    for i in range(1, 12):  # the covariate changes the fits: draw the other rows again until they end outside the band
        for _ in range(40):
            _, crit = ar.fit_row(values[i, 0::2], values[i, 1::2], y, cov, outcome, "max", 0.8, "chol")
            if not in_band(crit):
                break
            values[i] = ordinary_row(rng, y, outcome)
    return Case(values, y, cov, outcome, "max")


def compare(case_, got):
    """The device's rows against the restatement's: what is exact, and the largest error of the rest as a share of the tolerance"""
    want = case_.want
    for f in ("status", "n", "n_g1", "n_g2"):
        assert np.array_equal(got[f], want[f]), (f, np.nonzero(got[f] != want[f])[0][:8].tolist(), got[f][:8].tolist(), want[f][:8].tolist())
    for f in ("min_x", "max_x"):
        assert np.array_equal(got[f], want[f], equal_nan=True), f
    hold = ~case_.skip
    assert np.array_equal(got["n_iter"][hold], want["n_iter"][hold]), (got["n_iter"].tolist(), want["n_iter"].tolist())
    worst = ar.route_disagreement(got, want)
    ratio = worst / case_.tol
    print(f"assoc device-vs-restatement: worst relative difference {worst:.3e}, tolerance {case_.tol:.3e} "
          f"(routes disagree by {case_.disagreement:.3e}), ratio {ratio:.3f}")
    assert worst <= case_.tol, (worst, case_.tol)
    compare_rows(case_, got)
    compare_p(case_, got)
    return ratio


def compare_rows(case_, got, what="device"):
    """Every fitted row's scaled error against the long-double reference, held to that row's own tolerance
    (tests/assoc_reference.py: row_errors, tolerances).  -> the worst share of a tolerance"""
    tol, e_row, e_typ = case_.tol_row
    err = rf.row_errors(got, case_.ref, case_.fitted)
    share, i = rf.worst_share(err, tol, case_.fitted)
    typical = case_.fitted & (e_row <= e_typ)
    print(f"assoc {what}-vs-long-double per row: worst share {share:.3f} of its tolerance at row {i} (error {err[max(i, 0)]:.2e}, "
          f"tolerance {tol[max(i, 0)]:.2e}); tolerances {tol[case_.fitted].min() if case_.fitted.any() else 0:.2e} .. "
          f"{tol[case_.fitted].max() if case_.fitted.any() else 0:.2e}; largest error on the ordinary rows "
          f"{err[typical].max() if typical.any() else 0:.2e}, the f64 routes' there {e_row[typical].max() if typical.any() else 0:.2e}")
    bad = np.nonzero(err > tol)[0]
    assert not len(bad), (what, bad[:8].tolist(), err[bad[:8]].tolist(), tol[bad[:8]].tolist())
    return share


def host_p(case_, got):
    """the p-value the host's functions give for the statistic `got` carries: erfc(|z| / sqrt 2), or Student's t at n - p"""
    p = 2 + (0 if case_.cov is None else len(case_.cov))
    out = np.full(len(got["stat"]), math.nan)
    for i in np.nonzero(case_.fitted)[0]:
        s = float(got["stat"][i])
        if s == s:
            out[i] = (math.erfc(abs(s) / math.sqrt(2.0)) if case_.outcome == "binary"
                      else ar.student_t_two_sided(s, int(got["n"][i]) - p))
    return out


def compare_p(case_, got, what="device"):
    """p as a function of the statistic beside it (assoc_reference.check_p)"""
    if case_.outcome == "binary":
        allowed = np.full(len(got["p"]), rf.p_allowed(rf.P_UNITS_ERFC))
    else:  # by each row's own df = n - p; a row that is not fitted has no p and is not asked
        p = 2 + (0 if case_.cov is None else len(case_.cov))
        allowed = np.array([rf.p_allowed(rf.p_units_t(max(int(n) - p, 1))) for n in got["n"]])
    share, units = rf.check_p(got["p"], host_p(case_, got), what, allowed)
    print(f"assoc {what} p against the host's function of its own statistic: {units:.1f} units of 2^-52 max(1, |log p|), "
          f"{share:.4f} of what its row is allowed ({allowed.min() if len(allowed) else 0:.0f} .. {allowed.max() if len(allowed) else 0:.0f} units)")
    return share


# ---- the inputs of tests/test_gpu_assoc_edges.py --------------------------------------------------------------------------------

T_DF = (1, 2, 3, 61, 126, 298)
T_K = (0, 1, 6)


def t_targets(df):
    """the |t| a prescribed-t case has a row for; the 8th and 9th lie on the two sides of x < (a + 1) / (a + b + 2), where
    student_t_two_sided changes continued fractions (x = df / (df + t^2), a = df / 2, b = 1 / 2: t^2 = 3 df / (df + 2))"""
    s = math.sqrt(3.0 * df / (df + 2.0))
    return (1e-8, 1e-3, 0.5, 1.0, 1.5, 0.98 * s, 1.02 * s, 2.0, 3.0, 5.0, 8.0, 12.0, 20.0, 30.0, 37.0, 38.0, 39.0, 60.0, 1e3, 1e6)


def cf_branch(t, df):
    """does student_t_two_sided take the fraction in x (True) or the one in 1 - x"""
    a, b = 0.5 * df, 0.5
    return df / (df + t * t) < (a + 1.0) / (a + b + 2.0)


def _unit(v):
    return v / np.sqrt((v * v).sum())


@functools.lru_cache(maxsize=None)
def prescribed_t_case(df, k):
    """Continuous, n_samples = df + p, one row per t_targets(df), the signs of the slope alternating.  y and the covariates are
    shared by the rows, so each row's x is built for its t: with yr the unit residual of y on [1, covariates] and e a unit vector
    orthogonal to those and to yr (all in long double), x = 30 + 4 sqrt(ns) (r yr + sqrt(1 - r^2) e) has the partial correlation r
    and t = r sqrt(df / (1 - r^2)).  Rounding x to f32 moves r by about 1e-8, so the reference's own t is read back and r corrected
    (a small t: e drawn again) until it is within 5 % of the target; that every target was met and that both continued fractions
    are reached is asserted here."""
    LD = np.longdouble
    rng = np.random.default_rng(4100 + 10 * df + k)
    p = 2 + k
    ns = df + p
    y, cov = design(rng, ns, k, "continuous")
    basis = []
    for c in [np.ones(ns, LD)] + [c.astype(LD) for c in cov]:  # Gram-Schmidt, twice
        for _ in range(2):
            for q in basis:
                c = c - (c @ q) * q
        basis.append(_unit(c))

    def off(v, more=()):
        for _ in range(2):
            for q in list(basis) + list(more):
                v = v - (v @ q) * q
        return _unit(v)

    yr = off(y.astype(LD))
    Q = np.array(basis)

    def t_of(X):
        """the t of each row of X [c, ns] against y beside [1, covariates], the residual taken without 1 - r^2"""
        for _ in range(2):
            X = X - (X @ Q.T) @ Q
        along = X @ yr
        rest = X - along[:, None] * yr
        return along / np.sqrt((rest * rest).sum(axis=1) / df)

    rows = []
    for i, target in enumerate(t_targets(df)):
        sign, want = (-1) ** i, LD(target)
        e = off(rng.normal(size=ns).astype(LD), (yr,))
        for attempt in range(60):
            # 2000 scales of one direction: the same t but for the rounding to f32, which is what a small t is made of
            r, rc = want / np.sqrt(df + want ** 2), np.sqrt(df / (df + want ** 2))
            scale = 4 * np.sqrt(LD(ns)) * (1 + rng.random(2000).astype(LD) / 4)
            X = (30 + scale[:, None] * (sign * r * yr + rc * e)).astype(np.float32)
            t = t_of(X.astype(LD)) * sign
            miss = np.where(t > 0, np.abs(np.log(np.where(t > 0, t, 1) / target)), np.inf)
            best = int(np.argmin(miss))
            if miss[best] <= 0.03:
                break
            typical = np.median(t)
            if typical > 0:
                want = want * target / typical
            else:
                want, e = LD(target), off(rng.normal(size=ns).astype(LD), (yr,))
        rows.append(np.repeat(X[best], 2))
    out = Case(np.array(rows, dtype=np.float32), y, cov, "continuous", MODES[(df + k) % 3])
    out.t_ref = np.array(out.ref["stat"], dtype=np.float64)
    assert (out.want["status"] == ar.OK).all()
    assert np.all(np.abs(np.abs(out.t_ref) / np.array(t_targets(df)) - 1.0) <= 0.05), (out.t_ref.tolist(), t_targets(df))
    assert {cf_branch(t, df) for t in out.t_ref} == {True, False}
    assert cf_branch(out.t_ref[5], df) != cf_branch(out.t_ref[6], df)
    return out


@functools.lru_cache(maxsize=None)
def limit_case(ns, k, outcome):
    """n_samples at its limit of 65 535 (and 4096): 5 rows, one more than a workgroup; the mode goes round with the case"""
    return case(5000 + ns % 1000 + k, 5, ns, k, outcome, MODES[(ns + k + (outcome == "binary")) % 3])


Z_TARGETS = tuple(float(z) for z in range(0, 37, 3)) + (38.0, 42.0, 45.0)
Z_NS = 8192


def shifted_halves(rng, y, target, measure, in_band_, top):
    """x ~ N(0, 1) + d y rounded to halves, d bisected in [0, top] until measure(values) is within 0.25 of target (target 0: d = 0,
    whatever comes): the row as H1 / H2.  Whether such a fit ends in the convergence band is a matter of the size of the effect
    far more than of the draw, so a row that does is drawn again with the shift given to a part of group 2 only and half of the
    samples' noise wider or narrower, which changes the path the iteration takes to the same statistic."""
    for attempt in range(60):
        noise = rng.normal(size=len(y)) * np.where(rng.random(len(y)) < 0.5, 1.0 if attempt == 0 else rng.uniform(0.5, 2.2), 1.0)
        part = y * (rng.random(len(y)) < (1.0 if attempt == 0 else rng.uniform(0.7, 1.0)))
        make = lambda d: np.repeat(np.round(2.0 * (noise + d * part)) / 2.0, 2).astype(np.float32)
        lo, hi = 0.0, top
        v = make(0.0)
        if target:
            for _ in range(60):
                d = 0.5 * (lo + hi)
                v = make(d)
                m = measure(v)
                if abs(m - target) <= 0.25:
                    break
                lo, hi = (d, hi) if m < target else (lo, d)
            else:
                continue
        if not in_band_(v):
            return v
    raise AssertionError(("no row for", target))


@functools.lru_cache(maxsize=None)
def wald_case():
    """Binary, 8192 samples, no covariate: 16 rows whose Wald |z| runs from 0 to 45, so that erfc is followed through its last normal
    values (|z| > 30), a denormal one (37.6 < |z| < 38.4) and 0"""
    rng = np.random.default_rng(4300)
    y = (rng.random(Z_NS) < 0.35).astype(np.float64)
    cov = np.zeros((0, Z_NS))
    fit = lambda v: ar.fit_row(v[0::2], v[1::2], y, cov, "binary", "max", 0.8, "chol")
    # Wald's z falls again beyond d = 2 (the standard error outgrows the estimate): the search stays on the rising side
    rows = [shifted_halves(rng, y, z, lambda v: abs(fit(v)[0]["stat"]), lambda v: in_band(fit(v)[1]), 2.0) for z in Z_TARGETS]
    out = Case(np.array(rows, dtype=np.float32), y, cov, "binary", "max")
    z, p = np.abs(np.array(out.ref["stat"], dtype=np.float64)), out.ref["p"]
    assert (out.want["status"] == ar.OK).all() and z.min() < 1.5 and z.max() > 44.0 and np.all(np.diff(np.sort(z)) < 4.5), z.tolist()
    assert ((z > 30.0) & (p >= rf.P_MIN_NORMAL)).sum() >= 2 and ((p > 0.0) & (p < rf.P_MIN_NORMAL)).any() and (p == 0.0).any(), p.tolist()
    return out


@functools.lru_cache(maxsize=None)
def empty_case(ns, outcome):
    """n_samples 0 and 1: three rows, a value in both haplotypes, in one, in none"""
    y = np.array([1.0, 0.0][:ns])
    values = np.array([[7.0, 7.5], [np.nan, 9.0], [np.nan, np.nan]], dtype=np.float32)[:, :2 * ns]
    return Case(values, y, None if ns == 0 else np.zeros((0, ns)), outcome, "max")  # no covariate: [0, 0] is no shape to reshape to


INVARIANCE_NS = 129


@functools.lru_cache(maxsize=None)
def invariance_case(outcome):
    """129 samples, 2 covariates: 49 ordinary rows and, last, special_case's `separated`, whose criterion falls by 1 / e a step and
    ends in the convergence band: 50 rows, so that it is the one row in 50 that may"""
    rng = np.random.default_rng(4600)
    ns = INVARIANCE_NS
    y, cov = design(rng, ns, 2, outcome)
    hi = y > np.median(y) if outcome == "continuous" else y != 0.0
    h = 10.0 + rng.integers(0, 4, (ns, 2)).astype(np.float64)
    h[hi] += 8.0
    values = np.concatenate([random_values(rng, 49, y, cov, outcome, "max"), h.reshape(1, -1).astype(np.float32)])
    return Case(values, y, cov, outcome, "max")


def derived_case(c, values=None, y=None, cov=None, cutoff=None):
    """c with some of its inputs replaced, and c's reference and tolerances: for inputs that must give c's rows again"""
    out = Case(c.values if values is None else values, c.y if y is None else y, c.cov if cov is None else cov, c.outcome, c.mode,
               c.cutoff if cutoff is None else cutoff)
    out.ref, out.tol_row, out.fitted = c.ref, c.tol_row, c.fitted
    return out


def permuted(c, seed=1):
    """c's samples in another order: values, y and covariates together"""
    perm = np.random.default_rng(seed).permutation(len(c.y))
    v = c.values.reshape(len(c.values), -1, 2)[:, perm].reshape(len(c.values), -1)
    return derived_case(c, np.ascontiguousarray(v), c.y[perm], c.cov[:, perm])


def shifted(c, pad=65):
    """c with `pad` samples without a value in front, which moves every sample by a lane and a stride, and the cutoff lowered to
    what it was of c's n_samples"""
    ns = len(c.y)
    v = np.concatenate([np.full((len(c.values), 2 * pad), np.nan, dtype=np.float32), c.values], axis=1)
    y = np.concatenate([np.arange(pad) % 2 if c.outcome == "binary" else np.full(pad, 1e6), c.y]).astype(np.float64)
    cov = np.concatenate([np.full((len(c.cov), pad), -1e6), c.cov], axis=1)
    return derived_case(c, v, y, cov, c.cutoff * ns / (ns + pad))


def edge_cases():
    """(name, case) of everything tests/test_gpu_assoc_edges.py compares with a reference, for tests/test_assoc_reference.py"""
    for df in T_DF:
        for k in T_K:
            yield f"prescribed t df {df} k {k}", prescribed_t_case(df, k)
    for ns in (65535, 4096):
        for k in (0, 6):
            for o in ("binary", "continuous"):
                yield f"limit ns {ns} k {k} {o}", limit_case(ns, k, o)
    yield "wald", wald_case()
    for o in ("binary", "continuous"):
        for ns in (0, 1):
            yield f"empty ns {ns} {o}", empty_case(ns, o)
        yield f"invariance {o}", invariance_case(o)
