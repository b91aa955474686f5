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


def ordinary_row(rng, y, outcome):
    """H1 / H2 of a locus with a real effect of varying size: a base length, jitter, halves, 4 % missing haplotypes"""
    ns = len(y)
    base = float(rng.choice([8, 15, 31, 120, 400]))
    eff = rng.choice([0.0, 0.5, 1.0, 2.0, 4.0])
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
    return ratio
