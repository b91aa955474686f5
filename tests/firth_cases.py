"""Inputs for the inq_assoc_rows_firth tests, built on the CPU beside tests/assoc_cases.py: cohort matrices with the restatement's
rows of both routes computed once per case (tests/firth_restatement.py) and kept.

Iteration counts and the convergence band.  The kernel and the restatement stop on max_j |delta_j| sqrt(I_jj) < 1e-9.  Convergence
is linear, so a random row's last or last-but-one criterion lies within 1 % of 1e-9 about 2 % of the time, and such a row may stop a
step apart on the device: its counts are not held.  Every ordinary row here is drawn again, by the restatement alone, until both of
its fits end outside that band; the constructed rows cannot be, and Case asserts that at most 2 % of a case's rows are such rows and
that the restatement's two routes stop at the same step on every row.

chi2 and its relative error.  chi2 = 2 (l*_full - l*_null) is a difference: one unit in the last place of an l* moves it by
2 eps |l*| / chi2 of itself, whoever computes it.  The tolerance is relative and one number per case, so a row with chi2 = 1e-4
beside l* = -40 would set it (or miss it, where the routes happen to round alike there) by what a single rounding of l* does, a
million times what the kernel is held to in every other field.  An ordinary row is drawn again until chi2 >= |l*_full| / 8: a unit
in the last place of l* is then at most 16 eps of chi2, a quarter of the tolerance's floor.  That leaves out the rows without an
effect; what Firth's fit makes of those is held by the constructed cases, whose 100 ordinary rows are assoc_cases' own."""
import functools

import numpy as np

from tests import assoc_cases as ac
from tests import assoc_restatement as ar
from tests import firth_restatement as fr

FLOOR = ac.FLOOR
WHENS = ("fallback", "always")


class Case:
    """values, y, cov, mode, cutoff and R: what the restatement makes of them (firth_restatement.Rows)"""

    def __init__(self, values, y, cov, mode, cutoff=0.8):
        self.values, self.y, self.cov, self.mode, self.cutoff = values, y, cov, mode, cutoff
        self.R = R = fr.Rows(values, y, cov, mode, cutoff)
        # the two routes agree on every decision and stop at the same step; where they do not the input sits on a threshold and is no
        # test input
        for f in ("status", "n_iter_full", "n_iter_null"):
            assert np.array_equal(R.chol[f], R.qr[f]), (f, R.chol[f].tolist(), R.qr[f].tolist())
        self.skip = R.band
        assert self.skip.sum() <= 0.02 * len(values), (int(self.skip.sum()), len(values))

    def tol(self, when):
        """10 x the routes' largest relative disagreement on the rows `when` fits, never below 64 * 2^-52"""
        d = fr.disagreement(self.R.want(when, "chol"), self.R.want(when, "qr"))
        return max(10.0 * d, FLOOR), d


def random_values(rng, n_rows, y, cov, mode):
    rows = []
    for _ in range(n_rows):
        for _ in range(40):
            v = ac.ordinary_row(rng, y, "binary")
            row, _ = ar.fit_row(v[0::2], v[1::2], y, cov, "binary", mode, 0.8, "chol")
            if row["status"] not in (ar.OK, ar.NOT_CONVERGED):
                break
            firth, fits = fr.fit_row(v[0::2], v[1::2], y, cov, mode, "chol")
            if not fr.in_band(fits) and (firth["status"] != fr.OK or firth["chi2"] >= abs(firth["pll_full"]) / 8.0):
                break
        rows.append(v)
    return np.array(rows, dtype=np.float32).reshape(n_rows, 2 * len(y))


@functools.lru_cache(maxsize=None)
def case(seed, n_rows, ns, k, mode):
    rng = np.random.default_rng(seed)
    y, cov = ac.design(rng, ns, k, "binary")
    return Case(random_values(rng, n_rows, y, cov, mode), y, cov, mode)


@functools.lru_cache(maxsize=None)
def special_case(mode):
    """assoc_cases.special_case's matrix (its constructed rows in front of 100 ordinary ones, one covariate, cutoff 0.3).  Its ordinary
    rows were drawn for the ordinary fit's band, not for this one; the cap of 2 % holds them too.  The fallback rule must not sit on
    its bound here: no row's smallest min(mu, 1 - mu) lies in [1e-7, 1e-5]."""
    c = ac.special_case("binary", mode)
    out = Case(c.values, c.y, c.cov, mode, c.cutoff)
    m = out.R.min_mu
    assert not ((m >= 1e-7) & (m <= 1e-5)).any(), m[(m >= 1e-7) & (m <= 1e-5)].tolist()
    return out


@functools.lru_cache(maxsize=None)
def collinear_case():
    """A covariate that is 1000 x row 0's x plus noise of a tenth of x's spread: 1 - r^2 = 1e-8.  A covariate that IS x makes the
    ordinary fit SINGULAR, and Firth's is then never tried.  This one passes the ordinary fit's rank test and fails Firth's, because
    a Cholesky pivot is measured against the largest diagonal and the two kernels order their columns differently: the ordinary fit
    ([1, x, cov]) ends on the covariate's pivot, 1e-8 of the largest diagonal (the covariate's own); Firth's ([1, cov, x]) ends on
    x's, which is 1e-6 of that again, 1e-14 against the bound of 1e-11, three orders clear on either side.  Row 0 is SINGULAR in
    Firth's fit, rows 1 .. 11 (another x) are ordinary."""
    rng = np.random.default_rng(78)
    ns = 90
    y, _ = ac.design(rng, ns, 0, "binary")
    x0 = np.nan_to_num(ac.ordinary_row(rng, y, "binary"), nan=20.0)
    px = ar.predictor(x0[0::2], x0[1::2], "max")
    cov = (1000.0 * px + rng.normal(0.0, 0.1 * px.std(), ns))[None, :]
    values = np.concatenate([x0[None, :], random_values(rng, 11, y, cov, "max")])
    return Case(values, y, cov, "max")


def compare(case_, when, rows, firth, ordinary):
    """The device's rows under `when` against inq_assoc_rows' bytes and the restatement: what is exact, and the largest error of the
    rest as a share of the tolerance"""
    assert rows.tobytes() == ordinary.tobytes()
    want = case_.R.want(when)
    assert np.array_equal(firth["status"], want["status"]), (np.nonzero(firth["status"] != want["status"])[0][:8].tolist(),
                                                              firth["status"][:16].tolist(), want["status"][:16].tolist())
    assert np.array_equal(firth["status"] != fr.NOT_FITTED, case_.R.fitted(when))
    assert not firth["pad"].any()
    hold = ~case_.skip
    for f in ("n_iter_full", "n_iter_null"):
        assert np.array_equal(firth[f][hold], want[f][hold]), (f, firth[f].tolist(), want[f].tolist())
    tol, d = case_.tol(when)
    worst = fr.disagreement(firth, want)
    ratio = worst / tol
    each = " ".join(f"{f} {ar.rel_diff(firth[f], want[f]):.1e}" for f in fr.FIT_FIELDS)
    print(f"firth device-vs-restatement ({when}): worst relative difference {worst:.3e}, tolerance {tol:.3e} "
          f"(routes disagree by {d:.3e}), ratio {ratio:.3f} [{each}]")
    assert worst <= tol, (worst, tol)
    return ratio
