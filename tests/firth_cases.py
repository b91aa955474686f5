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
effect here; compare()'s per-row check holds chi2 at the scale of l* instead (tests/assoc_reference.py: firth_row_errors), and
no_effect_case below is made of such rows."""
import functools
import math

import numpy as np

from tests import assoc_cases as ac
from tests import assoc_reference as rf
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

    @functools.cached_property
    def ref(self):
        """the long-double reference's Firth rows of every row the ordinary fit lets through (tests/assoc_reference.py)"""
        return rf.firth_rows(rf.REFERENCE, self.values, self.y, self.cov, self.mode, self.cutoff)

    @functools.lru_cache(maxsize=None)
    def tol_row(self, when):
        """(tol_row, e_row, e_typ) of assoc_reference.tolerances over the rows `when` fits"""
        fitted = self.R.fitted(when)
        return rf.tolerances(rf.firth_row_errors(self.R.chol, self.ref, fitted), rf.firth_row_errors(self.R.qr, self.ref, fitted), fitted)


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
    compare_rows(case_, when, firth)
    compare_p(case_, when, firth)
    return ratio


def compare_rows(case_, when, firth, what="device"):
    """Every fitted row's scaled error against the long-double reference, held to that row's own tolerance
    (tests/assoc_reference.py: firth_row_errors, tolerances).  -> the worst share of a tolerance"""
    fitted = case_.R.fitted(when)
    tol, e_row, e_typ = case_.tol_row(when)
    err = rf.firth_row_errors(firth, case_.ref, fitted)
    share, i = rf.worst_share(err, tol, fitted)
    typical = fitted & (e_row <= e_typ)
    print(f"firth {what}-vs-long-double per row ({when}): worst share {share:.3f} of its tolerance at row {i} (error {err[max(i, 0)]:.2e}, "
          f"tolerance {tol[max(i, 0)]:.2e}); tolerances {tol[fitted].min() if fitted.any() else 0:.2e} .. "
          f"{tol[fitted].max() if fitted.any() else 0:.2e}; largest error on the ordinary rows "
          f"{err[typical].max() if typical.any() else 0:.2e}, the f64 routes' there {e_row[typical].max() if typical.any() else 0:.2e}")
    bad = np.nonzero(err > tol)[0]
    assert not len(bad), (what, when, bad[:8].tolist(), err[bad[:8]].tolist(), tol[bad[:8]].tolist())
    return share


def compare_p(case_, when, firth, what="device"):
    """p as erfc(sqrt(chi2 / 2)) of the chi2 beside it (assoc_reference.check_p)"""
    host = np.array([math.erfc(math.sqrt(c / 2.0)) if c == c else math.nan for c in firth["chi2"].tolist()])
    allowed = rf.p_allowed(rf.P_UNITS_ERFC)
    share, units = rf.check_p(firth["p"], host, f"{what} {when}", allowed)
    print(f"firth {what} p against the host's erfc of its own chi2 ({when}): {units:.1f} units of 2^-52 max(1, |log p|), "
          f"{allowed:.0f} allowed")
    return share


# ---- the inputs of tests/test_gpu_firth_edges.py ----------------------------------------------------------------------------------

def _in_band(v, y, cov, mode):
    return fr.in_band(fr.fit_row(v[0::2], v[1::2], y, cov, mode, "chol")[1])


@functools.lru_cache(maxsize=None)
def chi2_case():
    """assoc_cases.wald_case for the likelihood ratio: 8192 samples, no covariate, 16 rows whose sqrt(chi2) runs from 0 to 45.  The
    search reads chi2 and the criteria off the wave-order route, which costs a hundredth of the restatement here; that no row
    ends in the band is the restatement's to say, in Case"""
    rng = np.random.default_rng(4301)
    y = (rng.random(ac.Z_NS) < 0.35).astype(np.float64)
    cov = np.zeros((0, ac.Z_NS))
    root = lambda v: math.sqrt(float(rf.firth_fit_row(rf.WAVE, v[0::2], v[1::2], y, cov, "max")["chi2"]))

    def band(v):
        fits = []
        rf.firth_fit_row(rf.WAVE, v[0::2], v[1::2], y, cov, "max", fits)
        return fr.in_band(fits)

    rows = [ac.shifted_halves(rng, y, z, root, band, 3.0) for z in ac.Z_TARGETS]
    out = Case(np.array(rows, dtype=np.float32), y, cov, "max")
    z, p = np.sqrt(np.array(out.ref["chi2"], dtype=np.float64)), out.ref["p"]
    assert (out.R.chol["status"] == fr.OK).all() and z.min() < 1.5 and z.max() > 44.0 and np.all(np.diff(np.sort(z)) < 4.5), z.tolist()
    assert ((z > 30.0) & (p >= rf.P_MIN_NORMAL)).sum() >= 2 and ((p > 0.0) & (p < rf.P_MIN_NORMAL)).any() and (p == 0.0).any(), p.tolist()
    return out


@functools.lru_cache(maxsize=None)
def no_effect_case():
    """What most loci of a real file are: 24 rows of ordinary_row without an effect (129 samples, one covariate; drawn again only
    for the convergence band, not for the size of chi2), and a 25th that is symmetric between the groups - samples 2 j and 2 j + 1
    share y and the covariate and carry x = 20 + d and 20 - d, the last one x = 20 - so that beta_x = 0 solves the full fit's
    equations exactly, the two fits are one and chi2 is whatever the roundings of two l* leave: the device may give 0 there."""
    rng = np.random.default_rng(4400)
    ns = 129
    y, cov = ac.design(rng, 64, 1, "binary")
    y, cov = np.concatenate([np.repeat(y, 2), [1.0]]), np.concatenate([np.repeat(cov, 2, axis=1), [[0.25]]], axis=1)
    rows = []
    for _ in range(24):
        for _ in range(40):
            v = ac.ordinary_row(rng, y, "binary", eff=0.0)
            o, _ = ar.fit_row(v[0::2], v[1::2], y, cov, "binary", "max", 0.8, "chol")
            if o["status"] not in (ar.OK, ar.NOT_CONVERGED):
                continue  # a row a filter stops is no row of this case
            if not _in_band(v, y, cov, "max"):
                break
        else:
            raise AssertionError("no fitted row outside the band in 40 draws")
        rows.append(v)
    d = rng.integers(1, 6, 64).astype(np.float64)
    x = np.concatenate([np.stack([20.0 + d, 20.0 - d], axis=1).reshape(-1), [20.0]])
    rows.append(np.repeat(x, 2).astype(np.float32))
    out = Case(np.array(rows, dtype=np.float32), y, cov, "max")
    ref = out.ref
    assert (out.R.chol["status"] == fr.OK).all()
    assert ref["chi2"][24] < 1e-12 * abs(ref["pll_full"][24]), (ref["chi2"][24], ref["pll_full"][24])
    small = np.array(ref["chi2"][:24] < np.abs(ref["pll_full"][:24]) / 8.0)
    assert small.sum() >= 20, small.tolist()  # the rows random_values would have drawn again
    return out


@functools.lru_cache(maxsize=None)
def empty_case(ns):
    c = ac.empty_case(ns, "binary")
    return Case(c.values, c.y, c.cov, "max")


@functools.lru_cache(maxsize=None)
def invariance_case():
    c = ac.invariance_case("binary")
    return Case(c.values, c.y, c.cov, "max")


def derived_case(c, d):
    """d (assoc_cases.permuted / shifted of the ordinary case) as a Firth case with c's reference and tolerances"""
    out = Case(d.values, d.y, d.cov, d.mode, d.cutoff)
    out.ref, out.tol_row = c.ref, c.tol_row
    return out


def edge_cases():
    """(name, case, whens) of everything tests/test_gpu_firth_edges.py compares with a reference"""
    yield "chi2", chi2_case(), ("always",)
    yield "no effect", no_effect_case(), WHENS
    for ns in (0, 1):
        yield f"empty ns {ns}", empty_case(ns), WHENS
    yield "invariance", invariance_case(), ("always",)
