"""`inquistr assoc` on the GPU through the C ABI (inq_assoc_rows) against the restatement (tests/assoc_restatement.py, pinned without a
GPU by tests/test_assoc_restatement.py), on the shapes where a wave-per-locus kernel can go wrong.

Integers, statuses, min / max and the filter decisions are exact.  beta, se, stat, log(p) and the means are held, per case, to 10 x
the largest relative disagreement of the restatement's QR route and its Cholesky route on that same input, never below 64 * 2^-52
(tests/assoc_cases.py computes it on the CPU; the factor 10 covers the wave's order of summation, which is neither route's: a
choice, not a measurement).  n_iter is exact except on rows whose last convergence criterion lies within a factor 100 of 1e-8, at
most 2 % of a case's rows (asserted when the case is built).  Every test prints the share of the tolerance it used.

That one tolerance is set by the case's worst-conditioned row (and was 10, i.e. nothing, where one row's beta is 0), so compare()
also holds every fitted row to a tolerance of its own, against a long-double fit of the same iteration, in errors scaled so that a
beta of 0 is no special case (tests/assoc_reference.py), and holds p to the host's function of the device's own statistic."""
import json
import os

import numpy as np
import pytest

from inquistr_amd import hipcall
from tests import assoc_cases as ac
from tests import assoc_restatement as ar

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    c = hipcall.Context(0)
    yield c
    c.close()


def run(ctx, c):
    return ctx.assoc_rows(c.values, c.y, c.cov, c.outcome, c.mode, c.cutoff)


@pytest.mark.parametrize("outcome", ["binary", "continuous"])
@pytest.mark.parametrize("ns", [2, 3, 63, 64, 65, 127, 128, 129, 300])
def test_sample_counts_at_lane_and_stride_boundaries(ctx, ns, outcome):
    """one sample short of, at and one past one and two steps of a wave; k and the mode go round with ns"""
    c = ac.case(ns, 24, ns, [0, 1, 6][ns % 3], outcome, ac.MODES[ns % 3])
    ac.compare(c, run(ctx, c))


@pytest.mark.parametrize("outcome", ["binary", "continuous"])
@pytest.mark.parametrize("n_rows", [1, 3, 4, 5, 257])
def test_row_counts_around_a_workgroup(ctx, n_rows, outcome):
    """four rows to a workgroup: a part of one, exactly one, one row more, and 64 workgroups and a row"""
    c = ac.case(1000 + n_rows, n_rows, 65, 1, outcome, "max")
    got = run(ctx, c)
    ac.compare(c, got)
    assert not got["pad"].any()


@pytest.mark.parametrize("outcome", ["binary", "continuous"])
@pytest.mark.parametrize("mode", ac.MODES)
@pytest.mark.parametrize("k", [0, 1, 2, 3, 4, 5, 6])
def test_every_column_count_and_mode(ctx, k, mode, outcome):
    """one kernel instantiation per p = 2 + k: all seven, in all three modes"""
    c = ac.case(2000 + k, 16, 129, k, outcome, mode)
    ac.compare(c, run(ctx, c))


@pytest.mark.parametrize("outcome", ["binary", "continuous"])
@pytest.mark.parametrize("n_rows", [7, 8, 9, 17])
def test_tiles(ctx, n_rows, outcome):
    """rows go up tile by tile ("assoc_tile_rows" = 8 here): a row short of a tile, a tile, a row more, two tiles and a row - the
    same bytes as in one piece"""
    c = ac.case(3000 + n_rows, n_rows, 70, 2, outcome, "mean")
    whole = run(ctx, c)
    ctx.set_option("assoc_tile_rows", 8)
    try:
        tiled = run(ctx, c)
    finally:
        ctx.set_option("assoc_tile_rows", 0)
    assert tiled.tobytes() == whole.tobytes()
    ac.compare(c, tiled)


@pytest.mark.parametrize("outcome", ["binary", "continuous"])
@pytest.mark.parametrize("mode", ac.MODES)
def test_constructed_rows(ctx, mode, outcome):
    """NaNs in lane 0, in lane 63, in the last sample, in one haplotype only, in all samples; a constant row and one with two values;
    a group wiped out by NaNs; complete and quasi-complete separation; lengths near 10 000 with a spread of 1; an infinite value"""
    c = ac.special_case(outcome, mode)
    at = {n: i for i, n in enumerate(ac.SPECIAL_NAMES)}
    st = c.want["status"]
    # the restatement reaches what the rows were built for
    assert st[at["nan_everywhere"]] == ar.LOW_CALL_RATE and st[at["low_call_rate"]] == ar.LOW_CALL_RATE and st[at["constant"]] == ar.CONSTANT
    assert st[at["two_values"]] == ar.OK and st[at["near_10000"]] == ar.OK and st[at["nan_one_haplotype"]] == ar.OK
    assert c.want["n"][at["nan_lane0"]] == c.want["n"][at["nan_lane63"]] == c.want["n"][at["nan_last"]] == ac.SPECIAL_NS - 1
    if outcome == "binary":
        assert st[at["one_group"]] == ar.ONE_GROUP and st[at["separated"]] == ar.NOT_CONVERGED
        assert st[at["quasi_separated"]] in (ar.OK, ar.NOT_CONVERGED) and c.want["se"][at["quasi_separated"]] > 100.0
    assert st[at["inf_h1"]] == (ar.OK if mode == "min" else ar.SINGULAR)
    ac.compare(c, run(ctx, c))
    # the rows with the NaNs are held by their own conditioning, not by quasi_separated's, which sets the case's one tolerance
    tol = c.tol_row[0]
    names = ("nan_lane0", "nan_lane63", "nan_last", "nan_one_haplotype")
    print(f"one tolerance {c.tol:.2e} (quasi_separated: {tol[at['quasi_separated']]:.2e}); " + ", ".join(f"{n} {tol[at[n]]:.2e}" for n in names))
    assert all(c.fitted[at[n]] and tol[at[n]] < 1e-11 for n in names)


@pytest.mark.parametrize("outcome", ["binary", "continuous"])
@pytest.mark.parametrize("noise", [0.0, 1e-9])
def test_a_covariate_that_is_x(ctx, noise, outcome):
    c = ac.collinear_case(outcome, noise)
    assert c.want["status"][0] == ar.SINGULAR and (c.want["status"][1:] == ar.OK).all()
    got = run(ctx, c)
    ac.compare(c, got)
    assert np.isnan(got["beta"][0]) and np.isnan(got["p"][0]) and got["n"][0] == 90


def test_hand_derived_vectors(ctx):
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "kat_assoc.json")))
    for t in kat["tables"]["cases"]:
        a, b, c, d = t["a"], t["b"], t["c"], t["d"]
        x = np.array([1.0] * a + [1.0] * b + [0.0] * c + [0.0] * d)
        y = np.array([1.0] * a + [0.0] * b + [1.0] * c + [0.0] * d)
        got = ctx.assoc_rows(np.repeat(x, 2)[None, :].astype(np.float32), y, None, "binary", "mean")[0]
        beta, se = np.log(a * d / (b * c)), np.sqrt(1 / a + 1 / b + 1 / c + 1 / d)
        # the bounds of tests/test_assoc_restatement.py: beta within 1e-6 of its limit, the standard error (at the weights of the last
        # weighted least squares, i.e. of the iterate before) within 1e-4
        assert got["status"] == 0 and abs(got["beta"] - beta) < 1e-6 * max(1.0, abs(beta)) and abs(got["se"] - se) < 1e-4 * se
        assert (got["n"], got["n_g1"], got["n_g2"]) == (a + b + c + d, b + d, a + c)
        assert got["mean_g2"] == a / (a + c) and got["mean_g1"] == b / (b + d)
    o = kat["ols"]
    got = ctx.assoc_rows(np.repeat(np.array(o["x"], dtype=np.float32), 2)[None, :], np.array(o["y"]), None, "continuous", "max")[0]
    assert got["status"] == 0 and got["n"] == 5 and got["n_iter"] == 0
    for f, v in (("beta", o["beta"]), ("se", o["se"]), ("stat", o["t"]), ("p", o["p"])):
        assert abs(got[f] - v) <= 1e-9 * abs(v), (f, got[f], v)  # the hand arithmetic's own rounding: a dozen operations on 3-digit numbers
    assert (got["mean_all"], got["min_x"], got["max_x"]) == (o["mean"], o["min"], o["max"])
    for mode in ac.MODES:
        cases = kat["predictor"]["cases"]
        f = lambda v: float("nan") if v == "NaN" else float(v)
        # the rule shows in min / max / mean of a row made of one pair beside a pair that is there (4, 4)
        for t in cases:
            vals = np.array([[f(t["h1"]), f(t["h2"]), 4.0, 4.0]], dtype=np.float32)
            got = ctx.assoc_rows(vals, np.array([0.0, 1.0]), None, "binary", mode, missing_cutoff=0.0)[0]
            x = f(t[mode])
            if x != x:
                assert got["n"] == 1 and got["min_x"] == 4.0 == got["max_x"]
            else:
                assert got["n"] == 2 and got["min_x"] == min(x, 4.0) and got["max_x"] == max(x, 4.0) and got["mean_all"] == (x + 4.0) / 2


def test_arguments(ctx):
    L, h = ctx._L, ctx._h
    rows = np.zeros(4, dtype=hipcall.ASSOC_ROW_DTYPE)
    v = np.zeros((4, 8), dtype=np.float32)
    y = np.array([0.0, 1.0, 0.0, 1.0])
    cov = np.zeros((7, 4))
    call = lambda n_rows, ns, yy, k, outcome, mode, cut: L.inq_assoc_rows(h, v.ctypes.data, n_rows, ns, yy.ctypes.data, cov.ctypes.data, k, outcome,
                                                                        mode, cut, rows.ctypes.data)
    assert call(0, 4, y, 0, 0, 0, 0.8) == 0  # no rows: nothing to do
    assert call(4, 4, y, 7, 0, 0, 0.8) == -1 and call(4, 65536, y, 0, 0, 0, 0.8) == -1  # the limits, before any launch
    assert call(4, 4, y, 0, 2, 0, 0.8) == -1 and call(4, 4, y, 0, 0, 3, 0.8) == -1 and call(4, 4, y, 0, 0, 0, float("nan")) == -1
    assert call(4, 4, np.array([0.0, 1.0, 2.0, 1.0]), 0, 0, 0, 0.8) == -1  # a binary outcome is 0 or 1
    assert call(4, 4, np.array([0.0, 1.0, 2.0, 1.0]), 0, 1, 0, 0.8) == 0
    assert L.inq_assoc_rows(h, None, 4, 4, y.ctypes.data, None, 0, 0, 0, 0.8, rows.ctypes.data) == -1
