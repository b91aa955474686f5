"""inq_assoc_rows_firth on the inputs no other test runs (the cases of tests/firth_cases.py below "the inputs of
tests/test_gpu_firth_edges.py", every one checked on the CPU by tests/test_assoc_reference.py with the wave-order route in the
device's place): chi2 out to where erfc underflows, loci without an effect (most loci of a real file), no sample and one, and what
must not depend on where a row or a sample sits.

Every comparison goes through firth_cases.compare: the exact fields, the case's one tolerance, each row's own tolerance against the
long-double reference (chi2 at the scale of l*, which is what lets a row without an effect be held), and p as the host's erfc of
the device's own chi2."""
import numpy as np
import pytest

from inquistr_amd import hipcall
from tests import assoc_cases as ac
from tests import assoc_reference as rf
from tests import assoc_restatement as ar
from tests import firth_cases as fc
from tests import firth_restatement as fr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = hipcall.Context(0)
    yield c
    c.close()


def check(ctx, c, whens=fc.WHENS):
    ordinary = ctx.assoc_rows(c.values, c.y, c.cov, "binary", c.mode, c.cutoff)
    out = {}
    for when in whens:
        rows, firth = ctx.assoc_rows_firth(c.values, c.y, c.cov, c.mode, c.cutoff, when)
        fc.compare(c, when, rows, firth, ordinary)
        out[when] = firth
    return out


def test_chi2_out_to_underflow(ctx):
    c = fc.chi2_case()
    got = check(ctx, c, ("always",))["always"]
    tiny = c.ref["p"] < rf.P_MIN_NORMAL
    assert tiny.sum() >= 2 and ((got["p"][tiny] >= 0.0) & (got["p"][tiny] < rf.P_MIN_NORMAL)).all()


def test_loci_without_an_effect(ctx):
    """24 random rows whose chi2 is small beside l*, and one whose two fits are the same fit: chi2 is held to a few roundings of
    l*, and may be the 0 that max(0, .) makes of a negative difference"""
    c = fc.no_effect_case()
    got = check(ctx, c)
    r = got["always"][24]
    assert r["status"] == fr.OK and r["chi2"] >= 0.0 and r["p"] > 0.999, r  # how small chi2 is: compare(), at the scale of l*
    assert abs(r["beta"]) <= 1e-9 * r["se"]  # the stopping rule's own size: a step below 1e-9 standard errors
    assert not c.R.fitted("fallback").any() and (got["fallback"]["status"] == fr.NOT_FITTED).all()


@pytest.mark.parametrize("ns", [0, 1])
def test_no_sample_and_one(ctx, ns):
    c = fc.empty_case(ns)
    for when, firth in check(ctx, c).items():
        assert (firth["status"] == fr.NOT_FITTED).all() and not firth["n_iter_full"].any() and not firth["n_iter_null"].any()
        for f in ("beta", "se", "chi2", "p", "pll_full", "pll_null"):
            assert np.isnan(firth[f]).all(), (when, f)
    rows, _ = ctx.assoc_rows_firth(c.values, c.y, c.cov, c.mode, c.cutoff, "always")
    assert rows["status"].tolist() == ([ar.LOW_CALL_RATE] * 3 if ns == 0 else [ar.CONSTANT, ar.CONSTANT, ar.LOW_CALL_RATE])


def run(ctx, c, values=None, mode=None):
    return ctx.assoc_rows_firth(c.values if values is None else values, c.y, c.cov, mode or c.mode, c.cutoff, "always")


def test_a_row_does_not_depend_on_its_place(ctx):
    """an ordinary row and the separated one at each of the 8 places of two workgroups, among other neighbours every time, in one
    piece and in tiles of 3 rows: the bytes they have in the whole case, in both outputs"""
    c = fc.invariance_case()
    check(ctx, c, ("always",))
    whole = run(ctx, c)
    rng = np.random.default_rng(8)
    for target in (3, len(c.values) - 1):
        others = np.array([i for i in range(len(c.values)) if i != target])
        for place in range(8):
            rows = rng.choice(others, 7, replace=False).tolist()
            rows.insert(place, target)
            for tile in (0, 3):
                ctx.set_option("assoc_tile_rows", tile)
                try:
                    got = run(ctx, c, c.values[rows])
                finally:
                    ctx.set_option("assoc_tile_rows", 0)
                assert got[0].tobytes() == whole[0][rows].tobytes() and got[1].tobytes() == whole[1][rows].tobytes(), (target, place, tile)


@pytest.mark.parametrize("mode", ac.MODES)
def test_swapping_the_haplotypes_changes_nothing(ctx, mode):
    c = fc.invariance_case()
    swapped = np.ascontiguousarray(c.values.reshape(len(c.values), -1, 2)[:, :, ::-1]).reshape(len(c.values), -1)
    a, b = run(ctx, c, swapped, mode), run(ctx, c, None, mode)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("how", ["permuted", "shifted"])
def test_a_sample_may_sit_anywhere(ctx, how):
    """the samples in another order, and behind 65 samples without a value: the statuses and steps of the case as it was, the
    numbers within each row's tolerance of the SAME reference row"""
    c = fc.invariance_case()
    o = ac.invariance_case("binary")
    d = fc.derived_case(c, ac.permuted(o) if how == "permuted" else ac.shifted(o))
    base = run(ctx, c)[1]
    got = check(ctx, d, ("always",))["always"]
    assert np.array_equal(got["status"], base["status"])
    hold = ~(c.skip | d.skip)
    for f in ("n_iter_full", "n_iter_null"):
        assert np.array_equal(got[f][hold], base[f][hold]), f
