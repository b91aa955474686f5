"""inq_assoc_rows on the inputs no other test runs (the cases of tests/assoc_cases.py below "the inputs of
tests/test_gpu_assoc_edges.py", every one checked on the CPU by tests/test_assoc_reference.py with the wave-order route in the
device's place): prescribed t on both sides of the continued fractions' switch and out into the tail, n_samples at its limit,
Wald's z out to where erfc underflows, no sample and one, and what must not depend on where a row or a sample sits.

Every comparison goes through assoc_cases.compare: the exact fields, the case's one tolerance, each row's own tolerance against the
long-double reference, and p as the host's function of the device's own statistic."""
import numpy as np
import pytest

from inquistr_amd import hipcall
from tests import assoc_cases as ac
from tests import assoc_reference as rf
from tests import assoc_restatement as ar

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = hipcall.Context(0)
    yield c
    c.close()


def run(ctx, c, values=None, mode=None):
    return ctx.assoc_rows(c.values if values is None else values, c.y, c.cov, c.outcome, mode or c.mode, c.cutoff)


@pytest.mark.parametrize("k", ac.T_K)
@pytest.mark.parametrize("df", ac.T_DF)
def test_prescribed_t(ctx, df, k):
    """one row per |t| of assoc_cases.t_targets: 1e-8 to 1e6, the two sides of the switch between the continued fractions"""
    c = ac.prescribed_t_case(df, k)
    got = run(ctx, c)
    ac.compare(c, got)
    assert (got["n"] == df + 2 + k).all()
    assert [ac.cf_branch(t, df) for t in got["stat"]] == [ac.cf_branch(t, df) for t in c.t_ref]  # the device is on the side it was sent to


@pytest.mark.parametrize("outcome", ["binary", "continuous"])
@pytest.mark.parametrize("k", [0, 6])
@pytest.mark.parametrize("ns", [65535, 4096])
def test_n_samples_at_the_limit(ctx, ns, k, outcome):
    """65 535 samples: 1024 steps of a wave, the last one short a lane; df up to 65 533, the last entry of the coefficient table"""
    c = ac.limit_case(ns, k, outcome)
    assert (c.want["status"] == ar.OK).all()
    ac.compare(c, run(ctx, c))


def test_wald_z_out_to_underflow(ctx):
    c = ac.wald_case()
    got = run(ctx, c)
    ac.compare(c, got)
    tiny = c.ref["p"] < rf.P_MIN_NORMAL
    assert tiny.sum() >= 2 and ((got["p"][tiny] >= 0.0) & (got["p"][tiny] < rf.P_MIN_NORMAL)).all()


@pytest.mark.parametrize("outcome", ["binary", "continuous"])
@pytest.mark.parametrize("ns", [0, 1])
def test_no_sample_and_one(ctx, ns, outcome):
    c = ac.empty_case(ns, outcome)
    got = run(ctx, c)
    ac.compare(c, got)
    if ns == 0:
        assert (got["status"] == ar.LOW_CALL_RATE).all() and not got["n"].any() and not got["n_iter"].any()
        for f in ("beta", "se", "stat", "p", "mean_all", "mean_g1", "mean_g2", "min_x", "max_x"):
            assert np.isnan(got[f]).all(), f
    else:
        assert got["status"].tolist() == [ar.CONSTANT, ar.CONSTANT, ar.LOW_CALL_RATE] and got["n"].tolist() == [1, 1, 0]
        assert np.isnan(got["beta"]).all() and np.isnan(got["p"]).all() and got["min_x"][:2].tolist() == [7.5, 9.0]
    assert not got["pad"].any()


@pytest.mark.parametrize("outcome", ["binary", "continuous"])
def test_a_row_does_not_depend_on_its_place(ctx, outcome):
    """an ordinary row and the separated one at each of the 8 places of two workgroups, among other neighbours every time, in one
    piece and in tiles of 3 rows: the bytes it has in the whole case"""
    c = ac.invariance_case(outcome)
    whole = run(ctx, c)
    ac.compare(c, whole)
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
                assert got.tobytes() == whole[rows].tobytes(), (target, place, tile)


@pytest.mark.parametrize("outcome", ["binary", "continuous"])
@pytest.mark.parametrize("mode", ac.MODES)
def test_swapping_the_haplotypes_changes_nothing(ctx, mode, outcome):
    c = ac.invariance_case(outcome)
    swapped = np.ascontiguousarray(c.values.reshape(len(c.values), -1, 2)[:, :, ::-1]).reshape(len(c.values), -1)
    assert run(ctx, c, swapped, mode).tobytes() == run(ctx, c, None, mode).tobytes()


@pytest.mark.parametrize("outcome", ["binary", "continuous"])
@pytest.mark.parametrize("how", ["permuted", "shifted"])
def test_a_sample_may_sit_anywhere(ctx, how, outcome):
    """the samples in another order, and behind 65 samples without a value (another lane and another stride for every one): the
    statuses, counts and steps of the case as it was, the numbers within each row's tolerance of the SAME reference row"""
    c = ac.invariance_case(outcome)
    d = ac.permuted(c) if how == "permuted" else ac.shifted(c)
    base, got = run(ctx, c), run(ctx, d)
    ac.compare(d, got)
    for f in ("status", "n", "n_g1", "n_g2"):
        assert np.array_equal(got[f], base[f]), f
    hold = ~(c.skip | d.skip)
    assert np.array_equal(got["n_iter"][hold], base["n_iter"][hold])
    assert np.array_equal(got["min_x"], base["min_x"], equal_nan=True) and np.array_equal(got["max_x"], base["max_x"], equal_nan=True)
