"""Every locus reduce against Call multisets built to break it (tests/call_craft.py; tests/test_call_craft.py shows, without a GPU,
that each batch reaches the branch it is named for and that the oracle agrees with the rule's definition on it).

Every batch - one per (depth class, mode, support rule), the depth classes being the smallest depths at which each of the five
reduces can still go wrong - goes through `call_batch(debug=True)` under the promise variants `none` and `all` (the walk is not the
subject): rows equal as f64 (NaN where NaN) to the oracle's and to rows_by_definition's, per-pair Calls, bits and the tie count
equal to the oracle's.  Bit-exact; there is no tolerance.  The two deepest classes (one workgroup's radix select; the grid-wide
select) run again on contexts with grid_tail 1, 3 and 32: at 65 537 reads that is 1 slice, 3 slices of 22 016 and 29 slices of 2 304
(three workgroups hold none)."""
import pytest

from tests import call_craft as cc
from tests import gen
from tests.test_gpu_parity import _assert_same

pytestmark = pytest.mark.gpu

DEEPEST = cc.DEPTH_CLASSES[-2:]


def _id(key):
    n, unphased, rule = key
    return f"{n}-{'unphased' if unphased else 'phased'}-support_{rule}"


@pytest.fixture(scope="module")
def ctx():
    from inquistr_amd import hipcall

    c = hipcall.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", params=cc.GRIDS[:-1], ids=[f"tail{g}" for g in cc.GRIDS[:-1]])
def grid_ctx(request):
    """A context of its own per grid (32 is within every partition's CU count: the library's clamp leaves it as it is)."""
    from inquistr_amd import hipcall

    c = hipcall.Context(0)
    c.set_option("grid_tail", request.param)
    yield c
    c.close()


_ROWS = {}


def _run(ctx, orc, key, what):
    batch, loci = cc.batch_of(*key)
    want = cc.oracle_of(orc, *key)
    if key not in _ROWS:
        _ROWS[key] = cc.definition_rows(*key)
    p1, p2, ties = _ROWS[key]
    try:
        for variant in ("none", "all"):
            name = f"{what} {_id(key)} {gen.set_promise(batch, variant)}"
            rc, got = ctx.call_batch(batch, debug=True)
            assert rc == 0, name
            bad = [f"{l.dist}/{l.variant}: got ({got.phase1[j]}, {got.phase2[j]}), by definition ({p1[j]}, {p2[j]})" for j, l in enumerate(loci)
                   if not (gen.same_f64(got.phase1[j : j + 1], p1[j : j + 1]) and gen.same_f64(got.phase2[j : j + 1], p2[j : j + 1]))]
            assert not bad, f"{name}: " + "; ".join(bad)
            assert got.n_tie_loci == ties, name
            _assert_same(got, want, name)
    finally:  # the batch is every test's
        gen.set_promise(batch, "none")


@pytest.mark.parametrize("key", cc.batch_keys(), ids=_id)
def test_crafted_calls(ctx, orc, key):
    _run(ctx, orc, key, "default grid")


@pytest.mark.parametrize("key", [k for k in cc.batch_keys() if k[0] in DEEPEST], ids=_id)
def test_crafted_calls_of_the_deepest_classes_at_this_grid(grid_ctx, orc, key):
    _run(grid_ctx, orc, key, "grid_tail set")
