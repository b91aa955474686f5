"""The register reduce of a locus of at most 64 offered reads (csrc/kernels.hip reduce_locus_in_lanes, one read per lane), on both
sides of the line between its two ways of finding the unphased medians: a bitonic sort of the packed (value, lane) keys across the
wave when no kept Call is soft-clipped and every kept value fits the key - 15 stages when no kept read sits in a lane >= 32, 21
otherwise -, and the rank loop for every other locus.  Loci are written down as their Calls with tests/call_craft.py; read i of a
locus is lane i of its wave, so the file order below is the lane order.

    offered depths   1, 2, 3, 4, 31, 32, 33, 63, 64
    kept reads       low: only in lanes < 32, unkept reads (mapq <= 10) above; high: only in lanes >= 32 (depths > 32); spread:
                     interleaved with unkept ones over all lanes, lane 0 and the last lane among them
    kept counts      0, 1, support - 1, support, 5, 6 and the largest odd and even count the placement holds
    values           all equal; two values, split evenly; ascending and descending in file order; negative; kFit - 1 and -kFit
                     (the largest and smallest value of a key: sorted - kFit - 1 in lane 63 is a key equal to the pad of an unkept
                     lane) beside kFit and -kFit - 1 on the same shapes (rank loop, i64 compares)
    and each again with one clipped kept read added (rank loop) - in a lane without a kept read; a full locus has none, there the
    last kept read is the clipped one
    support          1, 3 and the depth; phased and unphased; promise variants `none` and `all`

Rows equal as f64 (NaN where NaN) to the oracle's and to rows_by_definition's; per-pair Calls, bits and the tie count equal to the
oracle's.  Bit-exact."""
import numpy as np
import pytest

from tests import call_craft as cc
from tests import gen
from tests.test_gpu_parity import _assert_same

pytestmark = pytest.mark.gpu

DEPTHS = (1, 2, 3, 4, 31, 32, 33, 63, 64)
KFIT = cc.K_FIT[1]


@pytest.fixture(scope="module")
def ctx():
    from inquistr_amd import hipcall

    c = hipcall.Context(0)
    yield c
    c.close()


def _placements(n):
    """name -> the lanes that may hold a kept read, in the order they are filled."""
    out = {"low": list(range(min(n, 32))), "spread": None}
    if n > 32:
        out["high"] = list(range(32, n))
    return out


def _lanes(n, where, k):
    if where != "spread":
        return _placements(n)[where][:k]
    if k <= 1:
        return [n // 2][:k]
    return sorted({round(i * (n - 1) / (k - 1)) for i in range(k)})  # k distinct lanes (k <= n), 0 and n - 1 among them


def _values(k):
    """pattern -> the k kept values in file order."""
    big = [3 * i - 4 for i in range(k)]
    out = {"equal": [37] * k,
           "two_values": [(10, 21)[(i + i // 2) % 2] for i in range(k - k % 2)] + [21] * (k % 2),
           "ascending": [5 + 3 * i for i in range(k)],
           "descending": [5 + 3 * (k - 1 - i) for i in range(k)],
           "negative": [-7 - 2 * ((5 * i) % max(k, 1)) for i in range(k)]}
    for name, top, bottom in (("fit", KFIT - 1, -KFIT), ("beyond_fit", KFIT, -KFIT - 1)):
        v = list(big)
        if k >= 1:
            v[-1] = top  # the last kept lane: lane 63 of a full or spread locus of 64
        if k >= 2:
            v[0] = bottom
        out[name] = v
    return out


def _counts(support, cap):
    want = {0, 1, support - 1, support, 5, 6, cap, cap - 1}
    return sorted(k for k in want if 0 <= k <= cap)


def _spec(n, lanes, values, clip):
    """n offered reads in lane order: the kept Calls (HP 1 and 2 in turn) in `lanes`, unkept filler elsewhere."""
    spec = cc.filler(n)
    for i, (lane, v) in enumerate(zip(lanes, values)):
        spec[lane] = (v, cc.SPAN, 1 + i % 2, True)
    if clip:
        free = [l for l in range(n) if l not in lanes]
        if free:
            spec[free[len(free) // 2]] = (13, cc.CLIP, 1, True)
        elif lanes:
            spec[lanes[-1]] = (values[-1], cc.CLIP, 1 + (len(lanes) - 1) % 2, True)
    return spec


def _loci(n, support, where):
    """[(name, spec)] of one batch: the loci of one placement."""
    out = []
    cap = n if where == "spread" else len(_placements(n)[where])
    for k in _counts(support, cap):
        lanes = _lanes(n, where, k)
        assert len(lanes) == k
        for pattern, values in _values(k).items():
            for clip in (False, True):
                out.append((f"{where}/kept{k}/{pattern}{'/clip' if clip else ''}", _spec(n, lanes, values, clip)))
    return out


def test_the_specs_reach_both_paths():
    """From the specs alone: the sorted path's own cases exist - kept reads in lanes < 32 only and in lanes >= 32, kFit - 1 in lane
    63 - and so do the rank loop's."""
    loci = {name: spec for where in _placements(64) for name, spec in _loci(64, 3, where)}
    kept_lanes = lambda spec: [l for l, e in enumerate(spec) if e[3]]
    assert max(kept_lanes(loci["low/kept32/ascending"])) == 31 and min(kept_lanes(loci["high/kept32/ascending"])) == 32
    assert loci["spread/kept64/fit"][63][:2] == (KFIT - 1, cc.SPAN) and loci["spread/kept64/fit"][0][0] == -KFIT
    assert loci["spread/kept64/beyond_fit"][63][0] == KFIT and loci["spread/kept64/beyond_fit"][0][0] == -KFIT - 1
    assert sum(e[3] and e[1] == cc.CLIP for e in loci["low/kept5/equal/clip"]) == 1
    assert not any(e[3] and e[1] == cc.CLIP for e in loci["low/kept5/equal"])
    for n in DEPTHS:
        for support in {1, 3, n}:
            assert all(len(spec) == n for where in _placements(n) for _, spec in _loci(n, support, where))


@pytest.mark.parametrize("unphased", (True, False), ids=("unphased", "phased"))
@pytest.mark.parametrize("n", DEPTHS)
def test_rows_of_shallow_loci(ctx, orc, n, unphased):
    for support, where in [(s, w) for s in sorted({1, 3, n}) for w in _placements(n)]:
        loci = _loci(n, support, where)
        batch = cc.build([spec for _, spec in loci], cc.MINLEN, support, unphased)
        oc, want = orc.call_batch(batch, debug=True, threads=8)
        assert oc == 0
        rows = [cc.rows_by_definition(spec, support, unphased) for _, spec in loci]
        p1, p2 = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
        for variant in ("none", "all"):
            what = f"depth {n} support {support} {where} {gen.set_promise(batch, variant)}"
            rc, got = ctx.call_batch(batch, debug=True)
            assert rc == 0, what
            bad = [f"{name}: got ({got.phase1[j]}, {got.phase2[j]}), by definition ({p1[j]}, {p2[j]})" for j, (name, _) in enumerate(loci)
                   if not (gen.same_f64(got.phase1[j : j + 1], p1[j : j + 1]) and gen.same_f64(got.phase2[j : j + 1], p2[j : j + 1]))]
            assert not bad, f"{what}: " + "; ".join(bad[:6])
            assert got.n_tie_loci == sum(int(r[2]) for r in rows), what
            _assert_same(got, want, what)
