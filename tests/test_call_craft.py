"""tests/call_craft.py against the oracle and against itself (no GPU): what keeps tests/test_gpu_call_craft.py honest.

For every (distribution, depth class, mode): the oracle's rows equal rows_by_definition, its per-pair Calls and kinds equal the
spec, and the property the distribution is named for holds, computed from the spec.  No case is dropped: the number of
(distribution, class) pairs equals the table's."""
import math

import numpy as np
import pytest

from inquistr_amd.batch import INQ_PAIR_CLIP, INQ_PAIR_FETCHED, INQ_PAIR_KEPT
from tests import call_craft as cc
from tests import gen

CASES = cc.cases()


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def test_the_case_list_is_the_tables():
    pairs = {(d, n) for d, n, _ in CASES}
    assert len(pairs) == sum(len(v) for v in cc.TABLE.values()) == 8 * 10 + 2 + 4 + 1
    assert pairs == {(d, n) for d, classes in cc.TABLE.items() for n in classes}
    assert len(CASES) == sum(len(cc.TABLE[d]) * len(modes) for d, (_, _, modes) in cc.DISTRIBUTIONS.items())
    assert set(cc.TABLE) == set(cc.DISTRIBUTIONS)
    for d, classes in cc.TABLE.items():
        assert set(classes) <= set(cc.DEPTH_CLASSES) and (d in cc.OMITTED) == (classes != cc.DEPTH_CLASSES)
    in_batches = {(l.dist, n, u) for n, u, r in cc.batch_keys() for l in cc.batch_of(n, u, r)[1]}
    assert in_batches == set(CASES), "every case is in a batch, and no batch holds anything else"


def test_compose_uses_the_fewest_ops_and_every_op_counts():
    for minlen in (0, 5, 12):
        for kind in (cc.SPAN, cc.CLIP):
            for v in (0, 1, -1, minlen, minlen + 1, -minlen, -minlen - 1, 255, cc.OP_MAX, cc.OP_MAX + 1, cc.OP_MAX + minlen, 20 - cc.OP_MAX,
                      2 * cc.OP_MAX + 1, 1 << 32, (1 << 40) - 7, (1 << 46) - 1, 1 << 46, -(1 << 25) - 1):
                ops = cc.compose(v, kind, minlen)
                total = sum(int(ln.sum()) * (-1 if op == "D" else 1) for op, ln in ops)
                assert total == v and all((ln > minlen).all() for _, ln in ops)
                assert (kind == cc.CLIP) == any(op == "S" for op, _ in ops) and not any(op == "I" for op, _ in ops if kind == cc.CLIP)
                if v > minlen:
                    assert sum(len(ln) for _, ln in ops) == -(-v // cc.OP_MAX)
    ops = cc.compose(1 << 46, cc.SPAN, 5)
    assert len(ops) == 1 and ops[0][1].shape[0] == 262_145 and (ops[0][1][:-1] == cc.OP_MAX).all() and ops[0][1][-1] == 262_144


def test_slice_geometry_is_the_tail_kernels():
    assert cc.slice_geometry(65_537, 32) == (2304, 29, 9)  # 29 slices: three of 32 workgroups hold none
    assert cc.slice_geometry(65_537, 1) == (65_792, 1, 257)
    assert cc.slice_geometry(65_537, 3) == (22_016, 3, 86)
    assert cc.slice_geometry(65_537, 256) == (512, 129, 2)
    assert cc.slice_geometry(1_000_000, 256) == (4096, 245, 16)


@pytest.mark.parametrize("n,unphased,rule", cc.batch_keys(), ids=lambda v: str(v))
def test_batch_layout_and_tie_count(orc, n, unphased, rule):
    batch, loci = cc.batch_of(n, unphased, rule)
    want = cc.oracle_of(orc, n, unphased, rule)
    assert batch.n_loci == len(loci) >= 1 and (np.diff(batch.locus_pair_off.astype(np.int64)) == n).all()
    assert len(set(zip(batch.locus_start.tolist(), batch.locus_end.tolist()))) == batch.n_loci, "every locus its own window"
    assert gen.checked_share(batch) == 1.0 and not batch.reads["promise"].any()
    assert batch.support == cc.support_of(n, rule) and batch.unphased == unphased
    p1, p2, ties = cc.definition_rows(n, unphased, rule)
    assert want.n_tie_loci == ties
    assert gen.same_f64(want.phase1, p1) and gen.same_f64(want.phase2, p2)
    assert (want.pair_bits & INQ_PAIR_FETCHED).all()


def _groups(locus, support, unphased):
    g1, g2, tie, seen = cc.groups_by_definition(locus.spec, unphased)
    return cc.group_facts(g1, support), cc.group_facts(g2, support), tie, seen


def _check_property(l, n, support, rule, unphased, rows):
    f1, f2, tie, seen = _groups(l, support, unphased)
    both = (f1, f2)
    m = l.meta
    if l.dist == "all_equal_mixed":
        assert tie == unphased and len({v for v, _ in seen}) == 1
        for f in both:
            assert f["live"] and ((f["take"] == 0) if rule == "3" else (f["take"] > 0 and f["lump"] == f["take"] and f["eq"] == f["nc"]))
    elif l.dist == "two_values_even_split":
        for f, r in zip(both, rows):
            assert f["M"] % 2 == 0 and f["below"] == f["M"] // 2 and f["lo"] < f["hi"] and r % 1.0 == 0.5
        assert rows == m["want"]
    elif l.dist == "two_values_off_by_one":
        for f in both:
            assert f["M"] % 2 == 0 and f["below"] != f["M"] // 2 and f["lo"] == f["hi"]
        assert rows == m["want"]
    elif l.dist == "lower_median_is_the_lump":
        for f in both:
            assert f["take"] > 0 and f["M"] % 2 == 0 and f["below"] == f["M"] // 2 and f["thr"] < f["hi"]
            if l.variant == "lump":
                assert f["lo"] == f["thr"] and f["between"] == 0 and f["lump"] == f["take"]
            else:
                assert f["thr"] < f["lo"] < f["hi"] and f["between"] == 1 and f["lump"] == f["take"] - 1
        assert rows == m["want"]
    elif l.dist == "threshold_ties_partial_lump":
        for f in both:
            assert f["live"] and 0 < f["lump"] < f["eq"] and f["thr"] - f["hi"] == m["thr_minus_hi"]
    elif l.dist == "lump_in_a_wide_key_space":
        assert cc.select_top(l.spec, unphased) == 5 >= 2
        for f, thr in zip(both, m["thr"]):
            assert f["live"] and f["take"] > 0 and f["lump"] > 0 and f["thr"] == thr and (thr + 7) % (1 << 24) == 0
            if l.variant == "lump_is_lower_median":
                assert f["M"] % 2 == 0 and f["below"] == f["M"] // 2 and f["lo"] == thr < f["hi"] and f["between"] == 0 and f["lump"] == f["take"]
            else:
                assert 0 < f["lump"] < f["eq"] and f["thr"] - f["hi"] == m["thr_minus_hi"]
        if "want" in m:
            assert rows == m["want"]
    elif l.dist == "equal_run_across_boundaries":
        lo, hi = m["run"]
        cut = m["cut"]
        X = l.spec[lo][0]
        kept = [e for e in l.spec if e[3]]
        below = sum(1 for e in kept if e[0] < X)
        r = len(kept) // 2 - below
        assert r == m["r"] == cut - lo and 0 < r < m["eq"] == hi - lo and tie
        assert all(e[0] == X and e[3] for e in l.spec[lo:hi]) and not any(e[0] == X and e[3] for e in l.spec[:lo] + l.spec[hi:])
        assert l.spec[lo][1] == cc.CLIP and l.spec[cut - 1][1] == l.spec[cut][1] == l.spec[hi - 1][1] == cc.SPAN
        assert f1["ns"] == support and f1["nc"] > 0 and f1["take"] == 0, "one spanning Call more and the clip rule lets go of h1"
        assert rows == m["want"]
        inside = lambda step: any(lo < k < cut for k in range(step, hi, step))  # a boundary inside the run, in front of the cut
        if n == 16_385:
            assert inside(-(-n // 256)), "a chunk of reduce_deep_select's 256"
        if n == 65_537:
            assert inside(256)
            for g in sorted(set(cc.GRIDS + cc.CLAMPED_GRIDS)):
                sl, n_slices, part = cc.slice_geometry(n, g)
                assert (n_slices == 1) == (g == 1)
                if n_slices > 1:
                    assert inside(sl), f"a slice boundary of grid {g}"
                s_lo = (cut // sl) * sl  # the slice the cut lies in: thread parts start at s_lo + t * part
                assert any(max(lo, s_lo) < s_lo + t * part < cut for t in range(1, 256)), f"a thread-part boundary of grid {g}"
    elif l.dist == "byte_boundaries":
        assert cc.select_top(l.spec, unphased) == m["top"] == 5 and min(v for v, _ in seen) == -7
        c_lo, c_hi = m["cluster"]
        if unphased:
            s = sorted(v for v, _ in seen)
            assert c_lo <= s[len(s) // 2] <= c_hi
        else:
            g1, g2, _, _ = cc.groups_by_definition(l.spec, unphased)
            for f, g in zip(both, (g1, g2)):
                assert c_lo <= f["lo"] < f["hi"] <= c_hi or c_lo <= f["lo"] == f["hi"] <= c_hi
                assert sum(1 for v, k in g if k == cc.CLIP and c_lo <= v <= c_hi) >= f["M"] // 5 >= 1, "unchosen keys that share its upper bytes"
    elif l.dist == "signs":
        vals = sorted(v for v, _ in seen)
        assert vals[0] < 0 < vals[-1]
        if unphased:
            assert vals[len(vals) // 2] == m["split"] and tie == (l.variant != "minus_half")
        else:
            assert rows == m["want_phased"]
    elif l.dist in ("fit_limits", "sort_key_limits"):
        lim = cc.SORT_KEY_LIMIT if l.dist == "sort_key_limits" else cc.K_FIT[1 if n <= 64 else 4]
        kept = [e[0] for e in l.spec if e[3]]
        assert (m["x"], cc.SPAN, 2 if not m["kept"] or m["x"] > 0 else 1, m["kept"]) in l.spec
        side = {"fit_minus_1": lim - 1, "fit": lim, "minus_fit": -lim, "minus_fit_minus_1": -lim - 1, "limit_minus_1": lim - 1, "limit": lim}
        assert m["x"] == side[l.variant.replace("_unkept", "")] and m["kept"] == (not l.variant.endswith("_unkept"))
        assert m["inside"] == (l.variant in ("fit_minus_1", "minus_fit", "limit_minus_1") or not m["kept"])
        assert all(-lim <= v < lim for v in kept) == m["inside"], "the side of the limit the variant is named for"
        assert len(kept) == 6 and len(set(kept)) == 6
        if m["kept"]:
            assert m["x"] in (min(kept), max(kept)) and sorted(abs(v) for v in kept)[-2] == 50, "alone on its side"
            assert not any(math.isnan(r) for r in rows)
        else:
            assert max(kept) == 60
    elif l.dist == "count_boundaries":
        if "ng" in m:
            assert (f1["ng"], f2["ng"]) == m["ng"] and not f1["live"] and f2["live"] and math.isnan(rows[0]) and not math.isnan(rows[1])
            assert f2["take"] == f2["nc"] == min(m["take_all"], support)
        if "ns" in m:
            assert (f1["ns"], f2["ns"]) == m["ns"] and f1["live"] and f2["live"] and f1["nc"] > 0 and f2["nc"] > 0
            assert [f["take"] for f in both] == [max(0, support - x) for x in m["ns"]]
        if "kept" in m:
            assert len(seen) == m["kept"] and math.isnan(rows[0]) and math.isnan(rows[1])
        if l.variant == "one_group_empty" and not unphased:
            assert f2["ng"] == 0 and math.isnan(rows[1]) and not math.isnan(rows[0])
        if l.variant == "all_in_hp0_or_none":
            assert (len(seen) == 0 and math.isnan(rows[0]) and math.isnan(rows[1])) if not unphased else len(seen) > 0
    elif l.dist == "two_deep_loci_of_different_spread":
        assert cc.select_top(l.spec, unphased) == m["top"]
    else:
        raise AssertionError(l.dist)


@pytest.mark.parametrize("dist,n,unphased", CASES, ids=[f"{d}-{n}-{'unphased' if u else 'phased'}" for d, n, u in CASES])
def test_distribution(orc, dist, n, unphased):
    seen_variants = 0
    for rule in cc.DISTRIBUTIONS[dist][1]:
        support = cc.support_of(n, rule)
        batch, loci = cc.batch_of(n, unphased, rule)
        want = cc.oracle_of(orc, n, unphased, rule)
        for j, l in enumerate(loci):
            if l.dist != dist:
                continue
            seen_variants += 1
            what = f"{dist}/{l.variant} n={n} unphased={unphased} support={support}"
            r1, r2, tie = cc.rows_by_definition(l.spec, support, unphased)
            assert _same(want.phase1[j], r1) and _same(want.phase2[j], r2), f"{what}: oracle {want.phase1[j]} {want.phase2[j]}, definition {r1} {r2}"
            p0, p1 = int(batch.locus_pair_off[j]), int(batch.locus_pair_off[j + 1])
            assert want.pair_call[p0:p1].tolist() == [e[0] for e in l.spec], what
            bits = [INQ_PAIR_FETCHED | (INQ_PAIR_CLIP if e[1] == cc.CLIP else 0) | (INQ_PAIR_KEPT if e[3] and (unphased or e[2] is not None) else 0)
                    for e in l.spec]
            assert want.pair_bits[p0:p1].tolist() == bits, what
            _check_property(l, n, support, rule, unphased, (r1, r2))
    assert seen_variants == cc.VARIANTS[dist] * len(cc.DISTRIBUTIONS[dist][1]), "no variant is dropped"
