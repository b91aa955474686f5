"""`inquiSTR outlier` restatement (oracle/outlier_oracle.py) against the reference's own unit-test vectors and
hand-derived ones; host-side text rules that need no GPU."""
import json
import os

import numpy as np
import pytest

from oracle import outlier_oracle as oo
from tests import gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def kat():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "kat_outlier.json")))["vectors"]


def test_oracle_reproduces_the_reference_unit_tests(kat):
    assert sum(1 for v in kat if v["name"].startswith("reference")) == 2
    for v in kat:
        vals = [np.float32(x) for x in v["values"]]
        if v["method"] == "zscore":
            got = oo.z_score_outliers(vals, v["samples"], v["cutoff"])
        else:
            got = oo.dbscan_outliers(vals, v["samples"], v["mincluster"])
        assert got == v["expect"], v["name"]


WRAPPING_ROW = [float("inf"), float("inf"), float("inf"), 12.0, 2.5e19]


def test_twice_the_mode_wraps_like_the_release_build():
    """`max(2 * mode, 10)` (src/outlier.rs:115) is usize arithmetic without overflow checks in the reference's release
    profile.  Three `inf` and 2.5e19 all cast to usize::MAX: the mode; twice that wraps to 2^64 - 2 = 1.8e19 as f64.
    12 and 2.5e19 are then 2.5e19 apart - not neighbours - and each alone is no cluster of two; an infinite value is
    not even its own neighbour (inf - inf is NaN).  All five are noise.  Without the wrap eps would be 3.7e19 and the
    two finite values a cluster."""
    row = [np.float32(x) for x in WRAPPING_ROW]
    assert oo.mode(row) == 2**64 - 1
    assert oo.dbscan_flags(row, 2) == [True] * 5
    vals = np.array([WRAPPING_ROW], dtype=np.float32)
    flags, keep = oo.c_outlier_rows(vals, [5], "dbscan", minsize=10, mincluster=2)
    assert keep.tolist() == [1] and flags[0].tolist() == [1] * 5
    # a mode of 2^63 wraps to 0, so eps is the floor of 10: 12 and 30 are noise (unwrapped, 2^64 would reach everything)
    vals = np.array([[2.0**63] * 3 + [12, 30]], dtype=np.float32)
    assert oo.dbscan_flags(list(vals[0]), 2) == [False, False, False, True, True]
    flags, keep = oo.c_outlier_rows(vals, [5], "dbscan", minsize=10, mincluster=2)
    assert keep.tolist() == [1] and flags[0].tolist() == [0, 0, 0, 1, 1]


def test_parse_f32_follows_rust():
    for ok in ["1", "-1.5", "+2", ".5", "5.", "1e3", "1E-2", "NaN", "nan", "inf", "-Infinity"]:
        oo.parse_f32(ok)
    for bad in ["", " 1", "1 ", "e5", ".", "0x10", "1_0", "1,5", "--1"]:
        with pytest.raises(oo.ReferencePanic):
            oo.parse_f32(bad)


def test_outlier_text_rules():
    head = "chromosome\tbegin\tend\tA_H1\tA_H2\tB_H1\tB_H2\tC_H1\tC_H2\tD_H1\tD_H2"
    rows = ["chr1\t10\t20\t1\t2\t2\t3\t1\tNaN\t3\t500", "chr1\t30\t40\t1\t2\t2\t3\t1\t5\t3\t2", "chr2\t5\t9\t400\t2\t2\t3\t1\t5\t3\t2"]
    assert oo.outlier_text([head] + rows, 10, 2.0) == "chrom\tbegin\tend\toutliers\nchr1\t10\t20\tD\nchr2\t5\t9\tA\n"
    assert oo.outlier_text([head] + rows, 10, 2.0, subset=["A"]) == "chrom\tbegin\tend\toutliers\nchr2\t5\t9\tA\n"
    assert oo.outlier_text([head] + rows, 1000, 2.0) == "chrom\tbegin\tend\toutliers\n"  # nothing reaches minsize
    with pytest.raises(oo.ReferencePanic):
        oo.outlier_text([head, "chr1\t1\t2\tx"], 10, 2.0)
    with pytest.raises(oo.ReferencePanic):
        oo.outlier_text(["chromosome\tbegin\tend"], 10, 2.0)


def test_outlier_command_without_gpu(tmp_path):
    """No CPU path for the arithmetic: without a gfx950 device the command ends with status 1; the reference's
    argument panics come first."""
    import torch

    from inquistr_amd import call

    p = tmp_path / "c.tsv"
    p.write_text("chromosome\tbegin\tend\tA_H1\tA_H2\nchr1\t1\t9\t12\t99\n")
    with pytest.raises(call.CallError) as e:
        call.outlier(tmp_path / "missing.tsv")
    assert e.value.status == 101 and "does not exist" in e.value.message
    (tmp_path / "s.txt").write_text("A\n")
    with pytest.raises(call.CallError) as e:
        call.outlier(p, sample="A", subset=tmp_path / "s.txt")
    assert e.value.status == 101
    if not torch.cuda.is_available():
        with pytest.raises(call.CallError) as e, open(tmp_path / "o.txt", "w") as f:
            call.outlier(p, out=f)
        assert e.value.status == 1 and "no CPU fallback" in e.value.message


@pytest.mark.parametrize("method", ["zscore", "dbscan"])
def test_c_restatement_agrees_with_the_python_one(method):
    import random

    rng = random.Random(5)
    n_rows, n_cols = 200, 37
    vals = np.zeros((n_rows, n_cols), dtype=np.float32)
    lens = np.zeros(n_rows, dtype=np.uint32)
    for i in range(n_rows):
        n = rng.choice([0, 1, 5, n_cols, n_cols])
        base = rng.choice([3, 12, 40])
        row = [base + rng.choice([-1, 0, 0, 1, 0.5]) for _ in range(n)]
        for _ in range(rng.choice([0, 1, 3])):
            if n:
                row[rng.randrange(n)] = rng.choice([base * 7.0, float("nan"), float("inf"), -4.0])
        vals[i, :n] = row
        lens[i] = n
    # rows whose mode is usize::MAX, so that `2 * mode` wraps: the known-answer row (at mincluster = 5 noise with or without the wrap)
    # and one in which only the wrap keeps the finite values from being a cluster of six
    wide = [float("inf")] * 7 + [12.0] * 3 + [2.5e19] * 3
    for i, row in ((n_rows - 2, WRAPPING_ROW), (n_rows - 1, wide)):
        vals[i] = 0
        vals[i, : len(row)] = row
        lens[i] = len(row)
    if method == "dbscan":
        assert oo.dbscan_flags(list(vals[n_rows - 1, : len(wide)]), 5) == [True] * len(wide)
    flags, keep = oo.c_outlier_rows(vals, lens, method, minsize=10, cutoff=2.0, mincluster=5, threads=2)
    for i in range(n_rows):
        row = [np.float32(0) if np.isnan(x) else x for x in vals[i, : lens[i]]]
        if not row:
            assert keep[i] == 2
        elif max(row) < np.float32(10):
            assert keep[i] == 0
        else:
            try:
                want = oo.z_score_flags(row, 2.0) if method == "zscore" else oo.dbscan_flags(row, 5)
            except oo.ReferencePanic:
                assert keep[i] == 3
                continue
            assert keep[i] == 1 and list(flags[i, : lens[i]].astype(bool)) == want, i


@pytest.mark.parametrize("stride,n_rows", gen.DBSCAN_CLASSES)
def test_dbscan_rows_cover_every_size_class(stride, n_rows):
    """What the wide-row GPU test relies on, from the reference alone: at every width kept rows, flagged values, edge points, a row
    without a mode and a row that only a wrapping `2 * mode` answers as the reference does; over the three matrices of a width
    every kind of row - lengths 0, 1, the width and both neighbours of a power of two, one repeated value at the full width, a row
    that is skipped -; nothing flagged behind a row's length; and, on the narrowest class, the C restatement's answer is the
    Python one's."""
    per = gen.dbscan_class_reference(stride, n_rows)
    gen.assert_dbscan_class_is_covered(stride, per)
    pow2 = 1 << ((stride - 1).bit_length() - 1)
    lengths, states, constant = set(), set(), False
    for vals, lens, mincluster, flags, keep in per:
        lengths |= set(lens.tolist())
        states |= set(keep.tolist())
        constant |= any(lens[i] == stride and (vals[i] == vals[i, 0]).all() for i in range(n_rows))
        assert not flags[np.arange(stride)[None, :] >= lens[:, None]].any()
        if mincluster >= 3:  # the wrap row: every value noise; unwrapped, only its infinities
            want = np.array(gen.dbscan_wrap_row(stride, mincluster), dtype=np.float32)
            at = [i for i in range(n_rows) if lens[i] == len(want) and np.array_equal(vals[i, : len(want)], want)]
            assert at and all(keep[i] == 1 and flags[i, : len(want)].all() for i in at)
            assert gen.dbscan_flags_by_definition(want, len(want), mincluster, False).tolist() == np.isinf(want).astype(int).tolist()
        if stride == 256 and mincluster == 8:
            for i in range(0, n_rows, 5):
                row = [np.float32(0) if np.isnan(x) else x for x in vals[i, : lens[i]]]
                if keep[i] == 1:
                    assert list(flags[i, : lens[i]].astype(bool)) == oo.dbscan_flags(row, mincluster), i
    assert {0, 1, stride, pow2 - 1, pow2, pow2 + 1} <= lengths and {0, 1, 2, 3} <= states and constant
