"""`inquiSTR outlier` on the GPU (inq_outlier_rows / inq_outlier) against the restatement, which the reference's
own unit tests pin (tests/test_outlier_oracle.py)."""
import gzip
import json
import os
import random
import subprocess

import numpy as np
import pytest

from inquistr_amd import call, hipcall
from oracle import outlier_oracle as oo
from tests import gen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    c = hipcall.Context(0)
    yield c
    c.close()


def test_reference_unit_test_vectors_on_the_gpu(ctx):
    for v in json.load(open(os.path.join(ROOT, "tests", "golden", "kat_outlier.json")))["vectors"]:
        vals = np.array([v["values"]], dtype=np.float32)
        rc, flags, keep = ctx.outlier_rows(vals, [vals.shape[1]], v["method"], minsize=0, zscore_cutoff=v.get("cutoff", 3.0),
                                           mincluster=v.get("mincluster", 1))
        assert rc == 0 and keep[0] == 1
        assert [oo._strip(v["samples"][k]) for k in np.nonzero(flags[0])[0]] == v["expect"], v["name"]


def _random_matrix(rng, n_rows, n_cols):
    rows, lens = [], []
    for _ in range(n_rows):
        n = n_cols if rng.random() < 0.8 else rng.randint(0, n_cols)
        kind = rng.random()
        if kind < 0.5:
            base = rng.choice([5, 12, 30, 200])
            r = [base + rng.choice([-1, 0, 0, 0, 1, 2]) + (0.5 if rng.random() < 0.2 else 0) for _ in range(n)]
            for _ in range(rng.choice([0, 1, 1, 2, 5])):
                if n:
                    r[rng.randrange(n)] = base * rng.choice([2, 3, 10]) + rng.randint(0, 400)
        elif kind < 0.7:
            r = [rng.choice([0, 1, 2, 3]) for _ in range(n)]  # mostly below minsize
        elif kind < 0.85:
            r = [rng.uniform(-50, 3000) for _ in range(n)]
        else:
            r = [float(rng.choice([7, 7, 7, 40])) for _ in range(n)]
        r = [float("nan") if rng.random() < 0.08 else x for x in r]
        if rng.random() < 0.05 and n:  # "inf" parses as an f32 too
            r[rng.randrange(n)] = rng.choice([float("inf"), float("-inf")])
        lens.append(n)
        rows.append(r + [0.0] * (n_cols - n))
    return np.array(rows, dtype=np.float32).reshape(n_rows, n_cols), np.array(lens, dtype=np.uint32)


@pytest.mark.parametrize("method", ["zscore", "dbscan"])
@pytest.mark.parametrize("seed,n_cols", [(1, 11), (2, 64), (3, 130), (4, 1), (5, 300)])
def test_outlier_rows_match_the_restatement(ctx, method, seed, n_cols):
    rng = random.Random(seed)
    vals, lens = _random_matrix(rng, 300, n_cols)
    minsize, cutoff, mincluster = rng.choice([0, 10, 10, 25]), rng.choice([1.0, 2.0, 3.0]), max(1, n_cols.bit_length() - 1)
    rc, flags, keep = ctx.outlier_rows(vals, lens, method, minsize=minsize, zscore_cutoff=cutoff, mincluster=mincluster)
    assert rc == 0
    for i in range(len(lens)):
        row = [np.float32(0) if np.isnan(x) else x for x in vals[i, : lens[i]]]
        if not row:
            assert keep[i] == 2
            continue
        if max(row) < np.float32(minsize):
            assert keep[i] == 0 and not flags[i].any()
            continue
        if method == "zscore":
            want = oo.z_score_flags(row, cutoff)
        else:
            try:
                want = oo.dbscan_flags(row, mincluster)
            except oo.ReferencePanic:
                assert keep[i] == 3
                continue
        assert keep[i] == 1
        assert list(flags[i, : lens[i]].astype(bool)) == want, (seed, i)
        assert not flags[i, lens[i]:].any()


@pytest.mark.parametrize("n_cols", [1, 3, 63, 64, 65, 127, 128, 129, 200, 255, 256, 257])
def test_zscore_through_the_lds_tile_equals_the_transposed_copy(ctx, n_cols):
    """Rows of at most 256 values take the LDS-tile kernel (one read of the row-major matrix, 64 or 32 rows per wave), wider ones and
    "outlier_tile" = 0 the transposed-copy kernel: the same flags and row states from both, on ragged rows (lengths 0 ... n_cols), a row
    count that is no multiple of a tile, NaNs, and equal to the plain-Python restatement."""
    rng = random.Random(1000 + n_cols)
    vals, lens = _random_matrix(rng, 777, n_cols)
    vals[rng.randrange(777), rng.randrange(n_cols)] = np.nan
    cutoff = rng.choice([1.0, 2.0, 3.0])
    rc, flags, keep = ctx.outlier_rows(vals, lens, "zscore", minsize=10, zscore_cutoff=cutoff, mincluster=3)
    ctx.set_option("outlier_tile", 0)
    try:
        rc2, flags2, keep2 = ctx.outlier_rows(vals, lens, "zscore", minsize=10, zscore_cutoff=cutoff, mincluster=3)
    finally:
        ctx.set_option("outlier_tile", 1)
    assert rc == rc2 == 0 and np.array_equal(flags, flags2) and np.array_equal(keep, keep2)
    for i in range(0, len(lens), 7):
        row = [np.float32(0) if np.isnan(x) else x for x in vals[i, : lens[i]]]
        if row and max(row) >= np.float32(10):
            assert keep[i] == 1 and list(flags[i, : lens[i]].astype(bool)) == oo.z_score_flags(row, cutoff), i
    assert keep.tolist().count(1) > 50


@pytest.mark.parametrize("method", ["zscore", "dbscan"])
def test_outlier_command_text(tmp_path, method):
    rng = random.Random(77)
    samples = [f"S{k}_H{h}" for k in range(20) for h in (1, 2)]
    vals, lens = _random_matrix(rng, 400, len(samples))
    lines = ["chromosome\tbegin\tend\t" + "\t".join(samples)]
    for i in range(len(lens)):
        if lens[i] == 0:
            lens[i] = 1  # a locus without values panics: tested separately
        cells = ["NaN" if np.isnan(x) else (str(int(x)) if float(x).is_integer() else repr(float(x))) for x in vals[i, : lens[i]]]
        lines.append(f"chr{1 + i % 3}\t{1000 * i}\t{1000 * i + 50}\t" + "\t".join(cells))
    plain, gz = tmp_path / "c.tsv", tmp_path / "c.tsv.gz"
    plain.write_text("\n".join(lines) + "\n")
    with gzip.open(gz, "wt") as f:
        f.write("\n".join(lines) + "\n")
    for path in (plain, gz):
        for kw in ({}, {"sample": "S3"}, {"minsize": 40, "zscore": 2.0}):
            out = tmp_path / "o.txt"
            with open(out, "w") as f:
                call.outlier(path, method=method, out=f, **kw)
            try:
                want = oo.outlier_text(lines, kw.get("minsize", 10), kw.get("zscore", 3.0), method,
                                       [kw["sample"]] if "sample" in kw else None)
            except oo.ReferencePanic:
                pytest.skip("a row without positive values under DBSCAN")
            assert out.read_text() == want, (path.name, kw)
    # the CLI prints the same bytes
    cli = os.path.join(ROOT, "inquistr_amd", "lib", "inquistr")
    r = subprocess.run([cli, "outlier", str(plain), "--method", method, "-z", "2.0", "--minsize", "40"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == oo.outlier_text(lines, 40, 2.0, method)


def test_outlier_command_panics_like_the_reference(tmp_path):
    head = "chromosome\tbegin\tend\tA_H1\tA_H2\tB_H1\tB_H2"
    good = "chr1\t1\t9\t12\t12\t12\t99"

    def run(text, **kw):
        p = tmp_path / "c.tsv"
        p.write_text(text)
        out = tmp_path / "o.txt"
        with open(out, "w") as f:
            try:
                call.outlier(p, out=f, zscore=1.0, **kw)
                status = 0
            except call.CallError as e:
                status = e.status
        return status, out.read_text()

    assert run(head + "\n" + good + "\n") == (0, "chrom\tbegin\tend\toutliers\nchr1\t1\t9\tB\n")
    # the lines in front of a bad number are still reported, then the panic
    assert run(head + "\n" + good + "\nchr1\t20\t30\t1\tx\t3\t4\n" + good + "\n") == (101, "chrom\tbegin\tend\toutliers\nchr1\t1\t9\tB\n")
    assert run(head + "\n" + good + "\nchr1\t20\n")[0] == 101
    assert run(head + "\nchr1\t20\t30\n")[0] == 101  # no values: max of nothing
    assert run("chromosome\tbegin\tend\n" + good + "\n") == (101, "chrom\tbegin\tend\toutliers\n")
    assert run("")[0] == 101
    with pytest.raises(call.CallError) as e:
        call.outlier(tmp_path / "missing.tsv")
    assert e.value.status == 101
    (tmp_path / "subset.txt").write_text("A\n")
    with pytest.raises(call.CallError) as e:
        call.outlier(tmp_path / "c.tsv", sample="A", subset=tmp_path / "subset.txt")
    assert e.value.status == 101


@pytest.mark.parametrize("stride,n_rows", gen.DBSCAN_CLASSES)
def test_dbscan_at_every_size_class(ctx, stride, n_rows):
    """launch_outlier picks outlier_dbscan_kernel<256, 64>, <2048, 256> or <8192, 256> by the matrix' width: widths on both sides of
    both edges and the widest (65.6 KB of LDS, a 13-stage bitonic sort, 16-bit indices and prefix counts), rows of gen.dbscan_rows
    - groups of equal values placed exactly eps - 1, eps and eps + 1 from a cluster, of one fewer, exactly and one more than
    `mincluster` values; NaN, +-inf, negative values; a mode key of 0; ragged lengths around a power of two; one repeated value -
    under mincluster 1, ilog2(width) and the width.  From mincluster 3 on every matrix holds gen.dbscan_wrap_row, whose flags a
    kernel that did not wrap `2 * mode` would get wrong (asserted from the reference by assert_dbscan_class_is_covered).  Flags and
    row states equal the C restatement's exactly."""
    per = gen.dbscan_class_reference(stride, n_rows)
    gen.assert_dbscan_class_is_covered(stride, per)  # from the reference alone (without a GPU: tests/test_outlier_oracle.py)
    for vals, lens, mincluster, want_flags, want_keep in per:
        rc, flags, keep = ctx.outlier_rows(vals, lens, "dbscan", minsize=0, mincluster=mincluster)
        assert rc == 0
        assert np.array_equal(keep, want_keep), (stride, mincluster, keep.tolist(), want_keep.tolist())
        bad = np.argwhere(flags != want_flags)
        assert bad.size == 0, (stride, mincluster, bad[:8].tolist())


@pytest.mark.parametrize("stride", [5, 257, 2049])
def test_dbscan_wraps_twice_the_mode(ctx, stride):
    """[inf, inf, inf, 12, 2.5e19] at mincluster 2, through each of the three kernels: the mode is usize::MAX, `2 * mode` wraps to
    2^64 - 2 as in the reference's release build (src/outlier.rs:115), so 12 and 2.5e19 are no neighbours and all five values are
    noise; a kernel that widened or saturated the product would make the two a cluster and flag the infinities only.  Beside it
    the row whose mode, 2^63, wraps to 0: eps is the floor of 10 and 12 and 30 are noise."""
    vals = np.full((2, stride), gen.DBSCAN_PAD, dtype=np.float32)
    vals[0, :5] = gen.DBSCAN_WRAP_ROW
    vals[1, :5] = [2.0**63] * 3 + [12, 30]
    lens = np.array([5, 5], dtype=np.uint32)
    want_flags, want_keep = oo.c_outlier_rows(vals, lens, "dbscan", minsize=10, mincluster=2)
    assert want_keep.tolist() == [1, 1] and want_flags[:, :5].tolist() == [[1, 1, 1, 1, 1], [0, 0, 0, 1, 1]]
    assert gen.dbscan_flags_by_definition(vals[0], 5, 2, False).tolist() == [1, 1, 1, 0, 0]
    rc, flags, keep = ctx.outlier_rows(vals, lens, "dbscan", minsize=10, mincluster=2)
    assert rc == 0 and keep.tolist() == [1, 1] and np.array_equal(flags, want_flags), flags[:, :5].tolist()


def test_dbscan_rows_wider_than_the_widest_class(ctx):
    """A matrix of 8 193 columns: the row that fills them is INQ_OUTLIER_ROW_TOO_WIDE and nothing of it is flagged; the rows beside
    it that fit the widest class are computed as ever."""
    rng = random.Random(8193)
    stride, lens = 8193, np.array([8193, 8192, 10, 0], dtype=np.uint32)
    vals, _ = gen.dbscan_rows(rng, stride, 4, 13)
    vals[1, :8192] = vals[0, :8192]
    vals[2, :10] = [12, 12, 13, 12, 400, 12, 11, 12, float("nan"), 12]
    rc, flags, keep = ctx.outlier_rows(vals, lens, "dbscan", minsize=10, mincluster=3)
    want_flags, want_keep = oo.c_outlier_rows(vals[1:], lens[1:], "dbscan", minsize=10, mincluster=3, threads=8)
    assert rc == 0 and want_keep.tolist() == [1, 1, 2] and want_flags[1, :10].tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0, 0]
    assert keep.tolist() == [4, 1, int(want_keep[1]), 2]
    assert not flags[0].any() and not flags[3].any()
    assert np.array_equal(flags[1:], want_flags)


def test_outlier_command_refuses_dbscan_on_more_than_8192_values(tmp_path):
    """`inquistr outlier --method dbscan` on a cohort file with 8 193 value columns: the error status and its message, and not one
    line on standard output - the same file is fine for the z-score."""
    names = "\t".join(f"S{k}_H{1 + k % 2}" for k in range(8193))
    cells = "\t".join(["12"] * 8192 + ["500"])
    p = tmp_path / "wide.tsv"
    p.write_text(f"chromosome\tbegin\tend\t{names}\nchr1\t100\t200\t{cells}\n")
    cli = os.path.join(ROOT, "inquistr_amd", "lib", "inquistr")
    r = subprocess.run([cli, "outlier", str(p), "--method", "dbscan"], capture_output=True, text=True)
    assert r.returncode == 1 and "more than 8192 values" in r.stderr and r.stdout == ""
    with pytest.raises(call.CallError) as e, open(tmp_path / "o.txt", "w") as f:
        call.outlier(p, method="dbscan", out=f)
    assert e.value.status == 1 and "more than 8192 values" in e.value.message and (tmp_path / "o.txt").read_text() == ""
    r = subprocess.run([cli, "outlier", str(p), "--method", "zscore"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "chrom\tbegin\tend\toutliers\nchr1\t100\t200\tS8192\n"


@pytest.mark.parametrize("stride", [257, 2049, 8193])
def test_zscore_on_wide_rows_equals_the_c_restatement(ctx, stride):
    """Rows wider than the LDS tile take the transposed copy: widths past 256, 2 048 and 8 192 values (the transpose's last tile
    holds one column), ragged, against the sequential f32 sums of the C restatement."""
    rng = random.Random(stride)
    vals, lens = _random_matrix(rng, 130, stride)
    lens[:3] = [stride, stride - 1, 0]
    for cutoff, minsize in ((2.0, 10), (3.0, 0)):
        rc, flags, keep = ctx.outlier_rows(vals, lens, "zscore", minsize=minsize, zscore_cutoff=cutoff, mincluster=3)
        want_flags, want_keep = oo.c_outlier_rows(vals, lens, "zscore", minsize=minsize, cutoff=cutoff, threads=8)
        assert rc == 0 and np.array_equal(keep, want_keep)
        assert np.array_equal(flags, want_flags), np.argwhere(flags != want_flags)[:8].tolist()
        assert (want_keep == 1).sum() > 50 and want_flags.any()
