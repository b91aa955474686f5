"""The two phases of the window-bounded walk (csrc/cigar_walk.h walk_pairs_rows): piece 0 of every read walked
statically, four reads a turn, then the reads that have not stopped compacted and walked on by rows that claim
them - and the switch that drops the device's domain checks in blocks whose reads are all promised.  Every batch
goes through every promise variant of tests/gen.py and must equal the C oracle bit for bit: rows, pair_call,
pair_bits, ties, status.  Needs an MI355X.
"""
import numpy as np
import pytest

from inquistr_amd import batch as B
from inquistr_amd.window_bytes import mark_checked
from tests.walkutil import _all_variants, _assert_same, open_ctx

pytestmark = pytest.mark.gpu

SE, EE = 1000, 1100  # start_ext / end_ext of the locus (1010, 1090)
COUNTS = (1, 3, 4, 5, 63, 64)


@pytest.fixture(scope="module")
def ctx():
    yield from open_ctx()


def _call(ctx, orc, batch, what):
    oc, want = orc.call_batch(batch, debug=True)
    rc, got = ctx.call_batch(batch, debug=True, check=False)
    assert rc == oc, (what, rc, oc)
    if rc == B.INQ_OK:
        _assert_same(got, want, what)
    return rc


def _stops(k):
    """A read that passes end_ext inside piece 0 (its first 64 ops) and has 200 ops; I ops in the window."""
    return EE - 40 - k % 7, [("M", 3), ("I", 6 + k % 5), ("M", 2), ("D", 7)] * 50


def _goes_on(k, pieces=3):
    """A read that reaches end_ext only in piece `pieces` (ops 64 * pieces ...): one-base ops up to there."""
    n = 64 * pieces + 5 + k % 9
    return EE - n, [("M", 1)] * (n - 30) + [("I", 6 + k % 4), ("M", 1), ("D", 6), ("M", 1)] * 30


def _block(unphased, reads):
    bb = B.BatchBuilder(minlen=2, support=1, unphased=unphased)
    return bb, [bb.add_read(pos, B.encode_cigar(cig), phase=1 + k % 2) for k, (pos, cig) in enumerate(reads)]


@pytest.mark.parametrize("unphased", [False, True])
@pytest.mark.parametrize("n", COUNTS)
def test_reads_that_stop_in_piece_0(ctx, orc, unphased, n):
    """Blocks of n reads of which 0, 1, all but one and all stop in piece 0, the others wherever in the block."""
    for n_stop in sorted({0, 1, n - 1, n}):
        for where in ("first", "last", "spread"):
            go = n - n_stop
            if where == "first":
                goes = set(range(go))
            elif where == "last":
                goes = set(range(n - go, n))
            else:
                goes = set((i * n) // go for i in range(go)) if go else set()
            reads = [_goes_on(k, 1 + k % 4) if k in goes else _stops(k) for k in range(n)]
            bb, idx = _block(unphased, reads)
            bb.add_locus(1010, 1090, idx)
            _all_variants(ctx, orc, bb.build(), f"n={n} stop={n_stop} {where}")


@pytest.mark.parametrize("unphased", [False, True])
@pytest.mark.parametrize("n", COUNTS)
def test_one_unpromised_read_in_a_promised_block(ctx, orc, unphased, n):
    """All promised, then exactly one read unpromised, first / middle / last: the block walks with the device's checks
    again and nothing else changes."""
    reads = [_goes_on(k, 1 + k % 3) if k % 3 else _stops(k) for k in range(n)]
    bb, idx = _block(unphased, reads)
    bb.add_locus(1010, 1090, idx)
    batch = bb.build()
    mark_checked(batch)
    assert (batch.reads["promise"] == B.INQ_READ_CHECKED).all()
    assert _call(ctx, orc, batch, f"n={n} all promised") == B.INQ_OK
    for k in sorted({0, n // 2, n - 1}):
        mark_checked(batch)
        batch.reads["promise"][idx[k]] = 0
        assert _call(ctx, orc, batch, f"n={n} read {k} unpromised") == B.INQ_OK


@pytest.mark.parametrize("unphased", [False, True])
@pytest.mark.parametrize("n", (1, 5, 64))
@pytest.mark.parametrize("kind", ["bad_op", "range"])
def test_unpromised_bad_read_is_still_found(ctx, orc, unphased, n, kind):
    """One unpromisable read among promised ones: an op code 9 in its tail far behind the window, or positions past
    2^31 - 1 in a later piece.  mark_checked leaves exactly that read unpromised and its status code comes out."""
    base = 2**31 - 5000 if kind == "range" else 0
    for at in sorted({0, n // 2, n - 1}):
        bb = B.BatchBuilder(minlen=2, support=1, unphased=unphased)
        idx = []
        for k in range(n):
            pos, cig = _goes_on(k, 1 + k % 3) if k % 2 else _stops(k)
            words = B.encode_cigar(cig)
            if k == at:
                if kind == "bad_op":
                    words = B.encode_cigar(cig + [("M", 2), ("I", 3)] * 100)
                    words[-1] = (9 << 4) | 9
                else:
                    words = B.encode_cigar(cig + [("M", 100)] * 60)
            idx.append(bb.add_read(base + pos, words, phase=1 + k % 2))
        bb.add_locus(base + 1010, base + 1090, idx)
        batch = bb.build()
        mark_checked(batch)
        assert (batch.reads["promise"] != 0).sum() == n - 1 and batch.reads["promise"][idx[at]] == 0
        want = B.INQ_ERR_CIGAR_OP if kind == "bad_op" else B.INQ_ERR_RANGE
        assert _call(ctx, orc, batch, f"{kind} n={n} at {at}") == want
        batch.reads["promise"] = 0
        assert _call(ctx, orc, batch, f"{kind} n={n} at {at}, none promised") == want


@pytest.mark.parametrize("unphased", [False, True])
@pytest.mark.parametrize("n", (4, 5, 63, 64))
def test_reads_settled_without_a_load(ctx, orc, unphased, n):
    """Empty CIGARs and promised reads that start past end_ext, at the start, in the middle and at the end of a block
    whose other reads go on past piece 0.  Every third settled read is empty at pos = start_ext: its reference_end is
    pos + 1 (rlen 0 -> 1), one past start_ext, so it is fetched - and would not be, were the end it is settled on one
    less."""
    for run in (1, 3, min(n - 1, 17)):
        for lo in sorted({0, (n - run) // 2, n - run}):
            reads, on_edge = [], []
            for k in range(n):
                if lo <= k < lo + run:
                    kind = (k - lo) % 3
                    on_edge.append(kind == 0)
                    reads.append([(SE, []), (1090, []), (EE + k % 3, [("M", 4), ("I", 9)] * 40)][kind])
                else:
                    on_edge.append(False)
                    reads.append(_goes_on(k, 1 + k % 3))
            bb, idx = _block(unphased, reads)
            bb.add_locus(1010, 1090, idx)
            batch = bb.build()
            _, want = orc.call_batch(batch, debug=True)
            edge = np.array(on_edge)
            assert edge.any() and (want.pair_bits[edge] & B.INQ_PAIR_FETCHED).all(), "the empty reads on start_ext are fetched"
            assert unphased or (want.pair_bits[edge] & B.INQ_PAIR_KEPT).all()
            _all_variants(ctx, orc, batch, f"n={n} run={run} at {lo}")


@pytest.mark.parametrize("unphased", [False, True])
def test_stop_rule_at_the_end_of_piece_0(ctx, orc, unphased):
    """pos + consumed on end_ext - 2 ... + 1 after exactly 63 and exactly 64 ops, with an I right behind; reads of
    exactly 64 and 65 ops that do and do not reach end_ext."""
    reads = []
    tail = [("I", 7), ("M", 1), ("D", 9), ("M", 1)] * 25
    for at in (63, 64):
        for d in (-2, -1, 0, 1):
            reads.append((EE + d - at, [("M", 1)] * at + tail))
            reads.append((EE + d - at, [("M", 1)] * (at - 2) + [("I", 6), ("M", 2)] + tail))
    for n_ops in (64, 65):
        for d in (-30, -2, -1, 0, 1):
            reads.append((EE + d - (n_ops - 1), [("M", 1)] * (n_ops - 2) + [("I", 8), ("M", 1)]))
            reads.append((EE + d - n_ops, [("M", 1)] * (n_ops - 1) + [("D", 1)]))
    bb, idx = _block(unphased, reads)
    bb.add_locus(1010, 1090, idx)
    bb.add_locus(1010, 1090, idx[::-1])
    for k in (1, 3, 4, 5):
        bb.add_locus(1010, 1090, idx[k : 2 * k])
    _all_variants(ctx, orc, bb.build(), "piece 0 edges")


@pytest.mark.parametrize("unphased", [False, True])
@pytest.mark.parametrize("n", (1, 3, 5, 64))
def test_wide_window_feeds_one_drain_from_several_pieces(ctx, orc, unphased, n):
    """A 40 000 bp window under reads of short ops: every lane of every piece is a window lane, so the 80 entries of a
    queue drain come from piece 0 and from later pieces of the same read (n = 1: pieces 0 ... 4 of the one read)."""
    reads = [(1005 + k, ([("S", 4)] if k % 2 else []) + [("M", 2), ("I", 3 + k % 4), ("M", 1), ("D", 3)] * 120) for k in range(n)]
    bb, idx = _block(unphased, reads)
    bb.add_locus(1010, 41000, idx)
    _all_variants(ctx, orc, bb.build(), f"wide n={n}")
