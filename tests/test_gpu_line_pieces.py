"""Pieces of the window-bounded walk on the 128-byte line grid (csrc/cigar_walk.h kLineMask).  Reads start at every cigar_off4 & 7 - filler reads of 1 to
7 groups that no locus is offered stand in front of them - in blocks of 1, 4, 5, 63 and 64 reads, under every promise
variant of tests/gen.py, and must equal the C oracle bit for bit: rows, pair_call, pair_bits, ties, status.  The oracle
ignores the promise byte (tests/test_window_bytes.py), so it runs once per batch.  The kernel has no half pieces (they
were measured and not kept): no kernel code for half pieces is tested here.  The two cases shaped for them - sparse
then dense, and the wide window - are kept as oracle-parity cases of the line grid, with reads whose bases per group
change abruptly between pieces; the model's "tail_half" layout only shows that the reads are shaped as the case says.
Needs an MI355X.
"""
import numpy as np
import pytest

from inquistr_amd import batch as B
from inquistr_amd.window_bytes import _walked_pieces, mark_checked
from tests import gen
from tests.walkutil import _all_variants, open_ctx

pytestmark = pytest.mark.gpu

SE, EE = 1000, 1100  # start_ext / end_ext of the locus (1010, 1090)
BLOCKS = (1, 4, 5, 63, 64)
SKIPS = range(8)


@pytest.fixture(scope="module")
def ctx():
    yield from open_ctx()


def _add_at(bb, skip, pos, cigar, k=0):
    """Adds the read so that it starts `skip` groups into a 128-byte line of the batch's CIGAR."""
    fill = (skip - bb._off4) % 8
    if fill:
        bb.add_read(0, B.encode_cigar([("M", 1)] * (4 * fill)), phase=1)
    i = bb.add_read(pos, B.encode_cigar(cigar), phase=1 + k % 2)
    assert bb._reads[i][0] % 8 == skip
    return i


def _batch(unphased, reads, window=(1010, 1090), blocks=BLOCKS):
    """reads: (skip, pos, cigar).  Every block size above 1 gets loci that together offer every read."""
    bb = B.BatchBuilder(minlen=2, support=1, unphased=unphased)
    idx = [_add_at(bb, s, pos, cig, k) for k, (s, pos, cig) in enumerate(reads)]
    for n in blocks:
        # (blocks of one read: every fifth read only, or the lone_* promise variants would have no read left to differ in)
        for lo in range(0, len(idx), 5 if n == 1 else n):
            take = [idx[(lo + j) % len(idx)] for j in range(n)]
            bb.add_locus(window[0], window[1], take)
    batch = bb.build()
    used = set(batch.pair_read.tolist())
    assert all(i in used for i in idx) and len(used) == len(idx), "fillers are offered to no locus"
    return batch


def _stop_read(s, n_ops, k=0):
    """A read of n_ops ops whose op s (0-based, from its start) is the first after which pos + consumed >= end_ext:
    one-base M ops, with I and D of minlen or more in the 24 ops either side of op s.  s >= n_ops: never gets there."""
    ops = []
    for i in range(n_ops):
        if i != s and abs(i - s) <= 24 and i % 4 == 1:
            ops.append(("I", 6 + (k + i) % 4))
        elif i != s and abs(i - s) <= 24 and i % 4 == 3:
            ops.append(("D", 3))
        else:
            ops.append(("M", 1))
    span = np.cumsum([ln if op in "MD" else 0 for op, ln in ops])
    reach = int(span[s]) if s < n_ops else int(span[-1]) + 5
    return EE - reach, ops


@pytest.mark.parametrize("unphased", [False, True])
def test_stop_op_around_every_half_and_full_piece_boundary(ctx, orc, unphased):
    """The stop op at -1, 0, +1 around every 32-op boundary, counted from the read's start and from the start of its
    line: the ends of piece 0 and of every half and full piece behind it, whichever way the pieces are laid."""
    reads = []
    for skip in SKIPS:
        for b in (32, 64, 96, 128, 160, 192):
            for d in (-1, 0, 1):
                for s in {b + d, b + d - 4 * skip}:
                    reads.append((skip, *_stop_read(s, 230 + skip, len(reads))))
    _all_variants(ctx, orc, _batch(unphased, reads), "stop op at boundaries")


@pytest.mark.parametrize("unphased", [False, True])
def test_read_lengths_around_the_line_and_piece_ends(ctx, orc, unphased):
    """Reads shorter than what is left of their first line, ending one group before, on and one group past the first
    line boundary, of exactly 16, 17, 24 groups less 0 and less skip, and of 31, 32 and 33 - skip groups - each once reaching end_ext in its last
    group, once stopping in its first and once not at all - with 1 to 4 ops in the last group."""
    reads = []
    for skip in SKIPS:
        # (31 ... 33 - skip: piece 1 holds 16 - skip groups and leaves up to 16 more, which a second piece must still load)
        lens = {1, 8 - skip - 1, 8 - skip, 8 - skip + 1, 16, 17, 24, 16 - skip, 17 - skip, 24 - skip, 31, 32, 33 - skip}
        for g in sorted(x for x in lens if x >= 1):
            for rem in (0, 1):
                n_ops = 4 * g - rem * (1 + skip % 3)
                for s in (n_ops - 1, min(2, n_ops - 1), n_ops + 1):
                    reads.append((skip, *_stop_read(s, n_ops, len(reads))))
    _all_variants(ctx, orc, _batch(unphased, reads), "read lengths")


@pytest.mark.parametrize("unphased", [False, True])
def test_half_piece_falls_short_and_full_piece_overshoots(ctx, orc, unphased):
    """Sparse then dense: piece 0 covers 10 bases an op, so the rule asks for a half piece, and the one-base ops behind
    need several more pieces.  Dense then sparse: one-base ops, so the rule asks for a full piece, whose first group
    passes end_ext.  The model walks them that way."""
    reads = []
    for skip in SKIPS:
        for extra in (20, 60, 100):  # ops of the dense part before the stop
            ops = [("M", 10)] * 64 + [("M", 1), ("I", 7), ("M", 1), ("D", 4)] * 60
            span = 10 * 64 + sum(ln for op, ln in ops[64 : 64 + extra + 1] if op in "MD")
            reads.append((skip, EE - span, ops))
        ops = [("M", 1), ("I", 7), ("M", 1), ("D", 4)] * 16 + [("M", 50), ("I", 9)] * 60
        reads.append((skip, EE - (16 * 6 + 50 + 20), ops))
    batch = _batch(unphased, reads)
    gen.set_promise(batch, "all")
    g0, groups, pieces, _ = _walked_pieces(batch, 64, "tail_half")
    first = {int(r): p for p, r in enumerate(batch.pair_read)}
    off4 = batch.reads["cigar_off4"]
    short = [first[i] for i in first if batch.reads["n_cigar"][i] == 304 and off4[i] % 8 == 0]
    over = [first[i] for i in first if batch.reads["n_cigar"][i] == 184 and off4[i] % 8 == 0]
    assert len(short) == 3 and len(over) == 1
    # (a read at skip 0 takes 16 + 8 h + 16 f groups in 1 + h + f pieces)
    assert any(pieces[p] >= 3 and groups[p] == 16 + 8 * (pieces[p] - 1) for p in short), "only half pieces behind piece 0, the first fell short"
    assert groups[over[0]] == 32 and pieces[over[0]] == 2, "a full piece where a half would have done"
    _all_variants(ctx, orc, batch, "sparse / dense")


@pytest.mark.parametrize("unphased", [False, True])
def test_first_and_last_group_of_the_batch(ctx, orc, unphased):
    """The read at cigar_off4 = 0 and the read that ends on the batch's last group, short and long, stopped and not."""
    for n_first, n_last in ((3, 5), (64, 64), (70, 97), (230, 300)):
        for s_first, s_last in ((1, 2), (n_first - 1, n_last - 1), (n_first + 1, n_last + 1)):
            reads = [(0, *_stop_read(s_first, n_first))]
            reads += [(k % 8, *_stop_read(40 + 9 * k, 200, k)) for k in range(1, 6)]
            reads.append((5, *_stop_read(s_last, n_last, 1)))
            batch = _batch(unphased, reads, blocks=(1, 4, 5))
            assert batch.reads["cigar_off4"][0] == 0
            last = batch.reads[-1]
            assert (int(last["cigar_off4"]) + (int(last["n_cigar"]) + 3) // 4) * 4 == batch.cigar.shape[0]
            _all_variants(ctx, orc, batch, f"first {n_first} last {n_last}")


@pytest.mark.parametrize("unphased", [False, True])
def test_wide_window_drains_mix_half_and_full_pieces(ctx, orc, unphased):
    """A 40 000 bp window: every lane of every piece is a window lane and the queue drains take entries from several
    pieces of one read.  Stretches of 1200-base ops between stretches of short ones make the rule ask for half pieces
    after the long ones and full pieces after the short ones."""
    reads = []
    for k, skip in enumerate(list(SKIPS) + [0, 3]):
        ops = ([("S", 4)] if k % 2 else []) + [("M", 2), ("I", 3 + k % 4), ("M", 1), ("D", 3)] * 16
        ops += [("M", 1200), ("I", 4)] * 32 + [("M", 2), ("I", 3), ("M", 1), ("D", 3)] * 20
        ops += [("M", 40), ("D", 5 + k % 3)] * 32 + [("M", 1), ("I", 5)] * 80
        reads.append((skip, 1005 + k, ops))
    batch = _batch(unphased, reads, window=(1010, 41000))
    gen.set_promise(batch, "all")
    g0, groups, pieces, _ = _walked_pieces(batch, 64, "tail_half")
    p = int(np.nonzero(batch.pair_read == 0)[0][0])  # the read at skip 0: 16 + 8 h + 16 f groups in 1 + h + f pieces
    assert batch.reads["cigar_off4"][0] == 0 and groups[p] < (batch.reads["n_cigar"][0] + 3) // 4
    h = 2 * (int(pieces[p]) - 1) - (int(groups[p]) - 16) // 8
    assert h >= 1 and int(pieces[p]) - 1 - h >= 1, "half and full pieces of one read"
    _all_variants(ctx, orc, batch, "wide window")


@pytest.mark.parametrize("unphased", [False, True])
@pytest.mark.parametrize("n", (4, 5, 64))
def test_unpromised_read_is_walked_whole_and_reported(ctx, orc, unphased, n):
    """One read among promised ones has op code 9 as its very last op, 400 ops behind the window: mark_checked leaves it
    alone unpromised, the walk takes it whole in full pieces and the batch fails with the oracle's code."""
    for at in sorted({0, n // 2, n - 1}):
        bb = B.BatchBuilder(minlen=2, support=1, unphased=unphased)
        idx = []
        for k in range(n):
            pos, ops = _stop_read(30 + 11 * (k % 12), 200 + k % 7, k)
            words = B.encode_cigar(ops + ([("M", 60), ("I", 3)] * 200 if k == at else []))
            if k == at:
                words[-1] = (9 << 4) | 9
            fill = ((k + at) % 8 - bb._off4) % 8
            if fill:
                bb.add_read(0, B.encode_cigar([("M", 1)] * (4 * fill)), phase=1)
            idx.append(bb.add_read(pos, words, phase=1 + k % 2))
        bb.add_locus(1010, 1090, idx)
        batch = bb.build()
        mark_checked(batch)
        assert batch.reads["promise"][idx[at]] == 0 and (batch.reads["promise"][idx] != 0).sum() == n - 1
        oc, _ = orc.call_batch(batch)
        rc, _ = ctx.call_batch(batch, debug=True, check=False)
        assert rc == oc == B.INQ_ERR_CIGAR_OP, (n, at, rc, oc)
        # ... and with a valid last op the same block passes under every variant
        batch.cigar[int(batch.reads["cigar_off4"][idx[at]]) * 4 + int(batch.reads["n_cigar"][idx[at]]) - 1] = (3 << 4) | 1
        _all_variants(ctx, orc, batch, f"n={n} at {at}")
