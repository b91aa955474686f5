"""The head phase of the window-bounded walk (csrc/cigar_walk.h walk_pairs_rows): the first kHeadLines = 4 lines of 128
bytes of every read of a block, walked by eight rows of eight lanes, read k of a 32-read pass in row k % 8 of load slot
k // 8.  Blocks of every size around the rows, the slots and the passes (and of 65 and 257 reads, which come to the walk
through the medium and the deep kernels), reads that start at every cigar_off4 & 7, end around every line's end and stop
around it, reads that load nothing, blocks of mixed promises, domain errors inside the head, and queue drains inside it -
each must equal the C oracle bit for bit: rows, pair_call, pair_bits, ties, status.  The oracle ignores the promise byte
(tests/test_window_bytes.py), so it runs once per batch.  Needs an MI355X.
"""
import numpy as np
import pytest

from inquistr_amd import batch as B
from inquistr_amd.window_bytes import HEAD_LINES, head_layout, mark_checked
from tests import gen
from tests.walkutil import _all_variants, _assert_same, open_ctx

pytestmark = pytest.mark.gpu

SE, EE = 1000, 1100  # start_ext / end_ext of the locus (1010, 1090)
BLOCKS = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 257)
SKIPS = range(8)
MODES = pytest.mark.parametrize("unphased", [False, True])


@pytest.fixture(scope="module")
def ctx():
    yield from open_ctx()


def _add_at(bb, skip, pos, words, k=0):
    """Adds the read so that it starts `skip` groups into a 128-byte line of the batch's CIGAR: a filler read of 1 to 7
    groups that no locus is offered (8 when the read is to start a line of its own behind another) stands in front."""
    fill = (skip - bb._off4) % 8 or (8 if k % 3 == 2 else 0)
    if fill:
        bb.add_read(0, B.encode_cigar([("M", 1)] * (4 * fill)), phase=1)
    i = bb.add_read(pos, words, phase=1 + k % 2)
    assert bb._reads[i][0] % 8 == skip
    return i


def _batch(unphased, reads, window=(1010, 1090), blocks=BLOCKS):
    """reads: (skip, pos, [(op, len)] or words).  Every block size gets loci that together offer every read, in blocks of
    that many; a block larger than the list takes its reads again from the start."""
    bb = B.BatchBuilder(minlen=2, support=1, unphased=unphased)
    idx = []
    for k, (s, pos, cig) in enumerate(reads):
        idx.append(_add_at(bb, s, pos, cig if isinstance(cig, np.ndarray) else B.encode_cigar(cig), k))
    for n in blocks:
        # (blocks of one read: every fifth read only, or the lone_* promise variants would have no read left to differ in)
        for lo in range(0, len(idx), 5 if n == 1 else n):
            bb.add_locus(window[0], window[1], [idx[(lo + j) % len(idx)] for j in range(n)])
    batch = bb.build()
    assert set(batch.pair_read.tolist()) == set(idx), "fillers are offered to no locus"
    return batch


def _stop_read(s, n_ops, k=0):
    """A read of n_ops ops whose op s (0-based, from its start) is the first after which pos + consumed >= end_ext:
    one-base M ops, with I and D of minlen or more in the 24 ops either side of op s, so that the ops around the stop are
    counted ones.  s >= n_ops: never gets there."""
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


def _line_end_ops(skip, line):
    """The first and the last op of the last group of the read's head line `line` (1-based), from the read's start."""
    last_group = 8 * line - skip - 1
    return 4 * last_group, 4 * last_group + 3


@MODES
def test_stop_on_the_last_group_of_every_head_line_and_on_the_first_behind(ctx, orc, unphased):
    """The stop op on the last group of head lines 1 to 4 (its first and its last op) and on the first group of line 5 -
    where the read goes to the continuation list with its next group on a line boundary - at every start offset, in
    blocks of every size.  The model walks them as the case says."""
    reads, want_lines = [], []
    for skip in SKIPS:
        for line in range(1, HEAD_LINES + 2):
            first, last = _line_end_ops(skip, line)
            for s in (first, last) if line <= HEAD_LINES else (last + 1, last + 4):
                reads.append((skip, *_stop_read(s, 230 + skip, len(reads))))
                want_lines.append(line if line <= HEAD_LINES else HEAD_LINES + 2)  # behind the head: one piece of two lines
    batch = _batch(unphased, reads)
    gen.set_promise(batch, "all")
    groups, lines, head, _ = head_layout(batch)
    first_pair = {int(r): p for p, r in reversed(list(enumerate(batch.pair_read)))}
    got = [int(lines[first_pair[i]]) for i in sorted(first_pair)]
    assert got == want_lines, "each read stops in the line it was built for"
    _all_variants(ctx, orc, batch, "stop at the line ends")


@MODES
def test_read_lengths_around_every_head_line_end(ctx, orc, unphased):
    """Reads of exactly 8 L - skip groups (they end with head line L), one group more and one fewer, L = 1 to 5, with 1 to
    4 ops in the last group - each once reaching end_ext in its last group, once stopping in its first and once not at all."""
    reads = []
    for skip in SKIPS:
        lens = {8 * line - skip + d for line in range(1, HEAD_LINES + 2) for d in (-1, 0, 1)} | {1}
        for g in sorted(x for x in lens if x >= 1):
            for rem in (0, 1):
                n_ops = 4 * g - rem * (1 + (skip + g) % 3)
                for s in (n_ops - 1, min(2, n_ops - 1), n_ops + 1):
                    reads.append((skip, *_stop_read(s, n_ops, len(reads))))
    _all_variants(ctx, orc, _batch(unphased, reads, blocks=(1, 8, 9, 32, 33, 64, 65)), "read lengths")


@MODES
def test_reads_that_load_nothing_among_reads_that_do(ctx, orc, unphased):
    """Empty CIGARs and promised reads that start at or past end_ext, alone in a row, filling a slot, filling a pass, and
    next to reads of one line and of six: their rows stay idle and their slots are skipped without a load."""
    empty = np.zeros(0, dtype=np.uint32)
    walked = [(k % 8, *_stop_read((20, 70, 150, 400)[k % 4], 230, k)) for k in range(12)]
    nothing = [(k % 8, EE + (0, 1, 40_000)[k % 3], [("M", 5), ("I", 4), ("M", 7)] * (1 + 9 * (k % 2))) for k in range(6)]
    nothing += [(0, SE + 5 * k, empty) for k in range(4)]
    last_start = [(3, EE - 1, [("M", 2), ("I", 5), ("D", 3)] * 4)]  # pos + 1 == end_ext: the last start that is walked
    for layout in range(4):
        if layout == 0:  # a whole pass of 32 reads with nothing to load, then reads that are walked
            reads = [nothing[k % len(nothing)] for k in range(32)] + walked
        elif layout == 1:  # slots 1 and 3 of the pass are idle
            reads = walked[:8] + nothing[:8] + walked[4:12] + [nothing[(k + 3) % len(nothing)] for k in range(8)] + last_start
        elif layout == 2:  # one live row in every slot
            reads = [walked[k // 8] if k % 8 == (3 * (k // 8)) % 8 else nothing[k % len(nothing)] for k in range(64)]
        else:  # alternating
            reads = [x for pair in zip(walked, nothing + nothing) for x in pair] + last_start
        bb = B.BatchBuilder(minlen=2, support=1, unphased=unphased)
        idx = [_add_at(bb, s, pos, c if isinstance(c, np.ndarray) else B.encode_cigar(c), k) for k, (s, pos, c) in enumerate(reads)]
        for n in (len(idx), 32, 33, 8, 1):
            for lo in range(0, len(idx), 5 if n == 1 else n):
                bb.add_locus(1010, 1090, idx[lo : lo + n])
        bb.add_locus(1010, 1090, (idx * 8)[:257])
        _all_variants(ctx, orc, bb.build(), f"nothing to load, layout {layout}")


def _mixed_block(unphased, n, at, odd_ops, other_ops, rule_breaker=None):
    """A block of n reads: read `at` is built by odd_ops(k), the others by other_ops(k); every read at another start offset.
    rule_breaker(words) damages read `at` so that mark_checked leaves it unpromised."""
    bb = B.BatchBuilder(minlen=2, support=1, unphased=unphased)
    idx = []
    for k in range(n):
        pos, ops = (odd_ops if k == at else other_ops)(k)
        words = B.encode_cigar(ops)
        if k == at and rule_breaker is not None:
            rule_breaker(words)
        idx.append(_add_at(bb, (k + at) % 8, pos, words, k))
    bb.add_locus(1010, 1090, idx)
    return bb.build(), idx


def _long_tail(k):
    """Over six lines: 230 ops that pass end_ext early, then 400 more, with counted ops far behind the window's end."""
    pos, ops = _stop_read(30 + 11 * (k % 12), 230, k)
    return pos, ops + [("M", 60), ("I", 3)] * 200


@MODES
@pytest.mark.parametrize("n", (8, 9, 32, 33, 64))
def test_one_read_of_the_other_promise_goes_through_the_head_and_the_list(ctx, orc, unphased, n):
    """One unpromised read of over six lines among promised ones: it is walked through the head's four lines and then to
    its end from the list, while its neighbours stop inside the head.  And the converse: one promised read among
    unpromised long ones."""
    for at in sorted({0, n // 2, n - 1}):
        batch, idx = _mixed_block(unphased, n, at, _long_tail, lambda k: _stop_read(30 + 11 * (k % 12), 200 + k % 7, k))
        oc, want = orc.call_batch(batch, debug=True)
        assert oc == B.INQ_OK
        for lone_is_promised in (False, True):
            mark_checked(batch)
            assert batch.reads["promise"][idx].all()
            keep = np.zeros(batch.n_reads, dtype=bool)
            keep[idx[at]] = True
            batch.reads["promise"][keep != lone_is_promised] = 0
            assert int((batch.reads["promise"][idx] != 0).sum()) == (1 if lone_is_promised else n - 1)
            rc, got = ctx.call_batch(batch, debug=True, check=False)
            assert rc == B.INQ_OK
            _assert_same(got, want, f"n={n} at {at} lone_is_promised={lone_is_promised}")
    # the same with the long reads in the majority: every read but one goes on to the list
    batch, idx = _mixed_block(unphased, n, n // 3, lambda k: _stop_read(45, 200, k), _long_tail)
    _all_variants(ctx, orc, batch, f"n={n}: long reads around a short one")


@MODES
@pytest.mark.parametrize("n", (1, 8, 33))
def test_domain_errors_inside_the_head_are_the_oracles(ctx, orc, unphased, n):
    """A block of promised reads and one that breaks a domain rule inside the head, so its producer left it unpromised: an
    op code 9 to 15 in its head line 2, a reference position that reaches 2^31 in its head line 3.  The status is the
    oracle's; with the rule mended the block passes under every variant."""
    def bad_op(code, op_at):
        def damage(words):
            words[op_at] = (5 << 4) | code
        return damage

    def far(op_at):
        def damage(words):
            words[op_at : op_at + 8] = (((1 << 28) - 1) << 4) | 0  # eight M of 2^28 - 1 bases: pos + span passes 2^31 at the eighth
        return damage

    for at in sorted({0, n // 2, n - 1}):
        skip = (2 * at) % 8  # (_mixed_block: read `at` starts (at + at) % 8 groups into its line)
        line2 = 4 * (8 - skip)  # the first op of head line 2, from the read's start
        line3 = 4 * (16 - skip)
        cases = [(B.INQ_ERR_CIGAR_OP, bad_op(code, line2 + off)) for code, off in ((9, 0), (12, 13), (15, 31))]
        cases += [(B.INQ_ERR_RANGE, far(line3 + off)) for off in (0, 11, 24)]
        for want_code, damage in cases:
            batch, idx = _mixed_block(unphased, n, at, lambda k: _stop_read(400, 300, k),
                                      lambda k: _stop_read(30 + 11 * (k % 12), 200 + k % 7, k), damage)
            whole = batch.cigar.copy()
            mark_checked(batch)
            assert batch.reads["promise"][idx[at]] == 0 and int((batch.reads["promise"][idx] != 0).sum()) == n - 1
            oc, _ = orc.call_batch(batch)
            rc, _ = ctx.call_batch(batch, debug=True, check=False)
            assert rc == oc == want_code, (n, at, rc, oc, want_code)
        # ... mended: one-base M ops in place of the damage
        o = 4 * int(batch.reads["cigar_off4"][idx[at]])
        batch.cigar[o + line3 : o + line3 + 40] = (1 << 4) | 0
        assert not np.array_equal(batch.cigar, whole)
        _all_variants(ctx, orc, batch, f"n={n} at {at} mended")


@MODES
def test_wide_window_drains_the_queue_inside_the_head(ctx, orc, unphased):
    """A 40 000 bp window: every lane of every line is a window lane, so a step of one slot queues up to 64 window lanes
    and 32 reads queue far more than the 64 that start a drain, several times inside the head.  Soft clips, counted and
    uncounted lengths; some reads end inside the head, some go on to the list."""
    reads = []
    for k in range(40):
        ops = ([("S", 4)] if k % 2 else []) + [("M", 2), ("I", 3 + k % 4), ("M", 1), ("D", 3)] * (6 + 5 * (k % 7))
        if k % 5 == 0:
            ops += [("M", 40), ("D", 5 + k % 3)] * 32 + [("M", 1), ("I", 5)] * 80
        reads.append((k % 8, 1005 + k, ops))
    batch = _batch(unphased, reads, window=(1010, 41000), blocks=(32, 33, 64, 7))
    gen.set_promise(batch, "all")
    groups, lines, head, _ = head_layout(batch)
    assert int(groups[:32].sum()) > 4 * 64 and int((lines > HEAD_LINES).sum()) > 0 and int((lines < HEAD_LINES).sum()) > 0
    _all_variants(ctx, orc, batch, "wide window")
