"""The producer promise (inq_read_t.promise) and the bytes a window-bounded CIGAR walk reads.

`checked_mask` restates the domain rules a producer vouches for with INQ_READ_CHECKED (op codes <= 8,
pos >= -1, pos + 1 + reference span < 2^31); `mark_checked` sets the byte where they hold.

`window_bounded_bytes` counts what the locus kernel's row walk (csrc/cigar_walk.h walk_pairs_rows) reads, in pieces
laid from each read's start (the LAYOUTS restate the pieces of earlier walks; `head_layout` is the walk's own now):
a checked read up to the piece after which pos + consumed >= end_ext, in whole 16-byte groups, nothing when
pos >= end_ext already; an unchecked read (or a wrapped window, see walk_pairs for the rest) whole.  Next to it the same per-pair and
per-locus bytes as `Batch.algorithmic_bytes()`, which keeps counting every op.
"""
from __future__ import annotations

import numpy as np

from .batch import INQ_READ_CHECKED, Batch

ROW_MAX_GROUPS = 1 << 23  # cigar_walk.h kRowMaxGroups
CONSUMES_REF = np.zeros(16, dtype=bool)
CONSUMES_REF[[0, 2, 3, 7, 8]] = True  # M D N = X


def _spans(batch: Batch):
    """(inclusive prefix sum of reference-consuming lengths over the whole CIGAR array, int64; per read: span, bad op)."""
    w = batch.cigar.astype(np.int64)
    op = w & 0xF
    ref = np.where(CONSUMES_REF[op], w >> 4, 0)
    csum = np.cumsum(ref)
    o = batch.reads["cigar_off4"].astype(np.int64) * 4
    n = batch.reads["n_cigar"].astype(np.int64)
    before = np.where(o > 0, csum[np.maximum(o - 1, 0)], 0) if csum.size else np.zeros_like(o)
    after = np.where(n > 0, csum[np.maximum(o + n - 1, 0)], before) if csum.size else np.zeros_like(o)
    bad_cum = np.cumsum(op > 8)
    bad_before = np.where(o > 0, bad_cum[np.maximum(o - 1, 0)], 0) if bad_cum.size else np.zeros_like(o)
    bad_after = np.where(n > 0, bad_cum[np.maximum(o + n - 1, 0)], bad_before) if bad_cum.size else np.zeros_like(o)
    return csum, before, after - before, bad_after > bad_before


def checked_mask(batch: Batch) -> np.ndarray:
    """Per read: True where the domain rules of INQ_READ_CHECKED hold."""
    _, _, span, bad = _spans(batch)
    pos = batch.reads["pos"].astype(np.int64)
    return (~bad) & (pos >= -1) & (pos + 1 + span < (1 << 31))


def mark_checked(batch: Batch) -> Batch:
    """Sets INQ_READ_CHECKED on every read whose domain rules hold, clears it on the others (in place)."""
    batch.reads["promise"] = np.where(checked_mask(batch), INQ_READ_CHECKED, 0).astype(np.uint8)
    return batch


LAYOUTS = ("read", "line", "line_half", "tail", "tail_half")
PIECE_GROUPS = 16  # cigar_walk.h kRowLanes: a full piece, two 128-byte lines
HALF_GROUPS = 8  # a half piece: lanes 0-7 of a row, one line
HALF_NUM, HALF_DEN = 7, 8  # the rule's factor, tuned on configs #3 and #5 (profiles/r08_line_pieces/summary.md)
HALF_SAT = (1 << 24) - 1  # the distance to end_ext and the bases covered saturate here: 24-bit multiplies in the kernel


def half_piece_next(d, lim, rtot, c=HALF_GROUPS, num: int = HALF_NUM, den: int = HALF_DEN):
    """THE half-piece rule, stated here once; cigar_walk.h (`half_piece_next` there) computes the same bits.

    After a piece of `lim` lanes (16-byte groups) that covered `rtot` reference bases and left the read `d` = end_ext -
    carry bases short of the window's end, the next piece of a promised read is a half piece - it ends on the next
    128-byte boundary and holds `c` groups, 8 unless the piece before ended inside a line - when such a piece, at the
    last piece's bases per group, is expected to pass end_ext with room to spare:

        d <= (num / den) * rtot * c / lim    <=>    d * lim * den <= num * rtot * c

    in integers, d and rtot each saturated at 2^24 - 1.  For c = 8 this is 2 * d <= (num / den) * rtot * 16 / lim.  With
    num / den = 7 / 8 the kernel evaluates min(d, 2^24 - 1) * (lim * 8) <= min(rtot, 2^24 - 1) * (7 * c).  The choice
    touches speed only: a half piece that falls short is followed by another piece, a full piece where half would have
    done reads one line too many."""
    return np.minimum(d, HALF_SAT) * lim * den <= num * np.minimum(rtot, HALF_SAT) * c


def _bounded(batch: Batch, piece_ops: int):
    """What every layout shares, per pair."""
    csum, before, _, _ = _spans(batch)
    r = batch.pair_read.astype(np.int64)
    off = batch.locus_pair_off.astype(np.int64)
    locus = np.repeat(np.arange(batch.n_loci, dtype=np.int64), np.diff(off))
    ee = (batch.locus_end.astype(np.int64)[locus] + 10) & 0xFFFFFFFF
    se1 = (batch.locus_start.astype(np.int64)[locus] - 9) & 0xFFFFFFFF
    n = batch.reads["n_cigar"].astype(np.int64)[r]
    n4 = (n + 3) // 4
    o = batch.reads["cigar_off4"].astype(np.int64)[r] * 4
    pos = batch.reads["pos"].astype(np.int64)[r]
    carry0 = (pos + 1) & 0xFFFFFFFF
    promised = (batch.reads["promise"][r] & INQ_READ_CHECKED) != 0
    # whole reads: no promise, a wrapped window, a block (up to 64 pairs of a locus) that holds a read of 2^23 groups
    # (more than 2^25 - 4 ops), a batch CIGAR of 4 GiB or more
    k = np.arange(batch.n_pairs, dtype=np.int64) - off[locus]
    _, inv = np.unique(locus * (1 << 32) + k // 64, return_inverse=True)
    block_long = np.zeros(inv.max() + 1, dtype=bool)
    np.logical_or.at(block_long, inv, n4 >= ROW_MAX_GROUPS)
    bounded = promised & (ee >= se1) & ~block_long[inv] & (batch.cigar.shape[0] // 4 < (1 << 28))
    return csum, before[r], ee, n, n4, o, carry0, bounded, inv


def _walked_pieces(batch: Batch, piece_ops: int = 64, layout: str = "read", factor=(HALF_NUM, HALF_DEN)):
    """Per pair: (first 16-byte group of its read, groups the walk loads, pieces it loads them in, its 64-pair block).

    Layouts of the pieces of a read that starts at group g0 (skip = g0 & 7 groups into its 128-byte line):
      "read"       pieces of 16 groups from g0 (what the walk did before the aligned grid)
      "line"       pieces of 16 groups from g0 - skip: piece 0 holds 16 - skip groups of the read, every later one two whole lines
      "line_half"  "line", and from piece 1 on a promised read takes half pieces where `half_piece_next` says so
      "tail"       piece 0 as in "read"; every later piece ends on the second line boundary behind its start, so piece 1
                   holds 16 - skip groups and the rest two whole lines
      "tail_half"  "tail" with half pieces, which end on the first line boundary: piece 1 then holds 8 - skip groups
    A promised read stops after the piece that takes carry = pos + 1 + consumed past end_ext, and loads nothing when it
    starts past it."""
    if layout not in LAYOUTS:
        raise ValueError(f"layout {layout!r}: one of {LAYOUTS}")
    if layout != "read" and piece_ops != 4 * PIECE_GROUPS:
        raise ValueError("the line layouts are pieces of 64 ops")
    csum, before, ee, n, n4, o, carry0, bounded, block = _bounded(batch, piece_ops)
    g0 = o // 4
    full = piece_ops // 4
    skip = g0 & 7 if layout != "read" else np.zeros_like(g0)
    halves = layout.endswith("_half")
    groups = np.zeros_like(n4)
    pieces = np.zeros_like(n4)
    carry = carry0.copy()
    lim = full - skip if layout.startswith("line") else np.full_like(n4, full)
    live = (n4 > 0) & ~(bounded & (carry0 > ee))  # an empty CIGAR, or starts past the window: nothing loaded
    while live.any():
        g_new = np.where(live, np.minimum(groups + lim, n4), groups)
        at = o + np.minimum(4 * g_new, n) - 1
        c_new = np.where(g_new > 0, carry0 + csum[np.maximum(at, 0)] - before, carry0)
        rtot = c_new - carry
        ends = (n4 - groups <= lim) | (bounded & (c_new > ee))
        pieces += live
        groups, carry = g_new, np.where(live, c_new, carry)
        live = live & ~ends
        into = (skip + groups) & 7  # groups of its line that lie before the next piece
        half = bounded & half_piece_next(ee - carry, lim, rtot, HALF_GROUPS - into, *factor) if halves else False
        lim = np.where(half, HALF_GROUPS, full) - into
    return g0, groups, pieces, block


def _walked_groups(batch: Batch, piece_ops: int, layout: str = "read"):
    """Per pair: (first 16-byte group of its read, groups the walk loads)."""
    if layout != "read":
        return _walked_pieces(batch, piece_ops, layout)[:2]
    csum, before, ee, n, n4, o, carry0, bounded, _ = _bounded(batch, piece_ops)
    # first op i of the read after which carry = pos + 1 + consumed > end_ext
    thr = ee - carry0 + before
    i = np.searchsorted(csum, thr, side="right") - o
    stop_piece = np.where((i >= 0) & (i < n), i // piece_ops, -1)
    groups = np.where(stop_piece >= 0, np.minimum(n4, (stop_piece + 1) * (piece_ops // 4)), n4)
    groups = np.where(carry0 > ee, 0, groups)  # starts past the window: nothing loaded
    return o // 4, np.where(bounded, groups, n4)


def window_bounded_cigar_bytes(batch: Batch, piece_ops: int = 64, layout: str = "read") -> int:
    """CIGAR bytes the row walk loads for every pair of the batch (pieces of `piece_ops` ops)."""
    if batch.n_pairs == 0:
        return 0
    return int(16 * _walked_groups(batch, piece_ops, layout)[1].sum())


def window_bounded_line_bytes(batch: Batch, piece_ops: int = 64, line: int = 128, layout: str = "read") -> int:
    """The same stretches counted in whole `line`-byte cache lines: every line a walked stretch touches, once per pair
    (reads start on 16-byte boundaries, so a stretch's first and last lines are usually shared with the neighbours)."""
    if batch.n_pairs == 0:
        return 0
    g0, groups = _walked_groups(batch, piece_ops, layout)
    b0, b1 = g0 * 16, (g0 + groups) * 16
    lines = np.where(groups > 0, (b1 + line - 1) // line - b0 // line, 0)
    return int(line * lines.sum())


def row_steps(batch: Batch, layout: str = "read", factor=(HALF_NUM, HALF_DEN)) -> float:
    """Row-steps of the walk over the batch, the instruction side's estimate: a block of cnt <= 64 pairs takes ceil(cnt / 4)
    piece-0 turns, and its pieces behind piece 0 are shared among the four rows."""
    if batch.n_pairs == 0:
        return 0.0
    _, groups, pieces, block = _walked_pieces(batch, 64, layout, factor)
    cnt = np.bincount(block)
    later = pieces - (pieces > 0)
    return float(((cnt + 3) // 4).sum() + later.sum() / 4.0)


HEAD_LANES = 8  # cigar_walk.h kHeadLanes: a row of the head phase, one 128-byte line per load
HEAD_LINES = 4  # cigar_walk.h kHeadLines


def head_layout(batch: Batch, head_lines: int = HEAD_LINES):
    """What the row walk does since its head phase (cigar_walk.h walk_pairs_rows), per pair: (groups it loads, 128-byte lines
    it loads, lines of them that the head walks), and the head steps of the whole batch.

    A read that starts skip = g0 & 7 groups into its line is walked one line at a time: 8 - skip groups, then whole lines,
    the stop rule of `_walked_pieces` after each, up to `head_lines` lines; no line is asked for twice.  What is left then
    goes on in pieces of two whole lines.  A block of up to 64 pairs is walked in passes of 32: pair k of the pass is row
    k % 8 of load slot k // 8 throughout, and a slot is stepped while one of its eight reads is live - so a slot costs as
    many head steps as the most lines any of its reads needs.  (A block without a promised read takes the whole walk, which
    has no head; its reads are counted here as the row walk would take them.)"""
    if batch.n_pairs == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z, 0
    csum, before, ee, n, n4, o, carry0, bounded, block = _bounded(batch, 4 * PIECE_GROUPS)
    g0 = o // 4
    groups = np.zeros_like(n4)
    head = np.zeros_like(n4)
    live = (n4 > 0) & ~(bounded & (carry0 > ee))  # an empty CIGAR, or starts past the window: nothing loaded
    lim = HEAD_LANES - (g0 & 7)
    piece = 0
    while live.any():
        g_new = np.where(live, np.minimum(groups + lim, n4), groups)
        at = o + np.minimum(4 * g_new, n) - 1
        c_new = np.where(g_new > 0, carry0 + csum[np.maximum(at, 0)] - before, carry0)
        ends = (n4 - groups <= lim) | (bounded & (c_new > ee))
        piece += 1
        if piece <= head_lines:
            head += live
        groups = g_new
        live = live & ~ends
        lim = np.full_like(n4, HEAD_LANES if piece < head_lines else PIECE_GROUPS)
    lines = np.where(groups > 0, ((g0 + groups) * 16 + 127) // 128 - (g0 * 16) // 128, 0)
    off = batch.locus_pair_off.astype(np.int64)
    k = np.arange(batch.n_pairs, dtype=np.int64) - np.repeat(off[:-1], np.diff(off))
    slot = block * 8 + (k % 64) // HEAD_LANES  # 64-pair block, then its eight slots of eight reads: passes of four slots
    per_slot = np.zeros(int(slot.max()) + 1, dtype=np.int64)
    np.maximum.at(per_slot, slot, head)
    return groups, lines, head, int(per_slot.sum())


def window_bounded_bytes(batch: Batch, piece_ops: int = 64) -> int:
    """`Batch.algorithmic_bytes()` with the CIGAR term replaced by what the window-bounded walk loads."""
    return window_bounded_cigar_bytes(batch, piece_ops) + 20 * batch.n_pairs + 32 * batch.n_loci
