"""The producer promise (inq_read_t.promise) and the bytes a window-bounded CIGAR walk reads.

`checked_mask` restates the domain rules a producer vouches for with INQ_READ_CHECKED (op codes <= 8,
pos >= -1, pos + 1 + reference span < 2^31); `mark_checked` sets the byte where they hold.

`window_bounded_bytes` counts what the locus kernel's row walk (csrc/cigar_walk.h walk_pairs_rows) reads:
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


def _walked_groups(batch: Batch, piece_ops: int):
    """Per pair: (first 16-byte group of its read, groups the walk loads)."""
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
    # first op i of the read after which carry = pos + 1 + consumed > end_ext
    thr = ee - carry0 + before[r]
    i = np.searchsorted(csum, thr, side="right") - o
    stop_piece = np.where((i >= 0) & (i < n), i // piece_ops, -1)
    groups = np.where(stop_piece >= 0, np.minimum(n4, (stop_piece + 1) * (piece_ops // 4)), n4)
    groups = np.where(carry0 > ee, 0, groups)  # starts past the window: nothing loaded
    # whole reads: no promise, a wrapped window, a block (up to 64 pairs of a locus) that holds a read of 2^23 groups
    # (more than 2^25 - 4 ops), a batch CIGAR of 4 GiB or more
    k = np.arange(batch.n_pairs, dtype=np.int64) - off[locus]
    _, inv = np.unique(locus * (1 << 32) + k // 64, return_inverse=True)
    block_long = np.zeros(inv.max() + 1, dtype=bool)
    np.logical_or.at(block_long, inv, n4 >= ROW_MAX_GROUPS)
    bounded = promised & (ee >= se1) & ~block_long[inv] & (batch.cigar.shape[0] // 4 < (1 << 28))
    return o // 4, np.where(bounded, groups, n4)


def window_bounded_cigar_bytes(batch: Batch, piece_ops: int = 64) -> int:
    """CIGAR bytes the row walk loads for every pair of the batch (pieces of `piece_ops` ops)."""
    if batch.n_pairs == 0:
        return 0
    return int(16 * _walked_groups(batch, piece_ops)[1].sum())


def window_bounded_line_bytes(batch: Batch, piece_ops: int = 64, line: int = 128) -> int:
    """The same stretches counted in whole `line`-byte cache lines: every line a walked stretch touches, once per pair
    (reads start on 16-byte boundaries, so a stretch's first and last lines are usually shared with the neighbours)."""
    if batch.n_pairs == 0:
        return 0
    g0, groups = _walked_groups(batch, piece_ops)
    b0, b1 = g0 * 16, (g0 + groups) * 16
    lines = np.where(groups > 0, (b1 + line - 1) // line - b0 // line, 0)
    return int(line * lines.sum())


def window_bounded_bytes(batch: Batch, piece_ops: int = 64) -> int:
    """`Batch.algorithmic_bytes()` with the CIGAR term replaced by what the window-bounded walk loads."""
    return window_bounded_cigar_bytes(batch, piece_ops) + 20 * batch.n_pairs + 32 * batch.n_loci
