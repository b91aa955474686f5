"""Seeded random test-case generator: python Records per locus + the packed Batch.

Shapes follow the edge cases the reference's semantics make interesting:
reads ending exactly on window edges, fully-inside reads, low mapq, missing / zero HP,
soft clips with and without a 2D supplementary alignment, every CIGAR op, empty CIGARs,
unmapped-but-placed reads, reads shared by neighbouring loci, empty loci, long CIGARs.
"""
from __future__ import annotations

import dataclasses
import functools
import random
from typing import List, Tuple

import numpy as np

from inquistr_amd.batch import Batch, BatchBuilder, encode_cigar
from oracle import pyoracle as py


def random_cigar(rng: random.Random, n_ops: int, big: bool = False) -> List[Tuple[str, int]]:
    ops = []
    for i in range(n_ops):
        r = rng.random()
        if i % 2 == 0 or r < 0.15:
            op = rng.choice("MMMMMM=X")
            ln = rng.randint(1, 60)
        elif r < 0.50:
            op, ln = "I", rng.choice([1, 2, 3, 5, 6, 7, 12, 40, 300])
        elif r < 0.85:
            op, ln = "D", rng.choice([1, 2, 4, 5, 6, 9, 15, 33])
        elif r < 0.90:
            op, ln = "N", rng.randint(1, 80)
        elif r < 0.94:
            op, ln = "S", rng.choice([3, 5, 6, 20, 150])
        elif r < 0.97:
            op, ln = "H", rng.randint(1, 50)
        else:
            op, ln = "P", rng.randint(1, 5)
        if big and rng.random() < 0.02:
            op, ln = "I", rng.randint(5000, 50000)
        ops.append((op, ln))
    return ops


def random_locus_reads(rng: random.Random, start: int, end: int, n: int, long_every: int = 0) -> List[py.Record]:
    start_ext, end_ext = start - 10, end + 10
    recs = []
    for k in range(n):
        style = rng.random()
        if style < 0.55:  # spanning read
            pos = start_ext - rng.randint(0, 400)
        elif style < 0.65:  # starts exactly on / next to the window edge
            pos = start_ext + rng.choice([-1, 0, 1])
        elif style < 0.80:  # starts inside the window
            pos = rng.randint(start_ext, end_ext)
        elif style < 0.90:  # far left, may or may not reach
            pos = start_ext - rng.randint(300, 900)
        else:  # at / beyond the right edge
            pos = end_ext + rng.choice([-2, -1, 0, 1, 50])
        pos = max(pos, 0)
        n_ops = rng.choice([0, 1, 2, 3, 5, 9, 17, 30, 63, 64, 65])
        if long_every and k % long_every == 0:
            n_ops = rng.choice([255, 256, 257, 300, 511, 513, 700, 1500])
        cig = random_cigar(rng, n_ops, big=rng.random() < 0.1)
        # sometimes force the read to end exactly on the right edge of the window
        if cig and rng.random() < 0.15:
            rlen = sum(l for o, l in cig if o in "MDN=X")
            want = end_ext - pos + rng.choice([-1, 0, 0, 1])
            if want > rlen:
                cig.append(("M", want - rlen))
        flag = 0
        if rng.random() < 0.3:
            flag |= 0x10
        if rng.random() < 0.03:
            flag |= 0x4
        hp = None
        r = rng.random()
        if r < 0.40:
            hp = ("C", 1)
        elif r < 0.80:
            hp = ("C", 2)
        elif r < 0.88:
            hp = ("C", 0)
        elif r < 0.92:
            hp = ("i", rng.choice([1, 2, 257, 258]))
        sa = None
        if rng.random() < 0.25:
            strand = rng.choice("+-")
            sa_pos = pos + rng.randint(-200, 200)
            entry = f"chr7,{sa_pos},{strand},{rng.randint(1, 300)}M{rng.randint(1, 50)}S,60,0;"
            if rng.random() < 0.15:
                entry += "chr2,100,+,50M,0,0;"
            sa = ("Z", entry)
        mapq = rng.choice([0, 5, 10, 11, 20, 60, 60, 60, 60])
        recs.append(py.Record(pos=pos, cigar=cig, mapq=mapq, flag=flag, hp=hp, sa=sa))
    return recs


def random_case(seed: int, n_loci: int = 40, unphased: bool = False, minlen: int = 5, support: int = 3,
                max_reads: int = 40, long_every: int = 0, share: bool = True):
    """Returns (Batch, per-locus python records)."""
    rng = random.Random(seed)
    bb = BatchBuilder(minlen=minlen, support=support, unphased=unphased)
    per_locus: List[List[py.Record]] = []
    cursor = 2000
    prev: List[Tuple[int, py.Record]] = []
    for j in range(n_loci):
        start = cursor + rng.randint(0, 300)
        end = start + rng.randint(0, 250)
        cursor = end + rng.randint(30, 1500)
        n = rng.choice([0, 1, 2, 3, 5, 6, 7, 12, 20, max_reads])
        if j == 1 and max_reads > 40:
            n = max_reads  # deep-locus tests need the depth they ask for
        recs = random_locus_reads(rng, start, end, n, long_every)
        idx = []
        merged: List[py.Record] = []
        # neighbouring loci share some reads (a read overlapping k loci is offered k times)
        if share and prev and rng.random() < 0.5:
            for ri, r in prev[: rng.randint(1, 4)]:
                idx.append(ri)
                merged.append(r)
        cur = []
        for r in recs:
            phase = py.get_phase(r)
            ri = bb.add_read(
                pos=r.pos,
                cigar_words=encode_cigar(r.cigar),
                mapq=r.mapq,
                phase=phase,
                reverse=bool(r.flag & 0x10),
                unmapped=bool(r.flag & 0x4),
                is_2d=py.is_accidental_2d(r),
            )
            idx.append(ri)
            merged.append(r)
            cur.append((ri, r))
        # "file order" = increasing position, ties by insertion (like a coordinate-sorted BAM)
        order = sorted(range(len(idx)), key=lambda k: (merged[k].pos, idx[k]))
        idx = [idx[k] for k in order]
        merged = [merged[k] for k in order]
        bb.add_locus(start, end, idx)
        per_locus.append(merged)
        prev = cur
    return bb.build(), per_locus


def py_expected(batch: Batch, per_locus) -> Tuple[np.ndarray, np.ndarray, int]:
    p1 = np.full(batch.n_loci, np.nan)
    p2 = np.full(batch.n_loci, np.nan)
    ties = 0
    for j, recs in enumerate(per_locus):
        s, e = int(batch.locus_start[j]), int(batch.locus_end[j])
        if batch.unphased:
            a, b, t = py.genotype_repeat_unphased(recs, 0, s, e, batch.minlen, batch.support)
            ties += int(t)
        else:
            a, b = py.genotype_repeat_phased(recs, 0, s, e, batch.minlen, batch.support)
        p1[j], p2[j] = a, b
    return p1, p2, ties


def same_f64(a: np.ndarray, b: np.ndarray) -> bool:
    """Bit-exact up to NaN payload: NaNs must coincide, everything else must be equal."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((np.isnan(a) & np.isnan(b)) | (a == b)))


def mixed_depth_case(seed: int, case_index: int = 0):
    """One batch that mixes the depth classes of DESIGN.md 3.2 - <= 64 offered reads, 65 - 256, 257 - 2 048 (reduced by the workgroup
    that walked them), 2 049 - 16 384, several loci of 16 385 - 65 536 (walked by a group of workgroups each) and, every fourth
    case_index, one locus beyond 65 536 (the whole grid) -, reads drawn from a pool of shapes (ties everywhere) plus reads with ONE
    indel of a wide range of lengths inside the window (Calls of many distinct values), HP / mapq / strand / 2D bits random per read,
    `support` from 1 to beyond a group's size.  Returns (Batch, depths)."""
    rng = random.Random(seed)
    unphased = bool(case_index & 1)
    support = rng.choice([1, 2, 3, 3, 5, 40, 700, 9000])
    minlen = rng.choice([5, 0, 12])
    start, end = 700_000, 700_000 + rng.choice([0, 40, 140])
    shapes = random_locus_reads(rng, start, end, rng.choice([12, 60, 200]), long_every=rng.choice([0, 7]))
    wide = rng.choice([3, 40, 3000])
    for _ in range(rng.choice([0, 100, 400])):
        pos = start - 10 - rng.randint(1, 300)
        op = rng.choice("IIID")
        ln = rng.randint(1, wide) if op == "I" else rng.randint(1, 30)
        lead = ("S", rng.choice([4, 30])) if rng.random() < 0.1 else None
        cig = ([lead] if lead else []) + [("M", start - pos + rng.randint(0, end - start + 5)), (op, ln), ("M", 400)]
        shapes.append(py.Record(pos=pos if not lead else start + rng.randint(-5, 5), cigar=cig, mapq=60, flag=rng.choice([0, 16])))
    n_pool = 72_000 if case_index % 4 == 0 else rng.choice([21_000, 30_000, 40_000])
    pool = [(shapes[rng.randrange(len(shapes))], rng.choice([9, 60, 60, 60]), rng.choice([None, 0, 1, 1, 2, 2]), rng.random() < 0.15) for _ in range(n_pool)]
    bb = BatchBuilder(minlen=minlen, support=support, unphased=unphased)
    ids = [bb.add_read(r.pos, encode_cigar(r.cigar), mapq=mq, phase=ph, reverse=bool(r.flag & 0x10), is_2d=twod) for r, mq, ph, twod in pool]
    order = sorted(range(len(ids)), key=lambda k: (bb._reads[ids[k]][2], k))
    depths = []
    for lo_d, hi_d, cnt in ((1, 64, 6), (65, 256, 5), (257, 2048, 5), (2049, 16384, 3), (16385, min(65536, n_pool), rng.choice([2, 5, 9]))):
        depths += [rng.randint(lo_d, hi_d) for _ in range(cnt)]
    if n_pool > 65_536:
        depths.append(rng.randint(65_537, n_pool))
    depths += [64, 65, 256, 257, 2048, 2049, 16384, 16385][: rng.randint(0, 8)]
    rng.shuffle(depths)
    for d in depths:
        off = rng.randint(0, n_pool - d)
        sh = rng.choice([-10, 0, 0, 10])  # (windows shifted against each other: not every locus sees the same Calls)
        bb.add_locus(start + sh, end + sh, [ids[k] for k in order[off : off + d]])
    return bb.build(), depths


# ---- promise variants -------------------------------------------------------------------------------------------
# Which reads of a batch carry the producer promise (inq_read_t.promise = INQ_READ_CHECKED) decides which walk a
# block of 64 pairs takes (csrc/cigar_walk.h walk_pairs) and, inside the row walk, which reads stop at the window.
# The oracle never reads the byte, so one oracle result serves every variant of a batch.

PROMISE_VARIANTS = ("none", "all", "half", "lone_promise", "lone_unpromised")
DEEP_PROMISE_VARIANTS = ("none", "all", "half")  # for batches whose every call is expensive


def checked_share(batch: Batch) -> float:
    """Share of the batch's reads that `mark_checked` promises (1.0 when the batch is empty)."""
    from inquistr_amd.window_bytes import checked_mask

    return float(checked_mask(batch).mean()) if batch.n_reads else 1.0


def _blocks(batch: Batch):
    """Per pair: the index of its block (up to 64 consecutive pairs of one locus); per block: its first pair, its size."""
    off = batch.locus_pair_off.astype(np.int64)
    assert off[0] == 0 and off[-1] == batch.n_pairs and (np.diff(off) >= 0).all(), "set the variant before damaging the layout"
    n = np.diff(off)
    nblk = (n + 63) // 64
    blk0 = np.concatenate([[0], np.cumsum(nblk)])
    locus = np.repeat(np.arange(batch.n_loci, dtype=np.int64), n)
    k = np.arange(batch.n_pairs, dtype=np.int64) - off[locus]
    block = blk0[locus] + k // 64
    first = np.repeat(off[:-1], nblk) + 64 * (np.arange(int(blk0[-1]), dtype=np.int64) - np.repeat(blk0[:-1], nblk))
    size = np.minimum(64, np.repeat(off[1:], nblk) - first)
    return block, first, size


def set_promise(batch: Batch, variant: str, seed: int = 0) -> str:
    """Rewrites batch.reads["promise"] in place to one of PROMISE_VARIANTS and returns a name for messages and ids.

    Every variant is `mark_checked(batch)` AND a mask, so no variant makes a false promise:
      none             nothing promised (what BatchBuilder leaves)
      all              every read whose domain rules hold
      half             a seeded Bernoulli(0.5) draw per read
      lone_promise     one read of every 64-pair block, the rest of the block unpromised (where loci share reads a read
                       is promised if any block chose it: at least one per block, not exactly one)
      lone_unpromised  the converse
    For half and lone_* the draw is repeated (seed, seed + 1, ...) until some block holds both kinds, whenever a block
    with two distinct promisable reads exists; the function asserts that, and the per-block rule of lone_*."""
    from inquistr_amd.batch import INQ_READ_CHECKED
    from inquistr_amd.window_bytes import checked_mask

    assert variant in PROMISE_VARIANTS, variant
    name = f"promise={variant}"
    if batch.n_reads == 0:
        return name
    ok = checked_mask(batch)

    def store(mask):
        batch.reads["promise"] = np.where(ok & mask, INQ_READ_CHECKED, 0).astype(np.uint8)
        assert not (batch.reads["promise"].astype(bool) & ~ok).any(), "a variant never sets a false promise"
        return name

    if variant == "none":
        return store(np.zeros(batch.n_reads, dtype=bool))
    if variant == "all":
        return store(np.ones(batch.n_reads, dtype=bool))
    if batch.n_pairs == 0:
        return store(np.zeros(batch.n_reads, dtype=bool))
    block, first, size = _blocks(batch)
    n_blocks = int(first.shape[0])
    r = batch.pair_read.astype(np.int64)
    assert (r < batch.n_reads).all(), "set the variant before damaging the layout"
    good = ok[r]  # per pair: its read may be promised
    # per block: the smallest and the largest promisable read index (two distinct ones <=> they differ)
    lo = np.full(n_blocks, batch.n_reads, dtype=np.int64)
    hi = np.full(n_blocks, -1, dtype=np.int64)
    np.minimum.at(lo, block[good], r[good])
    np.maximum.at(hi, block[good], r[good])
    has_good = hi >= 0
    can_mix = bool((hi > lo).any())

    def per_block_counts(mask):
        promised = np.bincount(block, weights=(good & mask[r]).astype(np.float64), minlength=n_blocks)
        unpromised = np.bincount(block, weights=(good & ~mask[r]).astype(np.float64), minlength=n_blocks)
        return promised, unpromised

    for attempt in range(64):
        rng = np.random.default_rng([seed + attempt, PROMISE_VARIANTS.index(variant)])
        if variant == "half":
            mask = rng.random(batch.n_reads) < 0.5
        else:
            # one promisable pair of every block that has one: the u-th of its promisable pairs
            gcount = np.bincount(block, weights=good.astype(np.float64), minlength=n_blocks).astype(np.int64)
            pick_rank = (rng.random(n_blocks) * np.maximum(gcount, 1)).astype(np.int64)
            rank = np.cumsum(good) - 1  # rank of a promisable pair among all promisable pairs
            base = np.concatenate([[0], np.cumsum(gcount)])[:-1]
            chosen_pair = np.nonzero(good & (rank - base[block] == pick_rank[block]))[0]
            assert chosen_pair.shape[0] == int(has_good.sum())
            chosen = np.zeros(batch.n_reads, dtype=bool)
            chosen[r[chosen_pair]] = True
            mask = chosen if variant == "lone_promise" else ~chosen
        promised, unpromised = per_block_counts(mask)
        if not can_mix or bool(((promised > 0) & (unpromised > 0)).any()):
            break
    else:
        raise AssertionError(f"{name}: no block holds both kinds after 64 draws")
    if variant == "lone_promise":
        assert (promised[has_good] >= 1).all(), "every block with a promisable read holds a promised one"
    if variant == "lone_unpromised":
        assert (unpromised[has_good] >= 1).all(), "every block with a promisable read holds an unpromised one"
    return store(mask)


def promise_variants(batch: Batch, variants=PROMISE_VARIANTS, seed: int = 0):
    """Sets each variant in turn on the same batch and yields its name."""
    for v in variants:
        yield set_promise(batch, v, seed)


# ---- cases shaped after the row walk (csrc/cigar_walk.h walk_pairs_rows) -------------------------------------------
# The dimensions are the kernel's: pairs per locus around the tiers of the locus kernels, ops per read around the
# 64-op piece and the "at most 16 groups left" test, the piece in which a promised read passes end_ext, window widths
# that make the lane queue drain many times, runs of reads claim() settles without a load.

ROW_DEPTHS_SMALL = (1, 2, 3, 4, 5, 16, 17, 63, 64)  # one wave, one block
ROW_DEPTHS_MID = (65, 128, 129, 256, 257, 300)  # wave_locus<4>; walk_locus with the in-place reduce
ROW_DEPTHS_DEEP = (2048, 2049)  # walk_locus: the last in-place reduce, the first into the tail kernel
ROW_OPS = (0, 1, 3, 4, 5, 60, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 5000)
ROW_WIDTHS = (0, 1, 100, 5_000, 40_000)
ROW_STOP_PIECES = (0, 1, 2, 5, 9)
_CONSUMES = np.zeros(16, dtype=bool)
_CONSUMES[[0, 2, 3, 7, 8]] = True


def _short_ops(rng, n, max_m):
    """n ops: M runs of 1 .. max_m bases alternating with short I / D / S ops (lengths on both sides of every minlen in use)."""
    op = np.where(np.arange(n) % 2 == 0, 0, rng.choice([1, 1, 2, 2, 4], size=n))
    ln = np.where(op == 0, rng.integers(1, max_m + 1, size=n), rng.choice([1, 2, 3, 4, 9, 13, 14], size=n))
    return op.astype(np.int64), ln.astype(np.int64)


def _span(op, ln):
    return int(ln[_CONSUMES[op]].sum())


def row_walk_case(seed: int, unphased: bool = None, max_depth: int = None):
    """One batch around a main window (end_ext = ee) plus shifted and narrow windows over the same reads.
    Returns (Batch, info); info["per_locus"] holds pyoracle Records per locus when the case is small enough for the
    Python oracle, else None; info["depths"], info["width"], info["stop_pieces"], info["settled_runs"] describe the draw."""
    rng = np.random.default_rng([seed, 20260])
    if unphased is None:
        unphased = bool(seed & 1)
    minlen = (0, 2, 12)[seed % 3]
    support = (1, 3)[(seed // 3) % 2]
    width = ROW_WIDTHS[seed % 5]
    start = 200_000 + int(rng.integers(0, 1000))
    end = start + width
    se, ee = start - 10, end + 10
    bb = BatchBuilder(minlen=minlen, support=support, unphased=unphased)
    attrs = []  # per read: (pos, flag, hp, sa, mapq) for the Python oracle
    stop_pieces = set()

    def add(pos, op, ln, settled=False):
        words = ((ln << 4) | op).astype(np.uint32)
        reverse, unmapped = bool(rng.random() < 0.3), bool(rng.random() < 0.03)
        mapq = int(rng.choice([5, 60, 60, 60]))
        phase = [None, 0, 1, 1, 2, 2][int(rng.integers(0, 6))]
        twod = bool(rng.random() < 0.2)
        sa = None
        if twod:  # one supplementary alignment on the other strand over the read's own start: is_accidental_2d
            sa = ("Z", f"chr7,{pos},{'+' if reverse else '-'},{max(1, _span(op, ln))}M,60,0;")
        attrs.append((pos, (0x10 if reverse else 0) | (0x4 if unmapped else 0), None if phase is None else ("C", phase), sa, mapq))
        return bb.add_read(pos, words, mapq=mapq, phase=phase, reverse=reverse, unmapped=unmapped, is_2d=twod)

    def edge_read():
        """The first 64 * (P + 1) ops take pos + consumed to ee + d exactly: a promised read stops after piece P (d >= 0)
        or one piece later (d < 0); with fewer ops than that, the stop and the read's end fall into the same piece."""
        n = int(rng.choice(ROW_OPS))
        op, ln = _short_ops(rng, n, 3)
        p = min(int(rng.choice(ROW_STOP_PIECES)), max(0, (n - 1) // 64))
        cut = min(n, 64 * (p + 1))
        d = int(rng.choice([-2, -1, 0, 1]))
        if n:
            stop_pieces.add(p)
        return add(ee + d - _span(op[:cut], ln[:cut]), op, ln)

    def wide_read(n=None):
        """1 - 30 bp M runs between short I / D / S ops, starting up to a third of its span left of the window."""
        n = int(rng.choice(ROW_OPS)) if n is None else n
        op, ln = _short_ops(rng, n, 30)
        return add(se - int(rng.integers(0, max(1, _span(op, ln) // 3) + 1)), op, ln)

    def any_op_read():
        n = int(rng.choice(ROW_OPS))
        op = rng.choice([0, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8], size=n).astype(np.int64)
        ln = rng.integers(1, 61, size=n).astype(np.int64)
        pos = se - int(rng.integers(0, 400)) if rng.random() < 0.7 else int(rng.integers(se, ee + 1))
        return add(pos, op, ln)

    def neg_read():
        op, ln = _short_ops(rng, int(rng.choice([5, 64, 129, 1000])), 30)
        op = np.concatenate([[0], op])
        ln = np.concatenate([[se - int(rng.integers(0, 300))], ln])
        return add(-1, op, ln)

    first = wide_read(int(rng.choice([1, 5, 64, 257])))  # the read at cigar_off4 == 0
    pool = [first]
    for _ in range(40):
        r = rng.random()
        pool.append(edge_read() if r < 0.40 else wide_read() if r < 0.75 else any_op_read() if r < 0.93 else neg_read())
    # reads claim() settles without a load: no CIGAR at all, or (promised) a start at or past end_ext of every window here;
    # pos = ee - 1 (pos + 1 == end_ext of the main window) is the last start that is NOT settled
    far = ee + 200
    settled = [add(int(rng.integers(se - 50, far)), np.zeros(0, np.int64), np.zeros(0, np.int64)) for _ in range(2)]
    for pos in (far, far + 1, far + 40_000):
        op, ln = _short_ops(rng, int(rng.choice([1, 64, 200])), 30)
        settled.append(add(pos, op, ln))
    for pos in (ee - 1, ee, ee + 1):
        op, ln = _short_ops(rng, int(rng.choice([3, 65, 129])), 30)
        pool.append(add(pos, op, ln))
    last = wide_read(int(rng.choice([1, 4, 63, 129])))  # its last group is the batch's last
    pool.append(last)

    depths = [int(x) for x in rng.choice(ROW_DEPTHS_SMALL, size=3)] + [ROW_DEPTHS_MID[seed % 6]]
    depths.append(ROW_DEPTHS_DEEP[(seed // 4) % 2] if seed % 4 == 0 else int(rng.choice(ROW_DEPTHS_SMALL + ROW_DEPTHS_MID)))
    if max_depth is not None:
        depths = [d for d in depths if d <= max_depth]
    windows = [(start, end), (start, end), (start - 25, end - 25), (start + 15, end + 15), (ee - 15, ee - 14)]
    loci = []
    settled_runs = []
    for k, depth in enumerate(depths):
        idx = [int(x) for x in rng.choice(pool, size=depth)]  # with replacement: a read may be offered twice to one locus
        nblk = (depth + 63) // 64
        b = int(rng.integers(0, nblk))
        size = min(64, depth - 64 * b)
        run = min(size, int(rng.choice([1, 2, 3, 4, 5, 8, 16, 33, 64])))
        at = 64 * b + (0, (size - run) // 2, size - run)[int(rng.integers(0, 3))]
        idx[at : at + run] = [int(x) for x in rng.choice(settled, size=run)]
        settled_runs.append(run)
        if depth >= 128 and rng.random() < 0.6:  # one block made only of them
            b2 = (b + 1) % nblk
            size2 = min(64, depth - 64 * b2)
            idx[64 * b2 : 64 * b2 + size2] = [int(x) for x in rng.choice(settled, size=size2)]
            settled_runs.append(size2)
        loci.append((windows[k % len(windows)] if k else windows[0], idx))
    loci.append((windows[0], [first, last, first]))
    order = rng.permutation(len(loci))
    per_locus_idx = []
    for k in order:
        (s, e), idx = loci[int(k)]
        bb.add_locus(s, e, idx)
        per_locus_idx.append(idx)
    batch = bb.build()
    assert batch.reads["cigar_off4"][first] == 0 and batch.reads["n_cigar"][first] > 0
    assert int(batch.reads["cigar_off4"][last]) + (int(batch.reads["n_cigar"][last]) + 3) // 4 == batch.cigar.shape[0] // 4
    info = {"depths": [len(x) for x in per_locus_idx], "width": width, "stop_pieces": stop_pieces, "settled_runs": settled_runs,
            "per_locus": None}
    # the Python oracle walks op by op, and looks at the SA entry (a second walk of the CIGAR) at every S op
    n_ops = batch.reads["n_cigar"].astype(np.int64)
    n_s = np.array([int(((batch.cigar[4 * int(o) : 4 * int(o) + int(n)] & 15) == 4).sum()) if attrs[i][3] else 0
                    for i, (o, n) in enumerate(zip(batch.reads["cigar_off4"], n_ops))], dtype=np.int64)
    r = batch.pair_read.astype(np.int64)
    if int((n_ops[r] * (1 + n_s[r])).sum()) <= 400_000:
        recs = {}
        for i in set(int(x) for x in r):
            w = batch.cigar[4 * int(batch.reads["cigar_off4"][i]) : 4 * int(batch.reads["cigar_off4"][i]) + int(n_ops[i])]
            pos, flag, hp, sa, mapq = attrs[i]
            recs[i] = py.Record(pos=pos, cigar=[(py.OPS[int(x) & 15], int(x) >> 4) for x in w], mapq=mapq, flag=flag, hp=hp, sa=sa)
        info["per_locus"] = [[recs[i] for i in idx] for idx in per_locus_idx]
    return batch, info


# ---- cases shaped after the launch geometry of the work-list kernels (csrc/kernels.hip walk_part, csrc/deep_select.hip) ------
# How many workgroups locus_call_mid_walk and locus_call_tail are launched with ("grid_medium", "grid_tail") decides how the three
# work lists are dealt, how a locus of more than kWalkSplit reads is split over a group of workgroups and what slice of a locus of
# more than kGridSelectMin reads a workgroup takes in every pass of the grid-wide select.  These batches put loci on every list.

# the smallest depths on both sides of kMediumSlots * 64 (64 | 65 is the list threshold itself), kReduceInPlace, kWalkSplit and
# kGridSelectMin, and a few between the last two: six loci on list 2, two of them the whole grid's
LADDER_DEPTHS = (0, 1, 64, 65, 256, 257, 2048, 2049, 16384, 16385, 20000, 30000, 65536, 65537, 70001)
LADDER_POOL = 70_001


@functools.lru_cache(maxsize=2)
def _ladder_layout(seed: int):
    rng = random.Random(seed)
    start, end = 900_000, 900_140
    shapes = random_locus_reads(rng, start, end, 60, long_every=9)  # few shapes: ties everywhere
    # ... and as many reads that cross every window of the ladder with an insertion or a soft clip of 6 / 8 / 20 bases every 30 - 60
    # bases: their Calls are the sums of what lies inside a window - other sums in every window, the same sum as Span and as Clip
    for _ in range(60):
        cig, span = [], 0
        while span < 620:
            m = rng.choice([30, 45, 60])
            cig += [("M", m), (rng.choice("IIIS"), rng.choice([6, 8, 20]))]
            span += m
        shapes.append(py.Record(pos=start - 260 - rng.randint(0, 20), cigar=cig + [("M", 50)], mapq=60, flag=rng.choice([0, 16])))
    pool = [(shapes[rng.randrange(len(shapes))], rng.choice([9, 60, 60, 60]), rng.choice([None, 0, 1, 1, 2, 2]), k % 7 == 0) for k in range(LADDER_POOL)]
    bb = BatchBuilder(minlen=5, support=3, unphased=False)
    ids = [bb.add_read(r.pos, encode_cigar(r.cigar), mapq=mq, phase=ph, reverse=bool(r.flag & 0x10), is_2d=twod) for r, mq, ph, twod in pool]
    order = sorted(range(len(ids)), key=lambda k: (bb._reads[ids[k]][2], k))  # file order: by position, then insertion
    loci = []
    for k, d in enumerate(LADDER_DEPTHS):
        # every step-th read of the file order from a random first one: a shallow locus too draws from the whole range of
        # positions (64 neighbours of the file order start within a base or two of each other and may all miss the window)
        step = LADDER_POOL // max(d, 1)
        off = rng.randint(0, LADDER_POOL - step * d)
        sh = 14 * k - 98  # every locus its own window, the deeper the wider: no two see the same Calls
        loci.append((d, start + sh, end + sh + 9 * k, [ids[i] for i in order[off : off + step * d : step]]))
    rng.shuffle(loci)
    for d, s, e, idx in loci:
        bb.add_locus(s, e, idx)
    return bb.build(), tuple(d for d, _, _, _ in loci)


def depth_ladder_case(seed: int, unphased: bool, support: int):
    """One locus at each depth of LADDER_DEPTHS, every one a file-ordered slice (every step-th read) of one pool of 70 001 reads
    drawn from 120 shapes - random_locus_reads' and reads with an insertion or soft clip every few dozen bases -, with 2D reads,
    mapq 9 / 60, phases none / 0 / 1 / 2; each locus has its own window, shifted and the deeper the wider.  The reads and the layout depend on
    `seed` only and are built once; `unphased` and `support` are the batch's scalars.  Returns (Batch, depth of every locus)."""
    base, depths = _ladder_layout(seed)
    return dataclasses.replace(base, reads=base.reads.copy(), support=support, unphased=unphased), list(depths)


def group_counts(batch: Batch, probe, locus: int):
    """Per haplotype group of `locus` (1, 2): (its Calls, the spanning ones among them), from the per-pair outputs of an oracle run
    of the batch (they do not depend on `support`).  Phased: the kept reads of HP 1 / 2.  Unphased: h1 = the lower half of the kept
    Calls, ties in file order (src/call.rs:311-313), h2 the rest."""
    p0, p1 = int(batch.locus_pair_off[locus]), int(batch.locus_pair_off[locus + 1])
    bits = probe.pair_bits[p0:p1].astype(np.int64)
    kept = (bits & 4) != 0
    if batch.unphased:
        at = np.nonzero(kept)[0]
        at = at[np.argsort(probe.pair_call[p0:p1][at], kind="stable")]
        grp = np.zeros(p1 - p0, dtype=np.int64)
        grp[at[: at.shape[0] // 2]] = 1
        grp[at[at.shape[0] // 2 :]] = 2
    else:
        grp = np.where(kept, batch.reads["phase"][batch.pair_read[p0:p1]].astype(np.int64), 0)
    return {g: (int((grp == g).sum()), int(((grp == g) & ((bits & 1) == 0)).sum())) for g in (1, 2)}


def clip_rule_support(batch: Batch, probe, locus: int):
    """A `support` at which median_str_length's clip rule (src/call.rs:509-513) bites on `locus`: for the haplotype group that
    holds more clipped Calls, more than its spanning Calls - so that half of its clipped Calls, the largest, ties at the threshold
    included, join them - and no more than the group holds.  Returns (support, the group, its Calls, the spanning ones among them)."""
    counts = group_counts(batch, probe, locus)
    g = max(counts, key=lambda k: counts[k][0] - counts[k][1])
    ng, ns = counts[g]
    assert ng - ns >= 2, "the group needs clipped Calls for the rule to pick from"
    return ns + (ng - ns) // 2, g, ng, ns


@functools.lru_cache(maxsize=1)
def _listed_pool():
    rng = random.Random(4242)
    start, end = 300_000, 300_120
    shapes = random_locus_reads(rng, start, end, 40, long_every=9)
    return start, end, [(shapes[rng.randrange(len(shapes))], rng.choice([9, 60, 60, 60]), rng.choice([None, 0, 1, 1, 2, 2]), k % 7 == 0) for k in range(700)]


def all_listed_case(n_loci: int, depth: int, unphased: bool = False, support: int = 3) -> Batch:
    """`n_loci` loci of depth .. depth + 3 reads each - every one on a work list when depth > 64 -, file-ordered slices of one pool
    of 700 reads, windows shifted against each other."""
    start, end, pool = _listed_pool()
    assert depth + 3 <= len(pool)
    bb = BatchBuilder(minlen=5, support=support, unphased=unphased)
    ids = [bb.add_read(r.pos, encode_cigar(r.cigar), mapq=mq, phase=ph, reverse=bool(r.flag & 0x10), is_2d=twod) for r, mq, ph, twod in pool]
    order = sorted(range(len(ids)), key=lambda k: (bb._reads[ids[k]][2], k))
    for j in range(n_loci):
        d = depth + j % 4
        off = (37 * j) % (len(pool) - d + 1)
        sh = j % 25 - 12
        bb.add_locus(start + sh, end + sh, [ids[i] for i in order[off : off + d]])
    return bb.build()


# ---- rows for the 1-D DBSCAN of `inquiSTR outlier` (csrc/outlier.hip outlier_dbscan_kernel) ----------------------------------
# The kernel has a size class per row width (up to 256, up to 2 048, up to 8 192 values).  What decides a value is whether
# |x - y| < eps holds (strictly) and whether a point has at least `mincluster` neighbours, itself included: the rows put groups of
# equal values exactly on both sides of both.

DBSCAN_WRAP_ROW = (float("inf"), float("inf"), float("inf"), 12.0, 2.5e19)  # mode usize::MAX: 2 * mode wraps (src/outlier.rs:115)
DBSCAN_PAD = 777.0  # behind a row's length: never read by the reference, and a kernel that reads it gets a value that matters


def _dbscan_struct(rng: random.Random, n: int, mincluster: int, base: int, near: bool = False) -> List[float]:
    """A dense cluster around `base` (its mode: eps = max(2 * base, 10)) whose largest value, top = base + 2, exactly two points
    hold, nothing else above top - 1.  Where `mincluster` leaves room: replicas of [a body of mincluster + 2 points at F - 2, two
    points at F, a satellite group of s equal values at F + off] far from one another (F steps by 10 eps + 1000), off in
    {eps - 1, eps, eps + 1}, s in {mincluster - 3 .. mincluster + 1}.  At off = eps - 1 the satellites' neighbours are themselves
    and the two points at F: core from s = mincluster - 2, an edge point below; from off = eps on they are on their own: core from
    s = mincluster, noise below.  Then a lone far value.  Where mincluster is near the row's length: the dense cluster and one
    satellite group of 1 - 3 values at top + off (`near`: off = eps - 1 - at the full width the two points at top then reach
    everything and are the only core points, every other value is an edge point; one value fewer and all are noise)."""
    eps, top = max(2 * base, 10), base + 2
    if n < 8:
        return [float(base)] * n
    extra: List[float] = []
    if mincluster > n // 3:
        extra = [float(top + (eps - 1 if near else rng.choice([eps - 1, eps, eps + 1])))] * rng.choice([1, 2, 3])
    else:
        sizes = [s for s in (mincluster - 3, mincluster - 2, mincluster - 1, mincluster, mincluster + 1) if s >= 1]
        first = [(s, o) for s, o in ((mincluster - 3, eps - 1), (mincluster - 2, eps - 1), (mincluster - 1, eps), (mincluster, eps)) if s >= 1]
        rest = [(s, o) for s in sizes for o in (eps - 1, eps, eps + 1) if (s, o) not in first]
        rng.shuffle(rest)
        room = n - (2 * mincluster + 10) - 1  # the dense cluster keeps enough points for `base` to stay the mode; one lone value
        F = top + 10 * eps + 1000
        for s, o in first + rest:
            need = mincluster + 2 + 2 + s
            if need > room:
                break
            extra += [float(F - 2)] * (mincluster + 2) + [float(F)] * 2 + [float(F + o)] * s
            room -= need
            F += 10 * eps + 1000
        extra.append(float(F + 5000))
    n_dense = n - len(extra)
    n_base = max(1, (n_dense - 2) * 7 // 10)
    dense = [float(top)] * 2 + [float(base)] * n_base
    dense += [base + rng.choice([-1.0, -0.5, 0.5, 1.0]) for _ in range(n_dense - len(dense))]
    row = dense + extra
    assert len(row) == n
    rng.shuffle(row)
    return row


def dbscan_wrap_row(stride: int, mincluster: int) -> List[float]:
    """A row whose flags depend on `2 * mode` wrapping (src/outlier.rs:115), scaled to `mincluster` >= 3: a values of 12 and b of
    2.5e19 with a < b < mincluster = a + b, and up to three infinities.  2.5e19 and inf both cast to usize::MAX, the mode.  Wrapped,
    eps is 2^64 - 2 = 1.8e19: the two groups do not reach each other, neither is a cluster, every value is noise.  Unwrapped (or
    saturated) eps would be 3.7e19 (1.8e19 and a bit): the a + b finite values would all be neighbours and core points, and only
    the infinities noise.  Below mincluster 3 no such row exists (DBSCAN_WRAP_ROW instead, which decides it at mincluster 2)."""
    if mincluster < 3:
        return list(DBSCAN_WRAP_ROW)
    a = (mincluster - 1) // 2
    b = mincluster - a
    assert 1 <= a < b < mincluster <= stride
    return [float("inf")] * min(3, stride - mincluster) + [12.0] * a + [2.5e19] * b


def dbscan_rows(rng: random.Random, stride: int, n_rows: int, mincluster: int, first_kind: int = 0):
    """Rows for inq_outlier_rows(method = dbscan) at width `stride`: (values f32 [n_rows, stride], lengths u32 [n_rows]).  Twelve kinds
    in turn from `first_kind` on: _dbscan_struct at the full width and one value past a power of two, dbscan_wrap_row, a row
    without a positive value (no mode), _dbscan_struct with NaN / +-inf / negative values thrown in at one value short of a power
    of two, positive values all inside (0, 1) (the mode's key is 0); then one repeated value at the full width (the sort's all-ties
    path), lengths 0 and 1, negative values only, and further _dbscan_struct rows of random length and of the full width with NaN
    and the like.  Behind a row's length lies DBSCAN_PAD."""
    pow2 = 1 << ((stride - 1).bit_length() - 1)  # the largest power of two below the width
    vals = np.full((n_rows, stride), DBSCAN_PAD, dtype=np.float32)
    lens = np.zeros(n_rows, dtype=np.uint32)
    inf = float("inf")
    for i in range(n_rows):
        kind = (i + first_kind) % 12
        base = (5, 12, 30, 200)[(i // 2 + i) % 4]
        if kind == 0:
            row = _dbscan_struct(rng, stride, mincluster, base, near=True)
        elif kind == 1:
            row = _dbscan_struct(rng, pow2 + 1, mincluster, base)
        elif kind == 2:
            row = dbscan_wrap_row(stride, mincluster)
        elif kind == 3:
            row = [rng.choice([0.0, -0.0, float("nan"), -1.0, -40.0]) for _ in range(pow2 - 1)] + [0.0]
        elif kind == 4 or kind == 11:
            row = _dbscan_struct(rng, pow2 - 1 if kind == 4 else stride, mincluster, base)
            for _ in range(max(3, len(row) // 30)):
                row[rng.randrange(len(row))] = rng.choice([float("nan"), inf, -inf, -3.0, -1e9, 0.0])
        elif kind == 5:
            row = [rng.choice([0.0, -2.0]) if rng.random() < 0.2 else rng.uniform(0.01, 0.99) for _ in range(stride)]
        elif kind == 6:
            row = [7.0] * stride
        elif kind == 7:
            row = []
        elif kind == 8:
            row = [12.0]
        elif kind == 9:
            row = [rng.choice([-5.0, -6.0, -inf]) for _ in range(pow2 // 2 + 3)]
        else:
            row = _dbscan_struct(rng, rng.randint(1, stride), mincluster, base)
        vals[i, : len(row)] = row
        lens[i] = len(row)
    return vals, lens


DBSCAN_CLASSES = ((256, 48), (257, 48), (2048, 12), (2049, 12), (8192, 6))  # (width, rows): both sides of every size class' edge


def dbscan_minclusters(stride: int):
    """1 (every finite value is a core point), usize::ilog2 of the width (what `inquiSTR outlier` passes), the width itself."""
    return (1, stride.bit_length() - 1, stride)


def dbscan_edge_points(values: np.ndarray, n: int, mincluster: int, flags: np.ndarray) -> int:
    """How many values of the row are neither flagged as noise nor core points - neighbours of a core point without `mincluster`
    neighbours of their own -, counted from the definition; 0 for a row with a value that is not a small finite number."""
    v = np.where(np.isnan(values[:n]), 0.0, values[:n]).astype(np.float64)
    if n == 0 or not np.isfinite(v).all() or np.abs(v).max() >= 2.0**23 or not (v > 0).any():
        return 0
    keys, counts = np.unique(np.floor(v[v > 0]), return_counts=True)
    eps = max(2.0 * float(keys[np.argmax(counts)]), 10.0)  # (argmax: the first, so the smallest, of equally frequent keys)
    s = np.sort(v)
    neighbours = np.searchsorted(s, v + eps, "left") - np.searchsorted(s, v - eps, "right")  # exact: small numbers, |x - y| < eps
    return int(((neighbours < mincluster) & (flags[:n] == 0)).sum())


def dbscan_flags_by_definition(values: np.ndarray, n: int, mincluster: int, wrap: bool) -> np.ndarray:
    """The noise flags of one row from the definition (src/outlier.rs:112-145, dbscan 0.3.1: neighbours at f64 distance < eps, a
    core point has at least `mincluster` of them, noise is neither a core point nor the neighbour of one), with `2 * mode` wrapped
    modulo 2^64 as the release build does or, `wrap` = False, not: what a kernel that widened or saturated it would give."""
    v = np.where(np.isnan(values[:n]), 0.0, values[:n]).astype(np.float64)
    counts = {}
    for x in v[v > 0].tolist():
        k = 2**64 - 1 if x >= 2.0**64 else int(x)
        counts[k] = counts.get(k, 0) + 1
    best = max(counts.values())
    twice = 2 * min(k for k, c in counts.items() if c == best)
    eps = float(max(twice % 2**64 if wrap else twice, 10))
    core = np.zeros(n, dtype=bool)
    near_core = np.zeros(n, dtype=bool)
    with np.errstate(invalid="ignore"):  # inf - inf: NaN, no neighbour
        for lo in range(0, n, 512):
            core[lo : lo + 512] = (np.abs(v[lo : lo + 512, None] - v[None, :]) < eps).sum(axis=1) >= mincluster
        for lo in range(0, n, 512):
            near_core[lo : lo + 512] = ((np.abs(v[lo : lo + 512, None] - v[None, :]) < eps) & core[None, :]).any(axis=1)
    return (~core & ~near_core).astype(np.uint8)


def rows_decided_by_the_wrap(vals, lens, mincluster, flags, keep) -> int:
    """How many kept rows of the reference's answer hold a flag that an unwrapped `2 * mode` would change (only a row with a value
    of 2^63 or more can); asserts on the way that the wrapped definition is the reference's answer for those rows."""
    n_rows = 0
    for i in np.nonzero(keep == 1)[0]:
        n = int(lens[i])
        if not (np.nan_to_num(vals[i, :n], nan=0.0) >= 2.0**63).any():
            continue
        assert np.array_equal(dbscan_flags_by_definition(vals[i], n, mincluster, True), flags[i, :n]), (i, mincluster)
        n_rows += int(not np.array_equal(dbscan_flags_by_definition(vals[i], n, mincluster, False), flags[i, :n]))
    return n_rows


def assert_dbscan_class_is_covered(stride: int, per_mincluster) -> None:
    """per_mincluster: [(values, lengths, mincluster, reference flags, reference keep)] of one width.  From the reference alone: the
    class has at least four kept rows, a flagged value, an unflagged value that is no core point, a row without a mode, and a row
    whose flags differ from what an unwrapped `2 * mode` gives - under every mincluster from 3 on, in fact."""
    kept = flagged = edge = no_mode = 0
    for vals, lens, mincluster, flags, keep in per_mincluster:
        kept = max(kept, int((keep == 1).sum()))
        flagged += int(flags.sum())
        no_mode += int((keep == 3).sum())
        edge += sum(dbscan_edge_points(vals[i], int(lens[i]), mincluster, flags[i]) for i in np.nonzero(keep == 1)[0])
        if mincluster >= 3:
            assert rows_decided_by_the_wrap(vals, lens, mincluster, flags, keep) >= 1, (stride, mincluster)
    assert kept >= 4 and flagged >= 1 and edge >= 1 and no_mode >= 1, (stride, kept, flagged, edge, no_mode)


_DBSCAN_REF = {}


def dbscan_class_reference(stride: int, n_rows: int):
    """dbscan_rows at one width under each of dbscan_minclusters, with the C restatement's flags and row states (minsize 0: a row
    without a positive value is kept and has no mode): [(values, lengths, mincluster, flags, keep)].  Under mincluster 1, where
    every finite value is a core point whatever the row, the kinds start with the seventh: the narrow matrix of the widest class
    holds the repeated value and the lengths 0 and 1 too.  Computed once per process."""
    from oracle import outlier_oracle as oo

    if stride not in _DBSCAN_REF:
        per = []
        for mincluster in dbscan_minclusters(stride):
            vals, lens = dbscan_rows(random.Random(31 * stride + mincluster), stride, n_rows, mincluster, first_kind=6 if mincluster == 1 else 0)
            flags, keep = oo.c_outlier_rows(vals, lens, "dbscan", minsize=0, mincluster=mincluster, threads=8)
            per.append((vals, lens, mincluster, flags, keep))
        _DBSCAN_REF[stride] = per
    return _DBSCAN_REF[stride]
