"""The window-bounded CIGAR walk: every batch is called with the producer promise (INQ_READ_CHECKED) set where
the domain rules hold and with it cleared, and both must equal the CPU oracle bit for bit - rows, pair_call,
pair_bits, ties and status.  Needs an MI355X.
"""
import random

import numpy as np
import pytest

from inquistr_amd import batch as B
from inquistr_amd.window_bytes import mark_checked
from tests import gen
from tests.walkutil import _all_variants, _assert_same, open_ctx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    yield from open_ctx()


def _both(ctx, orc, batch, what=""):
    """Calls the batch with the promise set (where it holds) and cleared; returns the status code."""
    codes = []
    for promise in (True, False):
        if promise:
            mark_checked(batch)
        else:
            batch.reads["promise"] = 0
        oc, want = orc.call_batch(batch, debug=True)
        rc, got = ctx.call_batch(batch, debug=True, check=False)
        assert rc == oc, (what, promise, rc, oc)
        if rc == B.INQ_OK:
            _assert_same(got, want, f"{what} promise={promise}")
        codes.append(rc)
    assert codes[0] == codes[1]
    return codes[0]


@pytest.mark.parametrize("seed", range(256))
@pytest.mark.parametrize("unphased", [False, True])
def test_row_walk_cases(ctx, orc, seed, unphased):
    """gen.row_walk_case: batches whose dimensions are walk_pairs_rows' own - pairs per locus on both sides of every tier of
    the locus kernels (1 ... 64, 65 ... 300, 2 048 / 2 049), ops per read around the 64-op piece and the 16-groups-left test,
    the piece (0, 1, 2, 5, 9) in which a promised read passes end_ext with pos + consumed on end_ext - 2 ... + 1 at the piece
    boundary, windows of 0 ... 40 000 bp under reads of short ops (the lane queue drains many times, fed by 16 row streams),
    runs of 1 ... 64 reads that claim() settles without a load and whole blocks of them, reads shared between loci with
    different windows - each under the five promise variants, bit for bit against the oracle."""
    batch, info = gen.row_walk_case(seed, unphased)
    assert gen.checked_share(batch) == 1.0
    assert _all_variants(ctx, orc, batch, f"row walk case {seed} unphased={unphased} {info['depths']}") == B.INQ_OK


@pytest.mark.parametrize("seed,unphased,long_every", [(1, False, 0), (2, True, 0), (3, False, 5), (4, True, 7)])
def test_random_cases(ctx, orc, seed, unphased, long_every):
    batch, _ = gen.random_case(7000 + seed, n_loci=60, unphased=unphased, long_every=long_every)
    assert (mark_checked(batch).reads["promise"] != 0).all()
    assert _both(ctx, orc, batch, f"seed {seed}") == B.INQ_OK


@pytest.mark.parametrize("seed,unphased,max_reads", [(11, False, 150), (12, True, 300), (13, True, 100)])
def test_deeper_loci(ctx, orc, seed, unphased, max_reads):
    """Loci of 65 - 300 offered reads go through locus_call_mid_walk (four 64-read blocks per wave, or the work list)."""
    batch, _ = gen.random_case(seed, n_loci=8, unphased=unphased, max_reads=max_reads, long_every=9)
    assert _both(ctx, orc, batch, f"seed {seed}") == B.INQ_OK


def _edge_batch(unphased, seed=0):
    """One window (start 1010, end 1090: start_ext 1000, end_ext 1100) and reads whose walk ends on every edge of the
    stop rule: pos + consumed == end_ext - 1 / == end_ext / == end_ext + 1 exactly at a 64-op piece boundary, a D op
    across end_ext, reads starting before / at / after end_ext, pos = -1, unmapped reads, reads without a
    reference span, I / S ops on the window's edges."""
    rng = random.Random(seed)
    bb = B.BatchBuilder(minlen=2, support=1, unphased=unphased)
    ee = 1100
    idx = []

    def add(pos, cig, **kw):
        idx.append(bb.add_read(pos, B.encode_cigar(cig), phase=kw.pop("phase", 1 + len(idx) % 2), **kw))

    for piece in (1, 2, 3):
        for d in (-2, -1, 0, 1):
            # 64 * piece one-base M ops end at pos + 64 * piece = end_ext + d, then 100 more ops
            pos = ee + d - 64 * piece
            tail = [("I", 7), ("M", 1), ("D", 9), ("M", 1)] * 25
            add(pos, [("M", 1)] * (64 * piece - 1) + [("M", 1)] + tail)
            add(pos, [("M", 1)] * (64 * piece - 2) + [("I", 6), ("M", 1)] + tail)
    add(1050, [("M", 45), ("D", 30), ("M", 20), ("I", 8), ("M", 300)])  # D from 1096 across end_ext
    add(1050, [("M", 49), ("D", 30), ("M", 20)] * 40)  # D starting at 1100 = end_ext: does not count
    add(1050, [("M", 48), ("I", 30), ("M", 20)] * 40)  # I at 1099: counts
    add(1050, [("M", 49), ("I", 30), ("M", 20)] * 40)  # I at 1100: does not
    for pos in (1098, 1099, 1100, 1101, 1200):
        add(pos, [("M", 3), ("I", 20), ("M", 50)] * 30)
    add(-1, [("M", 990), ("I", 12), ("M", 40), ("D", 15), ("M", 900)] + [("M", 2), ("I", 3)] * 200)
    add(-1, [("S", 30), ("M", 1020), ("I", 50), ("M", 80)])
    add(980, [("M", 40), ("I", 25), ("M", 500)] * 10, unmapped=True)
    add(1005, [("I", 40), ("S", 30)])  # rlen == 0 -> 1
    add(1005, [("S", 30), ("I", 40)] * 90)
    add(1090, [])  # empty CIGAR
    add(1000, [("S", 50), ("M", 99), ("I", 33)] + [("M", 1)] * 130, reverse=True)
    for _ in range(30):
        ops = []
        for _ in range(rng.randint(1, 400)):
            op = rng.choice("MMMIDSN=X")
            ops.append((op, rng.randint(1, 6) if op != "N" else rng.randint(1, 30)))
        add(rng.randint(700, 1110), ops, mapq=rng.choice([5, 60, 60]))
    rng.shuffle(idx)
    half = len(idx) // 2
    bb.add_locus(1010, 1090, idx[:half])
    bb.add_locus(1010, 1090, idx[half:])
    bb.add_locus(1010, 1090, idx)  # > 64 reads: the medium path
    bb.add_locus(1010, 1090, idx[:64])
    bb.add_locus(1095, 1096, idx[:40])
    return bb.build()


@pytest.mark.parametrize("unphased", [False, True])
def test_stop_rule_edges(ctx, orc, unphased):
    for seed in range(3):
        assert _both(ctx, orc, _edge_batch(unphased, seed), f"edges seed {seed}") == B.INQ_OK


@pytest.mark.parametrize("unphased", [False, True])
def test_wrapped_window(ctx, orc, unphased):
    """locus_end + 10 past 2^32: the window wraps and every read is walked whole, promise or not.  With end_ext < start_ext
    the reference's `start_ext < pos && pos < end_ext` holds for no position (u32, src/call.rs:387-403), so the I / D / S ops
    that reads starting at -1, 0 and 2 have at reference positions 0 ... end + 9 - 2^32 count for nothing."""
    bb = B.BatchBuilder(minlen=2, support=1, unphased=unphased)
    idx = [bb.add_read(100 + 7 * k, B.encode_cigar([("M", 30), ("I", 9), ("M", 5), ("D", 4)] * 50), phase=1 + k % 2)
           for k in range(20)]
    low = []
    for k, pos in enumerate((-1, 0, 2) * 4):
        head = [[("I", 9), ("M", 1), ("D", 4), ("S", 7), ("M", 1), ("I", 3)], [("S", 12), ("M", 2), ("I", 5), ("M", 1), ("D", 3)],
                [("M", 1), ("D", 3), ("I", 8), ("M", 2), ("S", 6)], [("D", 5), ("I", 6), ("M", 3), ("I", 4)]][k // 3]
        low.append(bb.add_read(pos, B.encode_cigar(head + [("M", 30), ("I", 9), ("M", 5), ("D", 4)] * (3 + 20 * (k % 2))),
                               phase=1 + k % 2, is_2d=(k == 7)))
    bb.add_locus(2**32 - 40, 2**32 - 5, idx + low)
    bb.add_locus(2**32 - 40, 2**32 - 11, idx + low)
    bb.add_locus(1010, 1090, idx + low)
    bb.add_locus(2**32 - 40, 2**32 - 1, low)  # end_ext = 9: reference positions 0 ... 8 lie "inside" the wrapped difference
    bb.add_locus(2**32 - 300, 2**32 - 10, low + idx)  # end_ext = 0
    bb.add_locus(2**32 - 40, 2**32 - 3, (idx + low) * 3)  # 96 pairs: wave_locus<4>
    bb.add_locus(2**32 - 25, 2**32 - 1, (low + idx) * 10)  # 320 pairs: walk_locus
    batch = bb.build()
    assert _both(ctx, orc, batch, "wrapped") == B.INQ_OK
    assert gen.checked_share(batch) == 1.0
    assert _all_variants(ctx, orc, batch, "wrapped") == B.INQ_OK
    # what the oracle says of the wrapped loci: no Call, no clip bit, though the same reads have Calls in the ordinary window
    code, want = orc.call_batch(batch, debug=True)
    off = batch.locus_pair_off.astype(np.int64)
    wrapped = np.ones(batch.n_pairs, dtype=bool)
    wrapped[off[1] : off[3]] = False  # (the second locus ends at 2^32 - 1: far from every read, but not wrapped)
    assert code == B.INQ_OK and not want.pair_call[wrapped].any() and not (want.pair_bits[wrapped] & B.INQ_PAIR_CLIP).any()
    assert (want.pair_call[off[2] : off[3]] != 0).sum() >= 20


@pytest.mark.parametrize("unphased", [False, True])
def test_bad_op_in_the_tail_of_an_unpromised_read(ctx, orc, unphased):
    """A bad op far behind the window is still found in a read without the promise, next to promised reads."""
    bb = B.BatchBuilder(minlen=2, support=1, unphased=unphased)
    idx = [bb.add_read(950, B.encode_cigar([("M", 20), ("I", 9)] * 40), phase=1 + k % 2) for k in range(10)]
    words = B.encode_cigar([("M", 20), ("I", 9)] * 150)
    words[-1] = (9 << 4) | 9  # op code 9 at op 299, far past end_ext
    idx.insert(4, bb.add_read(950, words, phase=1))
    bb.add_locus(1010, 1090, idx)
    batch = bb.build()
    assert _both(ctx, orc, batch, "bad op") == B.INQ_ERR_CIGAR_OP
    # a read whose positions pass 2^31 - 1 in piece 3, behind the piece (2) after which a promised read would stop
    bb = B.BatchBuilder(minlen=2, support=1, unphased=unphased)
    idx = [bb.add_read(2**31 - 5000, B.encode_cigar([("M", 20), ("I", 9)] * 40), phase=1) for _ in range(6)]
    idx.append(bb.add_read(2**31 - 5000, B.encode_cigar([("M", 1)] * 150 + [("M", 100)] * 60), phase=1))
    bb.add_locus(2**31 - 4900, 2**31 - 4850, idx)
    assert _both(ctx, orc, bb.build(), "range") == B.INQ_ERR_RANGE


def test_synthetic_workload_promised_and_cleared(ctx, orc):
    from inquistr_amd import synth

    for name in ("unphased100k", "phased10k", "expansion50k", "longreads20k"):
        batch = synth.generate_numpy(synth.WORKLOADS[name], 0, 200)
        assert (batch.reads["promise"] == B.INQ_READ_CHECKED).all()
        assert _both(ctx, orc, batch, name) == B.INQ_OK


def test_device_front_end_batches_carry_the_promise(ctx, tmp_path):
    from inquistr_amd import call
    from inquistr_amd.window_bytes import checked_mask
    from tests.test_host_frontend import _make_case

    bam, bed, loci, recs = _make_case(tmp_path, 31)
    sp = call.Spans(bam, region_file=bed, minlen=5, support=3, threads=2, unphased=True, max_comp_bytes=0)
    n = 0
    for span in sp.spans():
        rc, p1, p2, ties, stats = ctx.call_span(span["comp"], span["blocks"], span["anchors"], span["anchor_stop"],
                                                span["locus_tid"], span["locus_start"], span["locus_end"], 5, 3, True)
        assert rc == 0
        cigar, reads, pair_read, off = ctx.span_fetch_batch(stats, len(span["locus_index"]))
        b = B.Batch(cigar=cigar, reads=reads, pair_read=pair_read, locus_pair_off=off,
                    locus_start=np.zeros(len(off) - 1, np.uint32), locus_end=np.zeros(len(off) - 1, np.uint32))
        want = np.where(checked_mask(b), B.INQ_READ_CHECKED, 0)
        assert np.array_equal(reads["promise"], want)
        n += int(reads.shape[0])
    sp.close()
    assert n > 0


@pytest.mark.parametrize("n_ops", [(1 << 25) - 4, (1 << 25) - 3])
def test_longest_read_of_the_row_walk(ctx, orc, n_ops):
    """2^25 - 4 ops (2^23 - 1 groups) is the longest read the row walk takes; one op more sends the block to the whole
    walk.  Both must give the oracle's rows, with the read's end far behind the window."""
    bb = B.BatchBuilder(minlen=2, support=1, unphased=True)
    words = np.full(n_ops, (1 << 4) | 0, dtype=np.uint32)  # 1M each
    words[30] = (12 << 4) | 1  # an I inside the window
    idx = [bb.add_read(1000, words, phase=1)]
    idx += [bb.add_read(990 + k, B.encode_cigar([("M", 40), ("I", 5 + k), ("M", 200)]), phase=1) for k in range(5)]
    bb.add_locus(1010, 1090, idx)
    bb.add_locus(1012, 1080, idx[::-1])
    assert _both(ctx, orc, bb.build(), f"{n_ops} ops") == B.INQ_OK


@pytest.mark.parametrize("kind,code", [("op", B.INQ_ERR_CIGAR_OP), ("range", B.INQ_ERR_RANGE)])
def test_device_front_end_clears_the_promise_of_a_bad_read(ctx, tmp_path, kind, code):
    """The device front end leaves the byte clear on a read with a bad op or a span past 2^31 behind the window, and
    the call still fails with the matching error."""
    from inquistr_amd import call
    from tests.test_window_bytes import bam_with_one_bad_read

    bam, n_bad = bam_with_one_bad_read(tmp_path, kind)
    sp = call.Spans(bam, region="chr1:5000-5050", minlen=5, support=3, threads=1, unphased=True, max_comp_bytes=0)
    (span,) = list(sp.spans())
    rc, p1, p2, ties, stats = ctx.call_span(span["comp"], span["blocks"], span["anchors"], span["anchor_stop"],
                                            span["locus_tid"], span["locus_start"], span["locus_end"], 5, 3, True, check=False)
    assert rc == code
    cigar, reads, pair_read, off = ctx.span_fetch_batch(stats, len(span["locus_index"]))
    is_bad = reads["n_cigar"] == n_bad
    assert is_bad.sum() == 1 and reads.shape[0] == 9
    assert (reads["promise"][is_bad] == 0).all()
    assert (reads["promise"][~is_bad] == B.INQ_READ_CHECKED).all()
    sp.close()
