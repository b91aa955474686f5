"""The producer promise (inq_read_t.promise) on the CPU side: who sets it, and the byte count of the window-bounded
walk (inquistr_amd/window_bytes.py) against a direct count."""
import numpy as np
import pytest

from inquistr_amd import batch as B
from inquistr_amd import synth
from inquistr_amd.window_bytes import checked_mask, mark_checked, window_bounded_bytes, window_bounded_cigar_bytes
from tests import gen


@pytest.mark.parametrize("name", ["unphased100k", "phased10k", "expansion50k", "longreads20k"])
def test_synth_sets_the_promise_on_every_read(name):
    wl = synth.WORKLOADS[name]
    b = synth.generate_numpy(wl, 30, 60)
    assert (b.reads["promise"] == B.INQ_READ_CHECKED).all()
    assert checked_mask(b).all()
    d = synth.DeviceBatch(wl, "cpu", 30, 60)
    assert np.array_equal(d.reads.numpy().reshape(-1).view(B.READ_DTYPE)["promise"], b.reads["promise"])


def test_builder_leaves_the_byte_clear():
    batch, _ = gen.random_case(3, n_loci=10)
    assert (batch.reads["promise"] == 0).all()
    assert (mark_checked(batch).reads["promise"] == B.INQ_READ_CHECKED).all()


def test_checked_mask_rules():
    bb = B.BatchBuilder()
    ok = bb.add_read(100, B.encode_cigar([("M", 50), ("I", 5), ("D", 3)]), phase=1)
    bad = bb.add_read(100, np.array([(50 << 4) | 0, (5 << 4) | 9], dtype=np.uint32), phase=1)
    edge = bb.add_read(2**31 - 52, B.encode_cigar([("M", 50)]), phase=1)  # pos + 1 + 50 = 2^31 - 1
    over = bb.add_read(2**31 - 51, B.encode_cigar([("M", 50)]), phase=1)  # = 2^31
    neg = bb.add_read(-1, B.encode_cigar([("M", 50)]), phase=1)
    neg2 = bb.add_read(-2, B.encode_cigar([("M", 50)]), phase=1)
    bb.add_locus(1010, 1090, [ok, bad, edge, over, neg, neg2])
    assert list(checked_mask(bb.build())) == [True, False, True, False, True, False]


def _direct_cigar_bytes(batch, piece_ops):
    """Pair by pair, op by op."""
    total = 0
    consumes = {0, 2, 3, 7, 8}
    for j in range(batch.n_loci):
        ee = (int(batch.locus_end[j]) + 10) & 0xFFFFFFFF
        se1 = (int(batch.locus_start[j]) - 9) & 0xFFFFFFFF
        for p in range(int(batch.locus_pair_off[j]), int(batch.locus_pair_off[j + 1])):
            r = batch.reads[int(batch.pair_read[p])]
            o, n = int(r["cigar_off4"]) * 4, int(r["n_cigar"])
            n4 = (n + 3) // 4
            if not (r["promise"] & B.INQ_READ_CHECKED) or ee < se1:
                total += 16 * n4
                continue
            carry = (int(r["pos"]) + 1) & 0xFFFFFFFF
            if carry > ee:
                continue
            groups = n4
            for i in range(n):
                w = int(batch.cigar[o + i])
                if (w & 15) in consumes:
                    carry += w >> 4
                if carry > ee:
                    groups = min(n4, (i // piece_ops + 1) * (piece_ops // 4))
                    break
            total += 16 * groups
    return total


@pytest.mark.parametrize("piece_ops", [64, 32])
def test_window_bytes_match_a_direct_count(piece_ops):
    for seed in range(4):
        batch, _ = gen.random_case(100 + seed, n_loci=25, unphased=bool(seed & 1), long_every=5 if seed == 2 else 0)
        mark_checked(batch)
        if seed == 3:
            batch.reads["promise"][::3] = 0
        assert window_bounded_cigar_bytes(batch, piece_ops) == _direct_cigar_bytes(batch, piece_ops)
    b = synth.generate_numpy(synth.WORKLOADS["unphased100k"], 0, 40)
    got = window_bounded_bytes(b, piece_ops)
    assert got == _direct_cigar_bytes(b, piece_ops) + 20 * b.n_pairs + 32 * b.n_loci
    assert got < 0.6 * b.algorithmic_bytes()
    b.reads["promise"] = 0  # whole reads, in whole 16-byte groups
    assert window_bounded_bytes(b, piece_ops) == 16 * int(((b.cigar_ops_per_pair() + 3) // 4).sum()) + 20 * b.n_pairs + 32 * b.n_loci


def test_host_front_end_sets_the_promise_exactly(tmp_path):
    """The host sweep sets the byte exactly where the domain rules hold (every read of a valid BAM)."""
    from inquistr_amd import call
    from tests.test_host_frontend import _make_case

    bam, bed, loci, recs = _make_case(tmp_path, 5)
    fe = call.FrontEnd(bam, region_file=bed, minlen=5, support=3, threads=2, unphased=True)
    n = 0
    for batch, _ in fe.batches():
        assert (batch.reads["promise"] == np.where(checked_mask(batch), B.INQ_READ_CHECKED, 0)).all()
        assert (batch.reads["promise"] == B.INQ_READ_CHECKED).all()
        n += batch.n_reads
    assert n > 0


def bam_with_one_bad_read(tmp_path, kind):
    """chr1 with eight valid reads around 5000-5050 and one read that breaks a domain rule behind the window:
    kind "op" = op code 9 as its last op, kind "range" = pos + 1 + span past 2^31 (16 N ops of 2^27 at its end).
    Returns (bam path, n_cigar of the bad read)."""
    import struct

    from oracle import pyoracle as py
    from tools import bamio

    bam = str(tmp_path / f"bad_{kind}.bam")
    w = bamio.BamWriter(bam, [("chr1", 100000)])
    ok = [py.Record(pos=4800 + 20 * k, cigar=[("M", 210), ("I", 12), ("M", 300)], hp=("C", 1 + k % 2)) for k in range(8)]
    bad_pos = 4900
    if kind == "op":
        cigar = [("M", 1)] * 200 + [("I", 5)] * 100
    else:
        cigar = [("M", 1)] * 200 + [("N", 1 << 27)] * 16
    recs = [(r.pos, r) for r in ok] + [(bad_pos, None)]
    for i, (pos, r) in enumerate(sorted(recs, key=lambda x: x[0])):
        if r is not None:
            w.add(f"r{i}", r.flag, 0, r.pos, r.mapq, r.cigar, [("HP", r.hp[0], r.hp[1])])
            continue
        body = bytearray(bamio.encode_record(f"r{i}", 0, 0, bad_pos, 60, cigar, [("HP", "C", 1)]))
        if kind == "op":
            at = 32 + len(f"r{i}") + 1 + 4 * (len(cigar) - 1)
            word = struct.unpack_from("<I", body, at)[0]
            struct.pack_into("<I", body, at, (word & ~0xF) | 9)
        w.add_raw(struct.pack("<I", len(body)) + bytes(body), 0, bad_pos, bad_pos + bamio.ref_span(cigar))
    w.close()
    return bam, len(cigar)


@pytest.mark.parametrize("kind,code", [("op", B.INQ_ERR_CIGAR_OP), ("range", B.INQ_ERR_RANGE)])
def test_host_front_end_clears_the_promise_of_a_bad_read(tmp_path, orc, kind, code):
    """A bad op or a span past 2^31 behind the window: the host sweep leaves the byte clear on that read only, and the
    batch still fails with the error the reference's panic maps to."""
    from inquistr_amd import call

    bam, n_bad = bam_with_one_bad_read(tmp_path, kind)
    fe = call.FrontEnd(bam, region="chr1:5000-5050", minlen=5, support=3, threads=1, unphased=True)
    (batch, _), = list(fe.batches())
    is_bad = batch.reads["n_cigar"] == n_bad
    assert is_bad.sum() == 1 and batch.n_reads == 9
    assert (batch.reads["promise"][is_bad] == 0).all()
    assert (batch.reads["promise"][~is_bad] == B.INQ_READ_CHECKED).all()
    assert (batch.reads["promise"] == np.where(checked_mask(batch), B.INQ_READ_CHECKED, 0)).all()
    assert orc.call_batch(batch)[0] == code


def test_line_bytes_match_a_direct_count():
    from inquistr_amd.window_bytes import _walked_groups, window_bounded_line_bytes

    b = synth.generate_numpy(synth.WORKLOADS["unphased100k"], 0, 20)
    g0, groups = _walked_groups(b, 64)
    lines = sum(len({(16 * (int(s) + k)) // 128 for k in range(int(n))}) for s, n in zip(g0, groups))
    assert window_bounded_line_bytes(b) == 128 * lines
    assert window_bounded_cigar_bytes(b) <= window_bounded_line_bytes(b)


# ---- promise variants (tests/gen.py set_promise) and the premise of the window-bounded walk -------------------------


def _variant_batches():
    from tests.test_gpu_window_walk import _edge_batch

    yield "random_case", gen.random_case(41, n_loci=30, long_every=5)[0]
    yield "random_case_deep", gen.random_case(42, n_loci=8, unphased=True, max_reads=300, long_every=9)[0]
    yield "edge_batch", _edge_batch(True, 1)
    yield "row_walk_case", gen.row_walk_case(4, max_depth=300)[0]


def test_promise_variants_mean_what_they_say():
    """none / all are the two extremes, half and lone_* leave blocks that hold both kinds, lone_* hold their per-block rule,
    no variant promises a read `checked_mask` rejects, and the same seed gives the same bytes."""
    from inquistr_amd.window_bytes import _walked_groups

    for name, batch in _variant_batches():
        ok = checked_mask(batch)
        assert ok.all(), name
        block, first, size = gen._blocks(batch)
        assert int(size.sum()) == batch.n_pairs and size.min() >= 1 and size.max() <= 64
        seen = {}
        for what in gen.promise_variants(batch, seed=3):
            p = batch.reads["promise"].copy()
            assert set(np.unique(p)) <= {0, B.INQ_READ_CHECKED}
            seen[what] = p
            per_pair = p[batch.pair_read] != 0
            n_prom = np.bincount(block, weights=per_pair, minlength=first.shape[0])
            if what == "promise=none":
                assert not p.any()
            elif what == "promise=all":
                assert p.all()
            else:
                assert ((n_prom > 0) & (n_prom < size)).any(), f"{name} {what}: no block holds both kinds"
            if what == "promise=lone_promise":
                assert (n_prom >= 1).all() and n_prom.sum() < 0.5 * batch.n_pairs
            if what == "promise=lone_unpromised":
                assert (n_prom <= size - 1).all() and n_prom.sum() > 0.5 * batch.n_pairs
            assert gen.set_promise(batch, what.split("=")[1], seed=3) == what and np.array_equal(batch.reads["promise"], p)
        assert len({p.tobytes() for p in seen.values()}) == 5, name
        # the variants are different work for the row walk: fewer promises, more groups walked
        loads = {}
        for what in gen.promise_variants(batch, seed=3):
            loads[what] = int(_walked_groups(batch, 64)[1].sum())
        assert loads["promise=all"] < loads["promise=half"] < loads["promise=none"], (name, loads)
        assert loads["promise=all"] < loads["promise=lone_unpromised"] <= loads["promise=half"], (name, loads)
        assert loads["promise=half"] <= loads["promise=lone_promise"] < loads["promise=none"], (name, loads)


def test_promise_variants_never_promise_a_bad_read():
    bb = B.BatchBuilder()
    good = [bb.add_read(100, B.encode_cigar([("M", 50), ("I", 5), ("D", 3)]), phase=1) for _ in range(70)]
    bad_op = bb.add_read(100, np.array([(50 << 4) | 0, (5 << 4) | 9], dtype=np.uint32), phase=1)
    bad_range = bb.add_read(2**31 - 51, B.encode_cigar([("M", 50)]), phase=1)
    bb.add_locus(1010, 1090, good[:30] + [bad_op] + good[30:] + [bad_range])
    bb.add_locus(1010, 1090, [bad_op])  # a block without a promisable read
    batch = bb.build()
    assert gen.checked_share(batch) == 70 / 72
    for what in gen.promise_variants(batch):
        assert batch.reads["promise"][bad_op] == 0 and batch.reads["promise"][bad_range] == 0, what
    gen.set_promise(batch, "lone_promise")
    assert 1 <= int(batch.reads["promise"].sum()) <= 2  # one per 64-pair block of the first locus
    gen.set_promise(batch, "lone_unpromised")
    assert 68 <= int(batch.reads["promise"].sum()) <= 69
    # an empty batch and a batch of one-read loci have no block to mix: every variant still applies
    assert [what for what in gen.promise_variants(B.BatchBuilder().build())] == [f"promise={v}" for v in gen.PROMISE_VARIANTS]
    bb = B.BatchBuilder()
    bb.add_locus(1010, 1090, [bb.add_read(900, B.encode_cigar([("M", 300)]), phase=1)])
    one = bb.build()
    assert [what for what in gen.promise_variants(one)] == [f"promise={v}" for v in gen.PROMISE_VARIANTS]


def _same_result(a, b):
    return (gen.same_f64(a.phase1, b.phase1) and gen.same_f64(a.phase2, b.phase2) and np.array_equal(a.pair_call, b.pair_call)
            and np.array_equal(a.pair_bits, b.pair_bits) and a.n_tie_loci == b.n_tie_loci)


def test_oracle_ignores_the_promise_byte(orc):
    """Rows, pair_call, pair_bits, ties and status of the oracle are those of the byte-clear batch under every variant: GPU
    tests may compute the oracle once per batch and compare every variant with it."""
    for name, batch in _variant_batches():
        gen.set_promise(batch, "none")
        code0, want = orc.call_batch(batch, debug=True)
        assert code0 == B.INQ_OK
        for what in gen.promise_variants(batch):
            code, got = orc.call_batch(batch, debug=True)
            assert code == code0 and _same_result(got, want), f"{name} {what}"
    # ... and the status of a batch that fails
    bb = B.BatchBuilder()
    words = B.encode_cigar([("M", 20), ("I", 9)] * 150)
    words[-1] = (9 << 4) | 9
    bb.add_locus(1010, 1090, [bb.add_read(950, B.encode_cigar([("M", 200)]), phase=1), bb.add_read(950, words, phase=1)])
    batch = bb.build()
    assert [orc.call_batch(batch)[0] for _ in gen.promise_variants(batch)] == [B.INQ_ERR_CIGAR_OP] * 5


@pytest.mark.parametrize("unphased", [False, True])
def test_row_walk_case_generator(orc, unphased):
    """The first seeds of gen.row_walk_case through the C oracle and, where the case keeps per-locus records, through the
    Python oracle; the draws cover what the generator is for."""
    depths, stop_pieces, runs, widths, n_py = set(), set(), set(), set(), 0
    n_kept = n_clip = n_call = 0
    for seed in range(24):
        batch, info = gen.row_walk_case(seed, unphased)
        assert checked_mask(batch).all()
        again, _ = gen.row_walk_case(seed, unphased)
        assert np.array_equal(again.cigar, batch.cigar) and np.array_equal(again.pair_read, batch.pair_read)
        code, want = orc.call_batch(batch, debug=True)
        assert code == B.INQ_OK
        if info["per_locus"] is not None:
            p1, p2, ties = gen.py_expected(batch, info["per_locus"])
            assert gen.same_f64(p1, want.phase1) and gen.same_f64(p2, want.phase2) and ties == want.n_tie_loci, seed
            n_py += 1
        depths |= set(info["depths"])
        stop_pieces |= info["stop_pieces"]
        runs |= set(info["settled_runs"])
        widths.add(info["width"])
        n_kept += int(((want.pair_bits & B.INQ_PAIR_KEPT) != 0).sum())
        n_clip += int(((want.pair_bits & B.INQ_PAIR_CLIP) != 0).sum())
        n_call += int((want.pair_call != 0).sum())
        # reads in another order than their CIGARs, a read offered twice to one locus and to loci with different windows
        assert (np.diff(batch.pair_read.astype(np.int64)) < 0).any()
        off = batch.locus_pair_off.astype(np.int64)
        assert any(len(set(batch.pair_read[off[j] : off[j + 1]])) < off[j + 1] - off[j] for j in range(batch.n_loci))
        assert len(set(zip(batch.locus_start, batch.locus_end))) >= 3
    assert depths >= set(gen.ROW_DEPTHS_SMALL + gen.ROW_DEPTHS_MID + gen.ROW_DEPTHS_DEEP)
    assert stop_pieces >= {0, 1, 2, 5, 9} and widths == set(gen.ROW_WIDTHS)
    assert {1, 2, 3, 4, 5, 8, 16, 33, 64} <= runs
    assert n_py >= 4 and n_kept > 2000 and n_clip > 500 and n_call > 2000


def _truncated_copy(batch):
    """The batch with a private copy of the read per (locus, read) pair, each copy's CIGAR cut to the groups the row walk
    loads for that pair (window_bytes._walked_groups; 0 groups = an empty CIGAR).  Returns (Batch, pairs cut short)."""
    from inquistr_amd.window_bytes import _walked_groups

    g0, groups = _walked_groups(batch, 64)
    r = batch.pair_read.astype(np.int64)
    reads = batch.reads[r].copy()
    n = np.minimum(reads["n_cigar"].astype(np.int64), 4 * groups)
    n4 = (n + 3) // 4
    off4 = np.concatenate([[0], np.cumsum(n4)])
    cig = np.zeros(4 * int(off4[-1]), dtype=np.uint32)
    for k in range(batch.n_pairs):
        cig[4 * off4[k] : 4 * off4[k] + n[k]] = batch.cigar[4 * g0[k] : 4 * g0[k] + n[k]]
    cut = int((n < reads["n_cigar"]).sum())
    reads["cigar_off4"] = off4[:-1].astype(np.uint32)
    reads["n_cigar"] = n.astype(np.uint32)
    return B.Batch(cigar=cig, reads=reads, pair_read=np.arange(batch.n_pairs, dtype=np.uint32), locus_pair_off=batch.locus_pair_off.copy(),
                   locus_start=batch.locus_start.copy(), locus_end=batch.locus_end.copy(), minlen=batch.minlen,
                   support=batch.support, unphased=batch.unphased), cut


def test_cutting_a_promised_read_behind_the_window_changes_nothing(orc):
    """The premise of walk_pairs_rows (csrc/cigar_walk.h) and of bench.py's byte accounting: a promised read cut after the
    64-op piece that takes pos + 1 + consumed past end_ext keeps its Call and its fetch / keep / clip bits, hence the
    locus' rows and ties.  Checked on the oracle alone, with the cut `_walked_groups` reports."""
    from tests.test_gpu_window_walk import _edge_batch

    cases = [(f"random_case {s}", gen.random_case(300 + s, n_loci=25, unphased=bool(s & 1), long_every=5)[0]) for s in range(6)]
    cases += [(f"edge_batch {u} {s}", _edge_batch(u, s)) for u in (False, True) for s in range(3)]
    cases += [(f"row_walk_case {s}", gen.row_walk_case(s, max_depth=300)[0]) for s in range(20)]
    total_cut = 0
    for name, batch in cases:
        gen.set_promise(batch, "all")
        code, want = orc.call_batch(batch, debug=True)
        short, cut = _truncated_copy(batch)
        assert cut > 20, f"{name}: {cut} pairs cut short"
        assert checked_mask(short).all()
        code2, got = orc.call_batch(short, debug=True)
        assert code == code2 == B.INQ_OK
        bad = np.nonzero((got.pair_call != want.pair_call) | (got.pair_bits != want.pair_bits))[0]
        assert bad.size == 0, f"{name}: pairs {bad[:8]} differ once cut"
        assert _same_result(got, want), name
        total_cut += cut
    assert total_cut > 3000
