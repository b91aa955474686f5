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
