"""The per-read Calls behind each row on the GPU (inq_read_call_t): the *_reads entry points against lists derived from the ORACLE's
per-pair outputs (hand-written ones for a hand-built locus) over every shape the compaction's tiles can take, and `--read-calls` end to
end through both front ends and several devices against a plain-Python restatement."""
import os
import subprocess

import numpy as np
import pytest

from inquistr_amd import batch as B
from inquistr_amd import call, hipcall
from oracle import pyoracle as py
from tests import gen
from tests.test_gpu_evidence import expected_evidence
from tests.test_read_calls_host import HEADER, parse_list, row_text
from tests.test_tie_report import make_tie_case, row_order

pytestmark = pytest.mark.gpu

RC = hipcall.READ_CALL_DTYPE
EV = hipcall.EVIDENCE_DTYPE


@pytest.fixture(scope="module")
def ctx():
    c = hipcall.Context(0)
    assert c.backend.startswith("hip:gfx950")
    yield c
    c.close()


# ---- expected lists: from the oracle's per-pair outputs, never from the library --------------------------------------------------
def expected_read_calls(batch, want):
    """(kept_off [n_loci + 1], records) from pair_bits / pair_call of an oracle run (debug=True) and the descriptors' phase: the kept
    pairs in pair order"""
    bits = want.pair_bits.astype(np.int64)
    kept = (bits & B.INQ_PAIR_KEPT) != 0
    idx = np.nonzero(kept)[0]
    rec = np.zeros(len(idx), dtype=RC)
    rec["call"] = want.pair_call[idx]
    rec["read"] = batch.pair_read[idx]
    if not batch.unphased:
        rec["group"] = batch.reads["phase"][batch.pair_read[idx]]
    rec["flags"] = np.where(bits[idx] & B.INQ_PAIR_CLIP, hipcall.READ_CALL_CLIP, 0)
    before = np.concatenate([[0], np.cumsum(kept)]).astype(np.uint64)
    return before[batch.locus_pair_off.astype(np.int64)], rec


_ORACLE = {}


def _oracle(orc, key, batch):
    """(oracle Result with per-pair outputs, expected kept_off, expected records) of a batch, computed once per module"""
    if key not in _ORACLE:
        if batch.n_loci:
            oc, want = orc.call_batch(batch, debug=True, threads=8)
            assert oc == 0
        else:
            want = B.Result.alloc(batch, debug=True)
        _ORACLE[key] = (want,) + expected_read_calls(batch, want)
    return _ORACLE[key]


def _assert_lists(off, rec, exp_off, exp_rec, what=""):
    assert off.dtype == np.uint64 and np.array_equal(off, exp_off), f"{what}: kept_off"
    assert rec.dtype == RC and rec.shape == exp_rec.shape, what
    if rec.tobytes() != exp_rec.tobytes():
        bad = [i for i in range(len(exp_rec)) if rec[i].tobytes() != exp_rec[i].tobytes()]
        raise AssertionError(f"{what}: {len(bad)} records differ, first {bad[0]}: got {rec[bad[0]]}, want {exp_rec[bad[0]]}")


def _device_call(ctx, batch, lists=True, evidence=True, pair_outputs=True, check=True):
    """The batch through inq_call_batch_device_reads with torch tensors, on torch's stream.  Returns (code of the enqueue, status code,
    Result, flags, evidence, kept_off, ALL n_pairs record slots); every output starts as 0xFF bytes."""
    import torch

    dev = torch.device("cuda:0")

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)

    t = {k: up(getattr(batch, k)) for k in ("cigar", "reads", "pair_read", "locus_pair_off", "locus_start", "locus_end")}
    n = max(batch.n_loci, 1)
    p1 = torch.full((n,), 7.0, dtype=torch.float64, device=dev)
    p2 = torch.full((n,), 7.0, dtype=torch.float64, device=dev)
    pc = torch.zeros(max(batch.n_pairs, 1), dtype=torch.int64, device=dev)
    pb = torch.zeros(max(batch.n_pairs, 1), dtype=torch.uint8, device=dev)
    fl = torch.full((n,), 0xFF, dtype=torch.uint8, device=dev)
    ev = torch.full((n * EV.itemsize,), 0xFF, dtype=torch.uint8, device=dev)
    ko = torch.full(((batch.n_loci + 1) * 8,), 0xFF, dtype=torch.uint8, device=dev)
    kr = torch.full((max(batch.n_pairs, 1) * RC.itemsize,), 0xFF, dtype=torch.uint8, device=dev)
    b = B.InqBatchC()
    b.n_reads, b.n_cigar_words, b.n_pairs, b.n_loci = batch.n_reads, int(batch.cigar.shape[0]), batch.n_pairs, batch.n_loci
    for k, v in t.items():
        setattr(b, k, v.data_ptr())
    b.minlen, b.support, b.unphased, b.reserved = int(batch.minlen), int(batch.support), int(batch.unphased), 0
    r = B.InqResultC(p1.data_ptr(), p2.data_ptr(), pc.data_ptr() if pair_outputs else None, pb.data_ptr() if pair_outputs else None, 0)
    torch.cuda.synchronize()  # the uploads and fills are there: the enqueue below does not wait for torch's own work
    code = ctx.call_batch_device_reads(b, r, fl.data_ptr(), ev.data_ptr() if evidence else None, ko.data_ptr() if lists else None,
                                       kr.data_ptr() if lists else None, torch.cuda.current_stream().cuda_stream, check=check)
    rc, ties = ctx.status()  # (waits for the device)
    res = B.Result(phase1=p1.cpu().numpy()[: batch.n_loci], phase2=p2.cpu().numpy()[: batch.n_loci], pair_call=pc.cpu().numpy()[: batch.n_pairs],
                   pair_bits=pb.cpu().numpy()[: batch.n_pairs], n_tie_loci=ties)
    return (code, rc, res, fl.cpu().numpy()[: batch.n_loci], ev.cpu().numpy().view(EV)[: batch.n_loci], ko.cpu().numpy().view(np.uint64),
            kr.cpu().numpy().view(RC))


def _check_both_entries(ctx, batch, want, exp_off, exp_rec, what):
    """Host entry and device entry with the lists: the oracle-derived offsets and records; every byte of kept_off and of the records
    [0, total) written, the bytes behind still 0xFF; rows, flags, tie count, evidence and per-pair outputs those of the same call
    without the lists, and kept_off's differences the evidence's n_kept."""
    total = len(exp_rec)
    rc0, plain, flags0, ev0 = ctx.call_batch_evidence(batch, debug=True)
    assert rc0 == 0, what
    rc, got, flags, ev, off, rec = ctx.call_batch_reads(batch, debug=True)
    assert rc == 0, what
    _assert_lists(off, rec, exp_off, exp_rec, what + " host entry")
    if batch.n_loci == 0:
        return  # (the device entry has nothing to launch on)
    code, rc2, got2, flags2, ev2, off2, slots = _device_call(ctx, batch)
    assert code == 0 and rc2 == 0, what
    _assert_lists(off2, slots[:total], exp_off, exp_rec, what + " device entry")
    assert (slots[total:].view(np.uint8) == 0xFF).all(), f"{what}: records at and behind kept_off[n_loci] are not written"
    assert not rec["reserved"].any() and not slots[:total]["reserved"].any()
    for g, f, e in ((got, flags, ev), (got2, flags2, ev2)):
        assert gen.same_f64(g.phase1, plain.phase1) and gen.same_f64(g.phase2, plain.phase2), what
        assert np.array_equal(f, flags0) and g.n_tie_loci == plain.n_tie_loci, what
        assert e.tobytes() == ev0.tobytes(), what
        assert np.array_equal(g.pair_call, want.pair_call) and np.array_equal(g.pair_bits, want.pair_bits), what
        assert np.array_equal(np.diff(exp_off.astype(np.int64)), e["n_kept"]), what
    # nothing else asked for: no flags, no evidence, no per-pair outputs of the caller's
    rc3, got3, f3, e3, off3, rec3 = ctx.call_batch_reads(batch, debug=False, flags=False, evidence=False)
    assert rc3 == 0 and f3 is None and e3 is None and got3.pair_call is None
    _assert_lists(off3, rec3, exp_off, exp_rec, what + " host entry, nothing else asked for")
    assert gen.same_f64(got3.phase1, plain.phase1) and gen.same_f64(got3.phase2, plain.phase2)


# ---- a hand-built locus -----------------------------------------------------------------------------------------------------------
def _hand_built(unphased):
    """Locus 0 = chr:1000-1050 (window 990 .. 1060, minlen 5) with one read of every kind the record tells apart; locus 1 has no pairs;
    every read of locus 2 is fetched and filtered (mapq 5)."""
    bb = B.BatchBuilder(minlen=5, support=3, unphased=unphased)
    enc = B.encode_cigar
    reads = [
        # (pos, cigar, mapq, phase, is_2d)                                  read  unphased          phased
        (100, [("M", 50)], 60, 1, False),                          # 0     ends at 150: not fetched
        (900, [("M", 300)], 10, 1, False),                         # 1     mapq 10: fetched only
        (900, [("M", 130)], 60, 2, False),                         # 2     fetched only      HP 2, Span 0
        (900, [("M", 300)], 60, None, False),                      # 3     Span 0            no HP: fetched only
        (900, [("M", 300)], 60, 0, False),                         # 4     Span 0            HP 0, Span 0
        (900, [("M", 120), ("I", 12), ("M", 180)], 60, 1, False),  # 5     Span 12           HP 1
        (900, [("M", 120), ("D", 20), ("M", 180)], 60, 2, False),  # 6     Span -20          HP 2
        (900, [("M", 110), ("I", 7), ("M", 190)], 60, 1, False),   # 7     Span 7            HP 1
        (900, [("M", 300)], 11, 2, False),                         # 8     Span 0            HP 2
        (990, [("S", 10), ("M", 200)], 60, 2, False),              # 9     Clip 10           HP 2
        (990, [("S", 10), ("M", 200)], 60, 1, True),               # 10    Span 0 (2D)       HP 1
    ]
    idx = [bb.add_read(pos, enc(cig), mapq=mq, phase=ph, is_2d=twod) for pos, cig, mq, ph, twod in reads]
    bb.add_locus(1000, 1050, idx)
    bb.add_locus(2000, 2050, [])
    idx = [bb.add_read(2900, enc([("M", 300)]), mapq=5, phase=1 + k % 2) for k in range(3)]
    bb.add_locus(3000, 3050, idx)
    c = hipcall.READ_CALL_CLIP
    #         (call, read, group, flags, reserved)
    if unphased:
        rec = [(0, 3, 0, 0, 0), (0, 4, 0, 0, 0), (12, 5, 0, 0, 0), (-20, 6, 0, 0, 0), (7, 7, 0, 0, 0), (0, 8, 0, 0, 0), (10, 9, 0, c, 0), (0, 10, 0, 0, 0)]
    else:
        rec = [(0, 2, 2, 0, 0), (0, 4, 0, 0, 0), (12, 5, 1, 0, 0), (-20, 6, 2, 0, 0), (7, 7, 1, 0, 0), (0, 8, 2, 0, 0), (10, 9, 2, c, 0), (0, 10, 1, 0, 0)]
    return bb.build(), np.array([0, 8, 8, 8], dtype=np.uint64), np.array(rec, dtype=RC)


@pytest.mark.parametrize("unphased", [False, True])
def test_hand_built_locus(ctx, orc, unphased):
    batch, off_by_hand, rec_by_hand = _hand_built(unphased)
    want, exp_off, exp_rec = _oracle(orc, ("hand", unphased), batch)
    _assert_lists(exp_off, exp_rec, off_by_hand, rec_by_hand, "the oracle-derived lists against the hand-written ones")
    _check_both_entries(ctx, batch, want, off_by_hand, rec_by_hand, f"hand-built unphased={unphased}")


# ---- random batches ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unphased", [False, True])
@pytest.mark.parametrize("n_loci", [1, 3, 4, 5, 40])
def test_random_batches(ctx, orc, n_loci, unphased):
    for seed in (11, 12, 13):
        batch, _ = gen.random_case(990_000 + seed, n_loci=n_loci, unphased=unphased)
        want, exp_off, exp_rec = _oracle(orc, ("random", seed, n_loci, unphased), batch)
        for variant in ("none", "all"):  # (what a read promises changes the walk, never the Calls)
            name = gen.set_promise(batch, variant)
            _check_both_entries(ctx, batch, want, exp_off, exp_rec, f"random seed={seed} n_loci={n_loci} unphased={unphased} {name}")


# ---- every depth ------------------------------------------------------------------------------------------------------------------
def _ladder(orc, unphased):
    batch, depths = gen.depth_ladder_case(31, unphased, 3)
    return (batch, depths) + _oracle(orc, ("ladder", unphased), batch)


@pytest.mark.parametrize("unphased", [False, True])
def test_every_depth(ctx, orc, unphased):
    """One locus at each of 0, 1, 64, 65, ..., 65 537, 70 001 pairs: the compaction does not know a locus's depth, the deep ones span
    many tiles"""
    batch, depths, want, exp_off, exp_rec = _ladder(orc, unphased)
    T = ctx._L.inq_read_call_tile()
    n_kept = np.diff(exp_off.astype(np.int64))
    deep = np.array(depths) > 4 * T
    assert 0 in depths and 1 in depths and 70_001 in depths and deep.sum() >= 2
    assert (n_kept[deep] > 0).all() and (n_kept[deep] < np.array(depths)[deep]).all(), "deep loci with unkept pairs"
    if not unphased:
        for j in np.nonzero(deep)[0]:
            assert (exp_rec["group"][int(exp_off[j]) : int(exp_off[j + 1])] == 0).any(), "deep loci with HP 0 reads"
    assert exp_rec["flags"].any() and (exp_rec["call"] < 0).any()
    _check_both_entries(ctx, batch, want, exp_off, exp_rec, f"ladder unphased={unphased}")


# ---- tile geometry ----------------------------------------------------------------------------------------------------------------
# a pool of eight reads over the locus chr:1000-1050 (window 990 .. 1060), offered many times
KEPT, UNKEPT = (0, 1, 2, 3, 6, 7), (4, 5)


def _pool(unphased):
    bb = B.BatchBuilder(minlen=5, support=3, unphased=unphased)
    enc = B.encode_cigar
    for pos, cig, mq, ph in [
        (900, [("M", 300)], 60, 1),                         # 0  kept, HP 1, Span 0
        (900, [("M", 120), ("I", 12), ("M", 180)], 60, 2),  # 1  kept, HP 2, Span 12
        (900, [("M", 120), ("D", 20), ("M", 180)], 60, 0),  # 2  kept, HP 0, Span -20
        (990, [("S", 10), ("M", 200)], 60, 1),              # 3  kept, HP 1, Clip 10
        (900, [("M", 300)], 5, 2),                          # 4  mapq 5: fetched, not kept
        (100, [("M", 50)], 60, 1),                          # 5  not fetched
        (900, [("M", 110), ("I", 7), ("M", 190)], 60, 2),   # 6  kept, HP 2, Span 7
        (900, [("M", 300)], 11, 1),                         # 7  kept, HP 1, Span 0
    ]:
        bb.add_read(pos, enc(cig), mapq=mq, phase=ph)
    bb.add_locus(1000, 1050, [])
    return bb.build()


def _tiled(unphased, pair_read, sizes):
    """the pool's reads offered as pair_read to loci of the given sizes, all over the same window"""
    base = _pool(unphased)
    sizes = np.asarray(sizes, dtype=np.int64)
    assert int(sizes.sum()) == len(pair_read)
    n = len(sizes)
    return B.Batch(cigar=base.cigar, reads=base.reads, pair_read=np.asarray(pair_read, dtype=np.uint32),
                   locus_pair_off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64), locus_start=np.full(n, 1000, dtype=np.uint32),
                   locus_end=np.full(n, 1050, dtype=np.uint32), minlen=5, support=3, unphased=unphased)


def _mixed(n, seed):
    return np.random.default_rng(seed).integers(0, 8, size=n)


def _geometry(name, T, unphased):
    """(Batch, check(kept flags per pair, kept_off, records) asserting the property the case is named for)"""
    kept_pool = np.array(KEPT)
    none = lambda kept, off, rec: None
    if name.startswith("total="):
        n = {"0": 0, "1": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "2T": 2 * T, "2T+1": 2 * T + 1, "3T+5": 3 * T + 5}[name[6:]]
        return _tiled(unphased, _mixed(n, n), [n // 3, 0, n - n // 3]), none
    if name == "loci on tile boundaries":
        return _tiled(unphased, _mixed(3 * T, 1), [T, T, T]), none
    if name == "one locus over three tiles":
        def check(kept, off, rec):
            assert all(kept[a:b].any() for a, b in ((T - 3, T), (T, 2 * T), (2 * T, 2 * T + 3))), "kept pairs of the locus in each of its tiles"
        return _tiled(unphased, _mixed(2 * T + 10, 2), [T - 3, T + 6, 7]), check
    if name.startswith("empty runs of "):
        run = int(name.split()[-1])
        sizes = [0] * run + [T] + [0] * run + [T // 2] + [0] * run + [T // 2 + 7] + [0] * run  # at 0, at T, at T + T / 2, at the end
        def check(kept, off, rec):
            d = np.diff(off.astype(np.int64))
            assert (d == 0).sum() >= 4 * run and off[run] == 0 and off[-1] == off[-1 - run] == len(rec) > 0
        return _tiled(unphased, _mixed(2 * T + 7, 3), sizes), check
    if name == "all loci empty":
        return _tiled(unphased, [], [0] * 5), none
    if name == "no locus":
        return _tiled(unphased, [], []), none
    if name == "a tile without a kept pair, a tile of kept pairs":
        rng = np.random.default_rng(4)
        pr = np.concatenate([rng.choice(UNKEPT, T), rng.choice(kept_pool, T), _mixed(100, 5)])
        def check(kept, off, rec):
            assert not kept[:T].any() and kept[T : 2 * T].all()
        return _tiled(unphased, pr, [T + 10, T - 20, 110]), check
    if name == "kept pairs at the end of one tile and the start of the next":
        pr = np.full(2 * T, 4)
        pr[T - 1], pr[T] = 3, 1
        def check(kept, off, rec):
            assert list(np.nonzero(kept)[0]) == [T - 1, T] and len(rec) == 2
        return _tiled(unphased, pr, [5, 2 * T - 5]), check
    raise AssertionError(name)


GEOMETRY = ([f"total={n}" for n in ("0", "1", "T-1", "T", "T+1", "2T", "2T+1", "3T+5")]
            + ["loci on tile boundaries", "one locus over three tiles", "empty runs of 1", "empty runs of 2", "empty runs of 70", "all loci empty",
               "no locus", "a tile without a kept pair, a tile of kept pairs", "kept pairs at the end of one tile and the start of the next"])


@pytest.mark.parametrize("unphased", [False, True])
@pytest.mark.parametrize("name", GEOMETRY)
def test_tile_geometry(ctx, orc, name, unphased):
    T = int(ctx._L.inq_read_call_tile())
    assert T >= 64
    batch, check = _geometry(name, T, unphased)
    want, exp_off, exp_rec = _oracle(orc, ("tile", name, unphased), batch)
    kept = (want.pair_bits & B.INQ_PAIR_KEPT) != 0
    check(kept, exp_off, exp_rec)
    if batch.n_pairs >= 8:  # the pool does what it was built for: kept and unkept, a Clip, and (phased) every HP
        assert kept.any() and not kept.all() and (name.startswith("kept pairs") or exp_rec["flags"].any())
        assert np.array_equal(kept, np.isin(batch.pair_read, KEPT))
        if not unphased and not name.startswith("kept pairs"):
            assert set(exp_rec["group"]) == {0, 1, 2}
    _check_both_entries(ctx, batch, want, exp_off, exp_rec, f"{name} unphased={unphased}")


# ---- the contract of the device entry ----------------------------------------------------------------------------------------------
def test_device_entry_needs_the_per_pair_outputs(ctx, orc):
    batch, _ = gen.random_case(990_011, n_loci=5, unphased=False)
    want, exp_off, exp_rec = _oracle(orc, ("random", 11, 5, False), batch)
    code, rc, _res, _flags, _ev, off, slots = _device_call(ctx, batch, evidence=False, pair_outputs=False, check=False)
    assert code == B.INQ_ERR_ARG and rc == 0
    assert (off.view(np.uint8) == 0xFF).all() and (slots.view(np.uint8) == 0xFF).all()  # nothing was enqueued


def test_device_entry_without_the_lists_is_the_evidence_entry(ctx, orc):
    batch, _ = gen.random_case(990_011, n_loci=5, unphased=False)
    want, exp_off, exp_rec = _oracle(orc, ("random", 11, 5, False), batch)
    rc0, plain, flags0, ev0 = ctx.call_batch_evidence(batch, debug=True)
    code, rc, res, flags, ev, off, slots = _device_call(ctx, batch, lists=False)
    assert code == 0 and rc == 0
    assert (off.view(np.uint8) == 0xFF).all() and (slots.view(np.uint8) == 0xFF).all()
    assert ev.tobytes() == ev0.tobytes() and np.array_equal(flags, flags0)
    assert gen.same_f64(res.phase1, plain.phase1) and gen.same_f64(res.phase2, plain.phase2)
    # ... and the per-pair outputs stay optional without evidence and lists
    code, rc, res, _flags, _ev, _off, _slots = _device_call(ctx, batch, lists=False, evidence=False, pair_outputs=False)
    assert code == 0 and rc == 0 and gen.same_f64(res.phase1, plain.phase1)


def test_one_context_several_calls(orc):
    """With the lists, without, then with them on a larger batch (the scratch grows), then small again: each call is right, and
    inq_read_calls_fetch offers the last call's records and no more."""
    small, _ = gen.random_case(990_021, n_loci=5, unphased=True)
    want_s, off_s, rec_s = _oracle(orc, ("random", 21, 5, True), small)
    big, _depths, want_b, off_b, rec_b = _ladder(orc, True)
    assert 0 < len(rec_s) < len(rec_b)
    with hipcall.Context(0) as c:
        rc, got, _fl, _ev, off, rec = c.call_batch_reads(small)
        assert rc == 0
        _assert_lists(off, rec, off_s, rec_s, "first call")
        assert c.read_calls_fetch(len(rec_s) + 1, check=False)[0] == B.INQ_ERR_ARG
        assert c.read_calls_fetch(2).tobytes() == rec_s[:2].tobytes()
        rc, plain, flags = c.call_batch_flags(small)
        assert rc == 0 and gen.same_f64(plain.phase1, got.phase1) and gen.same_f64(plain.phase2, got.phase2)
        assert c.read_calls_fetch(1, check=False)[0] == B.INQ_ERR_ARG  # a call without the lists offers none
        assert c.read_calls_fetch(0, check=False)[0] == 0
        rc, got_b, _fl, _ev, off, rec = c.call_batch_reads(big)
        assert rc == 0
        _assert_lists(off, rec, off_b, rec_b, "third call, larger batch")
        assert c.read_calls_fetch(len(rec_b) + 1, check=False)[0] == B.INQ_ERR_ARG
        rc, got, _fl, _ev, off, rec = c.call_batch_reads(small)
        assert rc == 0
        _assert_lists(off, rec, off_s, rec_s, "fourth call, small again")
        assert c.read_calls_fetch(len(rec_s) + 1, check=False)[0] == B.INQ_ERR_ARG


# ---- the deferred batch -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,unphased", [(41, False), (42, True)])
def test_flush_with_the_lists(ctx, orc, tmp_path, seed, unphased):
    from tests.test_host_frontend import _make_case

    minlen, support = 5, 3
    bam, bed, _loci, _recs = _make_case(tmp_path, seed, n_loci=40)
    sp = call.Spans(bam, region_file=bed, minlen=minlen, support=support, threads=2, unphased=unphased, max_comp_bytes=8_000)
    spans = [{k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in s.items()} for s in sp.spans()][:2]
    sp.close()
    assert len(spans) == 2
    ctx.call_discard()
    sizes = {"n_cigar_words": 0, "n_reads": 0, "n_pairs": 0}
    for s in spans:
        rc, stats = ctx.call_span_deferred(s["comp"], s["blocks"], s["anchors"], s["anchor_stop"], s["locus_tid"], s["locus_start"], s["locus_end"],
                                           minlen, support, unphased)
        assert rc == 0
        for k in sizes:
            sizes[k] += int(getattr(stats, k))
    n = ctx.deferred_loci
    assert n == sum(len(s["locus_start"]) for s in spans)
    rc, p1, p2, ties, _ms, flags, ev, off, rec = ctx.call_flush_reads()
    assert rc == 0 and len(ev) == n and len(off) == n + 1

    class St:
        n_cigar_words, n_reads, n_pairs = sizes["n_cigar_words"], sizes["n_reads"], sizes["n_pairs"]

    cigar, reads, pair_read, poff = ctx.span_fetch_batch(St, n)
    batch = B.Batch(cigar=cigar, reads=reads, pair_read=pair_read, locus_pair_off=poff,
                    locus_start=np.concatenate([s["locus_start"] for s in spans]).astype(np.uint32),
                    locus_end=np.concatenate([s["locus_end"] for s in spans]).astype(np.uint32), minlen=minlen, support=support, unphased=unphased)
    oc, want = orc.call_batch(batch, debug=True)
    assert oc == 0
    exp_off, exp_rec = expected_read_calls(batch, want)
    _assert_lists(off, rec, exp_off, exp_rec, "flush")  # (`read` indexes the reads span_fetch_batch returned)
    assert ev.tobytes() == expected_evidence(batch, want).tobytes()
    assert gen.same_f64(p1, want.phase1) and gen.same_f64(p2, want.phase2) and ties == want.n_tie_loci == int(flags.sum())
    assert len(exp_rec) > 0 and batch.n_pairs > len(exp_rec)
    assert ctx.read_calls_fetch(len(exp_rec) + 1, check=False)[0] == B.INQ_ERR_ARG


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def file_calls(loci, recs, unphased, minlen):
    """The kept Calls of every BED line as (kind, value, HP) in file order, restated on the records the BAM was written from; and how
    many records fetch() yields"""
    out = []
    for _chrom, s, e, t in loci:
        se, ee = s - 10, e + 10
        fetched = py._fetch(recs[t], t, se, ee)
        calls = []
        for r in fetched:
            if unphased:
                if se < (r.pos & py.U32) or (py.reference_end(r) & py.U32) < ee or r.mapq <= 10:
                    continue
                phase = 0
            else:
                phase = py.get_phase(r)
                if phase is None or (se < (r.pos & py.U32) and (py.reference_end(r) & py.U32) < ee) or r.mapq <= 10:
                    continue
            calls.append(py.call_from_cigar(r, minlen, se, ee) + (phase,))
        out.append((calls, len(fetched)))
    return out


def calls_text(loci, calls, unphased, threads):
    return HEADER + "\n" + "".join(row_text(loci[i][0], loci[i][1], loci[i][2], calls[i][0], unphased) + "\n" for i in row_order(loci, threads))


def _check_against_inq(inq_text, rc_text, support=3):
    """every row's two numbers are median_str_length of the parsed h1 / h2"""
    rows, lines = inq_text.splitlines()[1:], rc_text.splitlines()[1:]
    assert len(rows) == len(lines)
    for row, line in zip(rows, lines):
        a, b = row.split("\t"), line.split("\t")
        assert a[:3] == b[:3] and len(b) == 6
        assert a[3] == py.format_f64(py.median_str_length(parse_list(b[3]), support)), line
        assert a[4] == py.format_f64(py.median_str_length(parse_list(b[4]), support)), line


def _check_against_evidence(ev_text, rc_text):
    for eline, line in zip(ev_text.splitlines()[1:], rc_text.splitlines()[1:]):
        e, b = eline.split("\t"), line.split("\t")
        h1, h2, other = (parse_list(x) for x in b[3:])
        assert e[:3] == b[:3] and int(e[4]) == len(h1) + len(h2) + len(other) and (int(e[5]), int(e[6])) == (len(h1), len(h2))
        vals = [v for _k, v in h1 + h2]
        assert int(e[7]) == sum(1 for k, _v in h1 + h2 if k == "Clip")
        assert (e[8], e[9]) == ((str(min(vals)), str(max(vals))) if vals else (".", "."))


def _cli(args, env):
    e = dict(os.environ)
    e.pop("INQ_SERVER", None)
    e.update(env)
    return subprocess.run([call.CLI_PATH] + args, capture_output=True, text=True, env=e, timeout=300)


@pytest.mark.parametrize("frontend", ["host", "device"])
@pytest.mark.parametrize("unphased", [False, True])
def test_end_to_end(tmp_path, frontend, unphased):
    from tests.test_host_frontend import _make_case

    bam, bed, loci, recs = _make_case(tmp_path, 51, n_loci=40)
    calls = file_calls(loci, recs, unphased, 5)
    # what the case must hold for the file to say anything
    group = lambda c, g: [x for x in c if unphased or x[2] == g]
    assert any((len(c) // 2 if unphased else len(group(c, 1))) < 3 for c, _f in calls), "a NaN row"
    assert any(k == "Clip" for c, _f in calls for k, _v, _g in c) and any(v < 0 for c, _f in calls for _k, v, _g in c)
    assert any(f > len(c) for c, f in calls), "a row with fetched > kept"
    assert row_order(loci, 4) != row_order(loci, 1)
    u = ["-u"] if unphased else []
    for threads in (1, 4):
        want = calls_text(loci, calls, unphased, threads)
        plain, with_r = tmp_path / f"plain{threads}.inq", tmp_path / f"r{threads}.inq"
        rcf, evf = tmp_path / f"r{threads}.tsv", tmp_path / f"e{threads}.tsv"
        with open(plain, "w") as f:
            call.genotype_repeats(bam, None, bed, 5, 3, threads, unphased, None, None, out=f, frontend=frontend)
        with open(with_r, "w") as f:
            call.genotype_repeats(bam, None, bed, 5, 3, threads, unphased, None, None, out=f, frontend=frontend, evidence=str(evf), read_calls=str(rcf))
        assert with_r.read_bytes() == plain.read_bytes()
        assert rcf.read_text() == want, f"library, -t {threads}"
        assert "NaN" in plain.read_text()
        _check_against_inq(plain.read_text(), rcf.read_text())
        _check_against_evidence(evf.read_text(), rcf.read_text())
        env = {"INQ_FRONTEND": frontend}
        p = _cli(["call", bam, "-R", bed, "-t", str(threads)] + u, env)
        assert p.returncode == 0, p.stderr
        cli_rc = tmp_path / f"cli{threads}.tsv"
        r = _cli(["call", bam, "-R", bed, "-t", str(threads), "--read-calls", str(cli_rc)] + u, env)
        assert r.returncode == 0, r.stderr
        assert r.stdout == p.stdout and r.stderr == p.stderr and r.stdout == plain.read_text()
        assert cli_rc.read_text() == want, f"CLI, -t {threads}"
    dev_rc = tmp_path / "devices.tsv"
    r = _cli(["call", bam, "-R", bed, "-t", "4", "--devices", "0,0", f"--read-calls={dev_rc}"] + u, {"INQ_FRONTEND": frontend})
    assert r.returncode == 0, r.stderr
    assert r.stdout == (tmp_path / "plain4.inq").read_text()
    assert dev_rc.read_text() == calls_text(loci, calls, unphased, 4), "--devices 0,0"


def test_ties(tmp_path):
    """On the loci of the tie report the split is the file-order one, and the median invariant holds all the same."""
    bam, bed, loci, recs, ties = make_tie_case(tmp_path)
    assert any(ties)
    calls = file_calls(loci, recs, True, 5)
    inq, rcf, tf = tmp_path / "t.inq", tmp_path / "t.tsv", tmp_path / "t.bed"
    with open(inq, "w") as f:
        call.genotype_repeats(bam, None, bed, 5, 3, 1, True, None, None, out=f, ties=str(tf), read_calls=str(rcf))
    assert rcf.read_text() == calls_text(loci, calls, True, 1)
    _check_against_inq(inq.read_text(), rcf.read_text())
    reported = {tuple(l.split("\t")) for l in tf.read_text().splitlines()}
    assert reported == {(c, str(s), str(e)) for (c, s, e, _t), tie in zip(loci, ties) if tie}
    for line in rcf.read_text().splitlines()[1:]:
        b = line.split("\t")
        if tuple(b[:3]) in reported:  # equal values of both kinds on the two sides of the split
            h1, h2 = parse_list(b[3]), parse_list(b[4])
            assert h1[-1][1] == h2[0][1] and {k for k, v in h1 + h2 if v == h2[0][1]} == {"Span", "Clip"}
