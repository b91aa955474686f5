"""No GPU: what the cases of tests/side_geometry_case.py claim, pinned from their inputs and the restatements alone - that consecutive
trips of one workgroup meet every ordered pair of locus kinds, that items one trip apart have different answers, that the counts leave a
partial last tile at every grid, and that the scan cases reach the second step with the carry they are named for."""
import numpy as np
import pytest

from inquistr_amd import batch as B
from tests import locus_motif_case as lm
from tests import read_motif_case as rm
from tests import read_seq_case as rs
from tests import side_geometry_case as sg
from tests.test_gpu_read_calls import KEPT

ALL_PAIRS = {(a, b) for a in sg.KINDS for b in sg.KINDS}


def _differs(rec, d):
    """per item i >= d: does its expected record differ from that of item i - d"""
    raw = np.ascontiguousarray(rec).view(np.uint8).reshape(len(rec), -1)
    return (raw[d:] != raw[:-d]).any(axis=1)


def test_counts_leave_a_partial_tile_at_every_grid():
    assert sg.CAPS == (1, 2, 3, 7) and sg.GRID_SIDES == (1, 2, 3, 7, 0)
    assert sg.N_SMALL == 16 * (3 * 7 + 1) + 5 == 357 and sg.READ_MOTIF_TILE == sg.SEQ_WINDOW_TILE == 16
    tiles = -(-sg.N_SMALL // 16)
    assert sg.N_SMALL % 16 and all(tiles > 3 * c for c in sg.CAPS), "every workgroup takes at least three trips, the last tile is partial"
    assert sg.N_BIG == 16 * sg.GRID_CAP + 16 + 1 and sg.GRID_CAP == 65536
    # item j and item j + GRID_CAP k are different members of a pool
    assert sg.POOL % 2 == 1 and all((sg.GRID_CAP * k) % sg.POOL for k in (1, 2)) and (16 * sg.GRID_CAP) % sg.POOL


def test_small_loci_put_every_pair_of_kinds_on_consecutive_trips():
    slices, kept_off, kinds, given, want = sg.small_locus_case()
    n = len(kinds)
    assert n == 400 == len(want) == len(kept_off) - 1 and all(kinds.count(k) == 80 for k in sg.KINDS)
    for j in range(n):
        assert sg.kind_of(slices[int(kept_off[j]) : int(kept_off[j + 1])], want[j]) == kinds[j], j
    a = [j for j in range(n) if kinds[j] == "a"]
    assert min(int(kept_off[j + 1] - kept_off[j]) for j in a) >= 5, "several records deep"
    assert len({int(want["word"][j]) for j in range(n) if kinds[j] == "b"}) >= 6, "another class wins from locus to locus"
    for cap in sg.CAPS:
        assert sg.trip_pairs(kinds, cap) == ALL_PAIRS, cap
    assert n < sg.GRID_CAP and sg.trip_pairs(kinds, sg.GRID_CAP) == set(), "at the default cap no workgroup takes a second locus"
    use = lm.words_in_use(given, want["word"])
    assert (use != want["word"]).any() and ((given != 0) & (use == want["word"])).any(), "given words that count and that do not"


def test_small_motif_records_differ_from_tile_to_tile():
    sq, packed, kept_off, words, want = sg.small_motif_case()
    assert len(sq) == len(want) == sg.N_SMALL and len(words) == len(kept_off) - 1
    counts = np.diff(kept_off.astype(np.int64))
    assert (counts == 0).sum() >= 5 and (counts[1:-1] == 0).any() and int(kept_off[-1]) == sg.N_SMALL - 3, "empty loci; records behind the last locus"
    filled = words[counts > 0]
    assert (filled[1:] != filled[:-1]).all(), "neighbours among the filled loci have different words"
    assert not want[-3:].view(np.uint32).any() and (want["run_len"][:-3] > 0).all()
    for cap in sg.CAPS:
        assert _differs(want, sg.READ_MOTIF_TILE * cap).all(), cap
    assert int(sq["n_bases"].max()) <= 60


def test_small_window_pairs_differ_from_tile_to_tile():
    batch, l_seq, q, n = sg.small_window_case()
    assert batch.n_pairs == sg.N_SMALL == len(q) == len(n)
    sizes = np.diff(batch.locus_pair_off.astype(np.int64))
    assert sizes.max() == 16 and (sizes == 0).any() and len({(int(s), int(e)) for s, e in zip(batch.locus_start, batch.locus_end)}) >= 20
    both = np.stack([q, n], axis=1)
    for cap in sg.CAPS:
        assert _differs(both, sg.SEQ_WINDOW_TILE * cap).all(), cap
    assert (n > 0).all() and (q.astype(np.int64) + n <= l_seq[batch.pair_read]).all() and len(set(batch.pair_read.tolist())) == batch.n_reads


@pytest.mark.parametrize("n_loci", [sg.GRID_CAP + 3, 2 * sg.GRID_CAP + 1])
def test_big_loci_repeat_a_pool_that_no_trip_repeats(n_loci):
    sq, packed, kept_off, given, found, use, kinds = sg.big_locus_case(n_loci)
    assert len(found) == len(use) == len(given) == n_loci == len(kept_off) - 1 and len(kinds) == sg.POOL
    counts = np.diff(kept_off.astype(np.int64))
    assert set(counts.tolist()) == {0, 1} and len(sq) == int(kept_off[-1]) and int(sq["n_bases"].max()) <= 24
    assert packed.size == int(((sq["n_bases"].astype(np.int64) + 1) // 2).sum())
    assert all(kinds.count(k) >= 99 for k in sg.KINDS)
    # the tiled expectation is the restatement's: a stretch across the seam of two repeats, computed afresh
    lo, hi = sg.POOL - 20, sg.POOL + 20
    seg = np.concatenate([[0], np.cumsum((sq["n_bases"].astype(np.int64) + 1) // 2)])
    codes = [np.stack((packed[seg[k] : seg[k + 1]] >> 4, packed[seg[k] : seg[k + 1]] & 15), axis=1).reshape(-1)[: int(sq["n_bases"][k])]
             for k in range(int(kept_off[lo]), int(kept_off[hi]))]
    assert lm.records_of(codes, kept_off[lo : hi + 1] - kept_off[lo]).tobytes() == found[lo:hi].tobytes()
    assert np.array_equal(use[lo:hi], lm.words_in_use(given[lo:hi], found["word"][lo:hi]))
    # the loci of the later trips: another pool member than the locus one trip before, and every pair of kinds where there are enough
    j = np.arange(sg.GRID_CAP, n_loci)
    assert ((j % sg.POOL) != ((j - sg.GRID_CAP) % sg.POOL)).all()
    tiled_kinds = [kinds[i % sg.POOL] for i in range(n_loci)]
    pairs = sg.trip_pairs(tiled_kinds, sg.GRID_CAP)
    assert len(pairs) == len(j) == 3 if n_loci == sg.GRID_CAP + 3 else pairs == ALL_PAIRS
    assert _differs(found, sg.GRID_CAP).mean() > 0.5 or len(j) == 3
    if n_loci > 2 * sg.GRID_CAP:
        assert tiled_kinds[0] != tiled_kinds[2 * sg.GRID_CAP] or found[0] != found[2 * sg.GRID_CAP], "workgroup 0's third locus"


def test_big_motif_records_differ_one_trip_apart():
    sq, packed, kept_off, words, want = sg.big_motif_case()
    assert len(sq) == len(want) == sg.N_BIG == int(kept_off[-1]) and len(words) == len(kept_off) - 1
    assert int(sq["n_bases"].max()) <= 40 and (np.diff(kept_off.astype(np.int64)) >= 0).all() and (np.diff(kept_off.astype(np.int64)) == 0).any()
    trip = sg.READ_MOTIF_TILE * sg.GRID_CAP
    assert sg.N_BIG - trip == 17 and _differs(want, trip).all() and (want["run_len"] > 0).all()
    # a record's word is its locus's, also in the last, partial repeat of the pool
    locus = np.searchsorted(kept_off, np.arange(sg.N_BIG - 600, sg.N_BIG), side="right") - 1
    seg = np.concatenate([[0], np.cumsum((sq["n_bases"].astype(np.int64) + 1) // 2)])
    codes = [np.stack((packed[seg[k] : seg[k + 1]] >> 4, packed[seg[k] : seg[k + 1]] & 15), axis=1).reshape(-1)[: int(sq["n_bases"][k])]
             for k in range(sg.N_BIG - 600, sg.N_BIG)]
    assert rm.records_of(codes, [int(words[j]) for j in locus]).tobytes() == want[-600:].tobytes()


def test_big_window_pairs_differ_one_trip_apart():
    batch, l_seq, q, n, table = sg.big_window_case()
    assert batch.n_pairs == sg.N_BIG == len(q) and batch.n_reads == 8
    sizes = np.diff(batch.locus_pair_off.astype(np.int64))
    assert 25 < sizes.mean() < 35 and (sizes == 0).any() and len(set(zip(batch.locus_start.tolist(), batch.locus_end.tolist()))) == len(sg.WINDOWS)
    assert len({tuple(x) for x in table.reshape(-1, 2).tolist()}) >= 15, "distinct answers among the (window, read) combinations"
    trip = sg.SEQ_WINDOW_TILE * sg.GRID_CAP
    assert _differs(np.stack([q, n], axis=1), trip).all() and sg.N_BIG - trip == 17
    # the gathered expectation is the formula's: the loci at both ends, computed pair by pair
    for lo, hi in ((0, 40), (batch.n_loci - 40, batch.n_loci)):
        p0, p1 = int(batch.locus_pair_off[lo]), int(batch.locus_pair_off[hi])
        part = B.Batch(cigar=batch.cigar, reads=batch.reads, pair_read=batch.pair_read[p0:p1], locus_pair_off=batch.locus_pair_off[lo : hi + 1] - np.uint64(p0),
                       locus_start=batch.locus_start[lo:hi], locus_end=batch.locus_end[lo:hi], minlen=5, support=3, unphased=True)
        want_q, want_n = rs.batch_windows(part, l_seq)
        assert np.array_equal(want_q, q[p0:p1]) and np.array_equal(want_n, n[p0:p1])


@pytest.mark.parametrize("unphased", [False, True])
@pytest.mark.parametrize("name", sg.SCAN_CASES)
def test_scan_cases_reach_the_second_step(orc, name, unphased):
    batch, want, exp_off, exp_rec = sg.scan_expected(orc, name, unphased)
    T, first = sg.READ_CALL_TILE, sg.FIRST_STEP
    assert first == 256 * T == 1 << 20
    total = {"256T": first, "256T+1": first + 1}.get(name, first + T + 5)
    assert batch.n_pairs == total and -(-total // T) == {"256T": 256, "256T+1": 257}.get(name, 258)
    off = batch.locus_pair_off.astype(np.int64)
    sizes = np.diff(off)
    assert sizes.max() <= 60 and (sizes == 0).sum() > 100 and (sizes == 1).any()
    kept = (want.pair_bits & B.INQ_PAIR_KEPT) != 0
    assert np.array_equal(kept, np.isin(batch.pair_read, KEPT))
    carry = int(kept[:first].sum())  # what the scan's first step hands to its second
    if name.startswith("carry"):
        j = int(np.nonzero(off == first)[0][0])
        assert int(exp_off[j]) == carry == 1 << 20, "the largest carry 256 tiles can hand on"
        assert kept[first:].any() and not kept[first:].all()
    else:
        j = int(np.searchsorted(off, first - 7, side="left"))
        assert off[j] == first - 7 and off[j + 1] == min(total, first - 7 + 30), "the locus at the step's edge"
        if total > first:
            assert off[j] < first < off[j + 1] and kept[first - 1] and kept[first], "it straddles pair 256 T, kept pairs on both sides"
            assert 0 < carry < first and int(exp_off[j]) < carry < int(exp_off[j + 1])
    assert int(exp_off[-1]) == len(exp_rec) == int(kept.sum()) and (len(exp_rec) > carry) == (total > first)
    if not unphased:
        assert set(exp_rec["group"][-50:].tolist()) <= {0, 1, 2} and exp_rec["flags"].any()


def test_the_kept_pair_case_keeps_more_than_2_20_pairs():
    """4 500 reads under 257 overlapping loci: with the pairs in file order under each locus, as the front end forms them, the kept
    records number 4 091 x 257, the last 2 811 of them behind index 2^20"""
    reads, loci = sg.kept_pair_reads(), sg.kept_pair_loci()
    n = len(reads)
    assert (n, len(loci), len(set(loci))) == (sg.PAIR_READS, sg.PAIR_LOCI, sg.PAIR_LOCI) and [r[2] for r in reads] == sorted(r[2] for r in reads)
    pair_read = np.tile(np.arange(n, dtype=np.uint32), len(loci))
    pair_off = np.arange(len(loci) + 1, dtype=np.uint64) * n
    q, nb, kept, kept_off = sg.kept_pair_expected(pair_read, pair_off, [s for s, _e in loci], [e for _s, e in loci])
    assert len(kept) == 1_156_500 and int(kept_off[-1]) == int(kept.sum()) == 4091 * 257 == 1_051_387
    assert int(kept_off[-1]) - sg.FIRST_STEP == 2811 and np.array_equal(np.diff(kept_off.astype(np.int64)), np.full(len(loci), 4091))
    tiles = kept[: len(kept) // sg.READ_CALL_TILE * sg.READ_CALL_TILE].reshape(-1, sg.READ_CALL_TILE).sum(axis=1)
    assert len(tiles) > sg.SCAN_STEP and (tiles < sg.READ_CALL_TILE).all() and (tiles > 0).all(), "kept and unkept pairs in every tile"
    assert 0 < int(tiles[: sg.SCAN_STEP].sum()) < sg.FIRST_STEP, "the carry into the scan's second step"
    assert len({(int(a), int(b)) for a, b in zip(q[:n], nb[:n])}) == 7 and len({(int(a), int(b)) for a, b in zip(q, nb)}) >= 22
    assert {int(x) & 1 for x in q} == {0, 1} and {int(x) & 1 for x in nb} == {0, 1} and (q.astype(np.int64) + nb == sg.PAIR_SEQ).all()
    # the gather of the packed bytes is read_seq_case.pack of each slice
    sel = np.nonzero(kept)[0][[0, 1, 4090, 4091, sg.FIRST_STEP, -1]]
    packed = sg.packed_slices(pair_read[sel], q[sel], nb[sel])
    assert bytes(packed) == b"".join(rs.pack(reads[int(pair_read[p])][6][int(q[p]) : int(q[p]) + int(nb[p])]) for p in sel)
    raw, lens = sg.names_of(pair_read[sel])
    assert bytes(raw) == b"".join(reads[int(pair_read[p])][0].encode() for p in sel) and int(lens.sum()) == len(raw)
