"""The side kernels past their first trip, the compaction's scan past its first step.

Seven kernels launch at most a cap of workgroups and let each take every gridDim.x-th tile: locus_motif_kernel (locus_motifs.hip),
read_motif_kernel (read_motifs.hip), seq_window_kernel, seq_slice_kernel, read_seq_record_kernel (read_seqs.hip), name_copy_kernel and
read_origin_kernel (read_names.hip).  The context option "grid_side" lowers that cap, so that a few hundred items take every workgroup
round its loop several times:

  small grids   "grid_side" 1, 2, 3, 7 and 0 (each launcher's own cap): inq_locus_motifs_find, inq_motif_runs, inq_seq_windows on the
                cases of tests/side_geometry_case.py, and whole flushes (origins, sequences, motif runs, locus motifs) behind deferred spans
                with names and sequences - there the span-time name_copy, seq_window and seq_slice launches and the flush-time
                read_origin, read_seq_record, name_copy, read_motif and locus_motif launches all run under the small grid
  the real cap  option at 0: locus_motif_kernel at 65 536 + 3 and 2 * 65 536 + 1 loci, read_motif_kernel and seq_window_kernel at
                16 * 65 536 + 16 + 1 items - a pool of 499 items repeated, the restatement computed once per item
  the scan      read_call_scan at 256 T, 256 T + 1 and 256 T + T + 5 pairs (T = inq_read_call_tile), and with a carry of exactly 2^20
                into the second step, through inq_call_batch_reads and the device entry against the C oracle; and one deferred flush
                with sequences and motif runs over 4 500 reads under 257 overlapping loci - 1 156 500 pairs, 1 051 387 kept - so that
                kept_pair is written past index 2^20 from the second step's bases, and read_seq_record_kernel, the by-pair name_copy and
                read_motif_kernel read it there

Every comparison is to the restatement, byte for byte; equality with the default grid's output is asserted beside it.  In front of each
stand-alone launch the same entry runs on an input whose every answer is zeros, under another grid and into the same context buffers:
a tile that is skipped shows as zeros, not as what the run before left there; in front of each flush another file goes through the same
launches at the default grid.

Not run at their real caps: seq_slice_kernel (2 097 152 pairs), read_seq_record_kernel (16 777 216), name_copy_kernel (2^25) and
read_origin_kernel (2^28) - 2 M to 268 M items do not fit a test of a few seconds; the small grids cover their loop."""
from contextlib import contextmanager

import numpy as np
import pytest

from inquistr_amd import batch as B
from inquistr_amd import hipcall
from tests import gen
from tests import locus_motif_case as lm
from tests import read_motif_case as rm
from tests import read_seq_case as rs
from tests import side_geometry_case as sg
from tests.read_table_case import make_named_case, span_records
from tests.test_gpu_read_calls import _check_both_entries
from tests.test_gpu_read_names import _check_origins, _cut, _names_of
from tests.test_gpu_read_seqs import _append, _bed, _run, _Sizes, _spans, _write
from tools import bamio

pytestmark = pytest.mark.gpu

WIPE_GRID = sg.GRID_CAP - 1  # "grid_side" of the zeros run in front of a launch at the real cap
SPAN_BYTES = 200_000  # compressed bytes of a span at most: a few spans of some hundred records each
_DEFAULT = {}  # what a case gave at the default grid
_WANT = {}  # the restatement of a flush's records, by the lists it was computed for


@pytest.fixture(scope="module")
def ctx():
    c = hipcall.Context(0)
    assert c.backend.startswith("hip:gfx950")
    yield c
    c.close()


@contextmanager
def side_grid(c, grid):
    c.set_option("grid_side", grid)
    try:
        yield
    finally:
        c.set_option("grid_side", 0)


def _default(c, key, run):
    """run() at the default grid, once per module"""
    if key not in _DEFAULT:
        c.set_option("grid_side", 0)
        _DEFAULT[key] = run()
    return _DEFAULT[key]


def _assert_records(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        raw_g, raw_w = (np.ascontiguousarray(x).view(np.uint8).reshape(len(x), -1) for x in (got, want))
        bad = np.nonzero((raw_g != raw_w).any(axis=1))[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(want)} differ, first {bad[:8].tolist()}: got {got[bad[0]]}, want {want[bad[0]]}")


def test_the_constants_are_the_library_s(ctx):
    L = ctx._L
    assert (L.inq_read_motif_tile(), L.inq_seq_window_tile(), L.inq_read_name_tile(), L.inq_read_call_tile()) == (
        sg.READ_MOTIF_TILE, sg.SEQ_WINDOW_TILE, sg.READ_NAME_TILE, sg.READ_CALL_TILE)
    for bad in (-1, 65536, 1 << 20, 1 << 40):
        assert L.inq_ctx_set_option(ctx._h, b"grid_side", bad) == B.INQ_ERR_ARG
    for good in (65535, 1, 0):
        assert L.inq_ctx_set_option(ctx._h, b"grid_side", good) == 0


# ---- the stand-alone entries ------------------------------------------------------------------------------------------------------------
# Each runs its entry under `grid`, behind the same entry on an input whose every answer is zeros under ANOTHER grid (`wipe`: the
# default one for the small cases, where it gives every tile a workgroup of its own; one short of the cap for the large ones) - a tile
# that a grid's stride skips is not skipped by both
def _find(c, grid, sq, packed, kept_off, given, use=True, wipe=0):
    with side_grid(c, wipe):
        c.locus_motifs_find(sq, packed, np.zeros(len(kept_off), dtype=np.uint64), None)  # every locus without a record
    with side_grid(c, grid):
        return c.locus_motifs_find(sq, packed, kept_off, given, use=use)


def _runs(c, grid, sq, packed, kept_off, words, wipe=0):
    with side_grid(c, wipe):
        c.motif_runs(sq, packed, kept_off, np.zeros(len(words), dtype=np.uint64))  # no locus has a motif
    with side_grid(c, grid):
        return c.motif_runs(sq, packed, kept_off, words)


def _windows(c, grid, batch, l_seq, wipe=0):
    with side_grid(c, wipe):
        c.seq_windows(batch, np.zeros(batch.n_reads, dtype=np.uint32))  # no read has a base
    with side_grid(c, grid):
        return c.seq_windows(batch, l_seq)


@pytest.mark.parametrize("grid", sg.GRID_SIDES)
def test_locus_motifs_at_small_grids(ctx, grid):
    """400 loci of five kinds in random order: a workgroup's consecutive loci are every ordered pair of kinds, so what one locus leaves in
    bins, sums or wave_best shows in the next"""
    slices, kept_off, kinds, given, want = sg.small_locus_case()
    sq, packed = rm.seq_arrays(slices)
    base = _default(ctx, "loci", lambda: (_find(ctx, 0, sq, packed, kept_off, None), _find(ctx, 0, sq, packed, kept_off, given)))
    for g, (base_found, base_use) in zip((None, given), base):
        found, use = _find(ctx, grid, sq, packed, kept_off, g)
        bad = [(j, kinds[j - grid] if grid and j >= grid else "-", kinds[j]) for j in range(len(want)) if found[j] != want[j]]
        assert not bad, f"grid_side {grid}: (locus, kind of the locus one trip before, kind) {bad[:8]}"
        _assert_records(found, want, f"grid_side {grid}")
        assert np.array_equal(use, lm.words_in_use(g, want["word"]))
        assert found.tobytes() == base_found.tobytes() and np.array_equal(use, base_use)
        found, none = _find(ctx, grid, sq, packed, kept_off, g, use=False)
        assert none is None
        _assert_records(found, want, f"grid_side {grid}, no use")


@pytest.mark.parametrize("grid", sg.GRID_SIDES)
def test_motif_runs_at_small_grids(ctx, grid):
    sq, packed, kept_off, words, want = sg.small_motif_case()
    base = _default(ctx, "motifs", lambda: _runs(ctx, 0, sq, packed, kept_off, words))
    got = _runs(ctx, grid, sq, packed, kept_off, words)
    _assert_records(got, want, f"grid_side {grid}")
    assert got.tobytes() == base.tobytes()


@pytest.mark.parametrize("grid", sg.GRID_SIDES)
def test_seq_windows_at_small_grids(ctx, grid):
    batch, l_seq, want_q, want_n = sg.small_window_case()
    base = _default(ctx, "windows", lambda: _windows(ctx, 0, batch, l_seq))
    q, n = _windows(ctx, grid, batch, l_seq)
    _assert_records(q, want_q, f"grid_side {grid}: q_beg")
    _assert_records(n, want_n, f"grid_side {grid}: n_bases")
    assert np.array_equal(q, base[0]) and np.array_equal(n, base[1])


# ---- whole flushes --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """one BAM per kind of flush, as the kinds' own tests write them, and the spans of each"""
    tmp = tmp_path_factory.mktemp("side_geometry")
    named = make_named_case(tmp, 71, n_loci=200)
    seq = rs.make_seq_case(tmp, 72, n_loci=200)
    motif = rm.make_motif_case(tmp, 73, n_loci=120)
    # every BED line two, three and five times, a base wider each time: more than 7 x 256 kept records in each flush, so that
    # read_origin_kernel and read_seq_record_kernel (256 records a workgroup) take a second trip at every small grid
    named_bed, seq_bed, motif_bed = _widened(named[1], 2), _widened(seq[1], 3), _widened(motif[1], 5)
    return {"named": (_spans(named[0], named_bed, False, SPAN_BYTES),), "seq": (seq[0], seq_bed),
            "motif": (_spans(motif[0], motif_bed, True, 2 * SPAN_BYTES), [hipcall.encode_motif(t) for t in motif[4] for _ in range(5)])}


def _widened(bed, times):
    """the BED with every line `times` times, its end one base further each time: overlapping loci over the same reads"""
    out = bed[:-4] + f".x{times}.bed"
    with open(bed) as f, open(out, "w") as g:
        for line in f:
            c, s, e, *rest = line.rstrip("\n").split("\t")
            for r in range(times):
                g.write("\t".join([c, s, str(int(e) + r)] + rest) + "\n")
    return out


def _second_trip(n_records, grid):
    """do n_records take every workgroup of the two kernels that deal 256 records to a workgroup round its loop again under this grid"""
    return grid == 0 or n_records > sg.RECORD_TILE * grid


def _scrub(c, spans, unphased):
    """another file through every side launch at the default grid, into the context buffers the flush behind it writes: what a skipped
    tile would show is that file's, not the answer of the same flush under the grid before"""
    c.call_discard()
    assert _append(c, spans, unphased)[0] == [0] * len(spans)
    assert c.call_flush_locus_motifs(None)[0] == 0


def _same_flush(a, b, what):
    """every element of two flushes' results but the time (the fifth)"""
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        if i == 4:
            continue
        if isinstance(x, np.ndarray) and x.dtype == np.float64:
            assert gen.same_f64(x, y), (what, i)
        elif isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, i)
        else:
            assert x == y, (what, i)


def _origins_flush(c, spans):
    """deferred spans with names and sequences, then inq_call_flush_origins: the batch's names and every kept record's origin and name
    against the records read back out of the spans' inflated bytes"""
    c.call_discard()
    codes, sizes = _append(c, spans, False)
    assert codes == [0] * len(spans)
    out = c.call_flush_origins()
    rc, _p1, _p2, _ties, _ms, _fl, _ev, off, rec, org, raw, total = out
    assert rc == 0
    written = [r for s in spans for r in span_records(s)]
    assert len(written) == sizes["n_reads"]
    name_off, all_names = c.span_fetch_names(sizes["n_reads"])
    assert _cut(name_off, all_names) == [r[0] for r in written], "the batch's names"
    assert len(org) == len(rec) == int(off[-1]) and total == len(raw) == int(org["name_len"].sum())
    _check_origins(written, rec, org, _names_of(org, raw))
    return out


@pytest.mark.parametrize("grid", sg.GRID_SIDES)
def test_flush_origins_at_small_grids(ctx, files, grid):
    (spans,) = files["named"]
    assert len(spans) >= 2
    base = _default(ctx, "flush origins", lambda: _origins_flush(ctx, spans))
    _scrub(ctx, files["motif"][0], True)
    with side_grid(ctx, grid):
        out = _origins_flush(ctx, spans)
    assert _second_trip(len(out[8]), grid), len(out[8])
    _same_flush(out, base, f"grid_side {grid}")


@pytest.mark.parametrize("grid", sg.GRID_SIDES)
def test_flush_seqs_at_small_grids(ctx, files, grid):
    """test_gpu_read_seqs._run: every pair's slice at span time and every kept record's at flush time against the written records"""
    bam, bed = files["seq"]
    base = _default(ctx, "flush seqs", lambda: _run(ctx, bam, bed, True, SPAN_BYTES))
    _scrub(ctx, files["motif"][0], True)
    with side_grid(ctx, grid):
        got = _run(ctx, bam, bed, True, SPAN_BYTES)
    assert len(got["spans"]) >= 2 and _second_trip(len(got["flush"][8]), grid), len(got["flush"][8])
    _same_flush(got["flush"], base["flush"], f"grid_side {grid}")
    assert np.array_equal(got["seq_off"], base["seq_off"])


def _motif_flushes(c, spans, target_words):
    """inq_call_flush_locus_motifs and inq_call_flush_motifs behind deferred spans with sequences: the found records, the words in use
    and every kept record's runs against the restatements on the written records"""
    words = np.array([target_words[int(i)] for s in spans for i in s["locus_index"]], dtype=np.uint64)
    c.call_discard()
    assert _append(c, spans, True)[0] == [0] * len(spans)
    n_loci = c.deferred_loci
    auto = c.call_flush_locus_motifs(words)
    rc, _p1, _p2, _ties, _ms, _fl, _ev, off, rec, _org, _raw, _nt, sq, _packed, _st, mt, found = auto
    assert rc == 0 and len(found) == n_loci and len(mt) == len(rec) == int(off[-1])
    key = (off.tobytes(), rec["read"].tobytes())
    if key not in _WANT:  # (the lists are the compaction's, which no grid of a side kernel changes)
        written = [r for s in spans for r in rs.span_seq_records(s)]
        starts = np.concatenate([s["locus_start"] for s in spans])
        ends = np.concatenate([s["locus_end"] for s in spans])
        slices, windows = [], []
        for j in range(n_loci):
            for kk in range(int(off[j]), int(off[j + 1])):
                wds, pos, l_seq, codes = written[int(rec["read"][kk])]
                q, n = rs.window(wds, pos, l_seq, int(starts[j]), int(ends[j]))
                windows.append((q, n))
                slices.append(codes[q : q + n])
        want = lm.records_of(slices, off)
        per_record = lambda w: [int(w[j]) for j in range(n_loci) for _ in range(int(off[j]), int(off[j + 1]))]
        _WANT[key] = (np.array(windows, dtype=np.uint32).view(hipcall.SEQ_DTYPE).reshape(-1), want,
                      rm.records_of(slices, per_record(lm.words_in_use(words, want["word"]))), rm.records_of(slices, per_record(words)))
    want_sq, want, want_auto, want_given = _WANT[key]
    _assert_records(sq, want_sq, "slices")
    _assert_records(found, want, "found")
    _assert_records(mt, want_auto, "runs under the words in use")
    assert _append(c, spans, True)[0] == [0] * len(spans)
    given = c.call_flush_motifs(words)
    assert given[0] == 0
    _assert_records(given[15], want_given, "runs under the given words")
    return auto, given


@pytest.mark.parametrize("grid", sg.GRID_SIDES)
def test_flush_motifs_at_small_grids(ctx, files, grid):
    spans, target_words = files["motif"]
    base = _default(ctx, "flush motifs", lambda: _motif_flushes(ctx, spans, target_words))
    _scrub(ctx, files["named"][0], False)
    with side_grid(ctx, grid):
        auto, given = _motif_flushes(ctx, spans, target_words)
    assert _second_trip(len(auto[8]), grid), len(auto[8])
    _same_flush(auto, base[0], f"grid_side {grid}: locus motifs")
    _same_flush(given, base[1], f"grid_side {grid}: motifs")


# ---- the real cap ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_loci", [sg.GRID_CAP + 3, 2 * sg.GRID_CAP + 1])
def test_locus_motifs_past_the_grid_cap(ctx, n_loci):
    """three loci on a second trip; workgroup 0 on its third"""
    sq, packed, kept_off, given, found_want, use_want, _kinds = sg.big_locus_case(n_loci)
    found, use = _find(ctx, 0, sq, packed, kept_off, given, wipe=WIPE_GRID)
    _assert_records(found, found_want, f"{n_loci} loci")
    _assert_records(use, use_want, f"{n_loci} loci: the words in use")
    found, use = _find(ctx, 0, sq, packed, kept_off, None, wipe=WIPE_GRID)
    _assert_records(found, found_want, f"{n_loci} loci, no given word")
    _assert_records(use, found_want["word"], f"{n_loci} loci, no given word: the words in use")


def test_motif_runs_past_the_grid_cap(ctx):
    sq, packed, kept_off, words, want = sg.big_motif_case()
    _assert_records(_runs(ctx, 0, sq, packed, kept_off, words, wipe=WIPE_GRID), want, f"{len(sq)} records")


def test_seq_windows_past_the_grid_cap(ctx):
    batch, l_seq, want_q, want_n, _table = sg.big_window_case()
    q, n = _windows(ctx, 0, batch, l_seq, wipe=WIPE_GRID)
    _assert_records(q, want_q, f"{batch.n_pairs} pairs: q_beg")
    _assert_records(n, want_n, f"{batch.n_pairs} pairs: n_bases")


# ---- the compaction's scan --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unphased", [False, True])
@pytest.mark.parametrize("name", sg.SCAN_CASES)
def test_read_call_scan_past_256_tiles(ctx, orc, name, unphased):
    """kept_off and the records of the host entry and of the device entry against the oracle's, the second step's tiles among them"""
    batch, want, exp_off, exp_rec = sg.scan_expected(orc, name, unphased)
    assert batch.n_pairs >= sg.SCAN_STEP * int(ctx._L.inq_read_call_tile())
    _check_both_entries(ctx, batch, want, exp_off, exp_rec, f"{name} unphased={unphased}")


def test_flush_with_sequences_past_2_20_kept_pairs(ctx, tmp_path):
    """kept_pair[k] for k >= 2^20: every kept record's slice, packed bytes, origin and name against the written reads - the expectation is
    computed per distinct (CIGAR, pos) and locus and gathered (side_geometry_case.kept_pair_expected) -, every pair's slice at span time,
    and the motif runs of the records behind 2^20 and of the first thousand"""
    reads, loci = sg.kept_pair_reads(), sg.kept_pair_loci()
    bam = _write(tmp_path / "pairs.bam", reads, block=bamio.BLOCK)
    spans = _spans(bam, _bed(tmp_path / "pairs.bed", loci), True)
    assert len(spans) == 1 and [r[0] for r in span_records(spans[0])] == [r[0].encode() for r in reads], "pair_read indexes the reads as written"
    ctx.call_discard()
    codes, sizes = _append(ctx, spans, True)
    n_loci = ctx.deferred_loci
    assert codes == [0] and n_loci == sg.PAIR_LOCI and sizes["n_pairs"] == sg.PAIR_READS * sg.PAIR_LOCI
    cag = hipcall.encode_motif("CAG")
    rc, _p1, _p2, _ties, _ms, _fl, _ev, off, rec, org, raw, name_total, sq, packed, seq_total, mt = ctx.call_flush_motifs(np.full(n_loci, cag, dtype=np.uint64))
    assert rc == 0
    _cigar, _reads, pair_read, pair_off = ctx.span_fetch_batch(_Sizes(sizes), n_loci)
    q, n, kept, want_off = sg.kept_pair_expected(pair_read, pair_off, spans[0]["locus_start"], spans[0]["locus_end"])
    n_kept = int(want_off[-1])
    assert n_kept == 4091 * sg.PAIR_LOCI > sg.FIRST_STEP and np.array_equal(off, want_off)
    kept_pairs = np.nonzero(kept)[0]
    read = pair_read[kept_pairs].astype(np.int64)
    assert len(rec) == len(sq) == len(org) == len(mt) == n_kept
    _assert_records(rec["read"], pair_read[kept_pairs], "the records' reads")
    want_sq = np.zeros(n_kept, dtype=hipcall.SEQ_DTYPE)
    want_sq["q_beg"], want_sq["n_bases"] = q[kept_pairs], n[kept_pairs]
    _assert_records(sq[sg.FIRST_STEP :], want_sq[sg.FIRST_STEP :], "slices behind record 2^20")
    _assert_records(sq, want_sq, "slices")
    want_packed = sg.packed_slices(read, q[kept_pairs], n[kept_pairs])
    behind = int(((want_sq["n_bases"][: sg.FIRST_STEP].astype(np.int64) + 1) // 2).sum())  # where record 2^20's bytes begin
    assert seq_total == len(packed) == len(want_packed) > behind
    _assert_records(packed[behind:], want_packed[behind:], "packed bytes behind record 2^20")
    _assert_records(packed, want_packed, "packed bytes")
    want_raw, lens = sg.names_of(read)
    assert np.array_equal(org["name_len"], lens) and np.array_equal(org["pos"], np.array([r[2] for r in reads])[read])
    assert name_total == len(raw) == len(want_raw)
    _assert_records(raw, want_raw, "names")
    # span time: every pair
    q_all, n_all, seq_off, all_packed = ctx.span_fetch_seqs(len(pair_read), int(((n.astype(np.int64) + 1) // 2).sum()))
    _assert_records(q_all, q, "q_beg of every pair")
    _assert_records(n_all, n, "n_bases of every pair")
    _assert_records(all_packed, sg.packed_slices(pair_read, q, n), "packed bytes of every pair")
    # the motif runs: the records the scan's second step placed, and the first thousand
    for sel in (np.arange(sg.FIRST_STEP, n_kept), np.arange(1000)):
        slices = [reads[int(read[k])][6][int(want_sq["q_beg"][k]) : int(want_sq["q_beg"][k]) + int(want_sq["n_bases"][k])] for k in sel]
        _assert_records(mt[sel], rm.records_of(slices, [cag] * len(sel)), "motif runs")
    ctx.call_discard()
