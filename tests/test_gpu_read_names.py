"""The names and origins of the reads behind the per-read Calls on the GPU (inq_read_origin_t; read_names.hip): the two segmented byte
gathers - at span time out of the inflated bytes, at flush time for the kept records - against the records the BAM was written from.
The tests are built around lengths and boundaries: every name length from 0 to 254 that sits on or next to a word, a 16-byte, a
32-byte piece, names that straddle BGZF blocks, a name that ends four bytes in front of the inflated bytes' end, and record counts
around the copy kernel's workgroup and the scans' tile."""
import struct

import numpy as np
import pytest

from inquistr_amd import batch as B
from inquistr_amd import call, hipcall
from tests import gen
from tests.read_table_case import span_records
from tools import bamio

pytestmark = pytest.mark.gpu

ORG = hipcall.ORIGIN_DTYPE
LADDER = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 253, 254]
SCAN_TILE = 4096  # elements per tile of the exclusive scans that place the names


@pytest.fixture(scope="module")
def ctx():
    c = hipcall.Context(0)
    assert c.backend.startswith("hip:gfx950")
    yield c
    c.close()


def _name(length, k):
    """a name of `length` bytes that names its record: no two of a file are equal, no byte repeats with a short period"""
    return (f"n{k}_" + "".join(chr(33 + (7 * k + 3 * i) % 90) for i in range(length)))[:length] if length else ""


def _spans(bam, bed, unphased, max_comp_bytes=0):
    sp = call.Spans(bam, region_file=bed, minlen=5, support=3, threads=2, unphased=unphased, max_comp_bytes=max_comp_bytes)
    spans = [{k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in s.items()} for s in sp.spans()]
    sp.close()
    return spans


def _append(c, spans, unphased, names, check=True):
    """the spans into one deferred batch; (codes, sizes summed over the spans that went in)"""
    sizes = {"n_cigar_words": 0, "n_reads": 0, "n_pairs": 0}
    codes = []
    for s, with_names in zip(spans, names if isinstance(names, (list, tuple)) else [names] * len(spans)):
        rc, stats = c.call_span_deferred(s["comp"], s["blocks"], s["anchors"], s["anchor_stop"], s["locus_tid"], s["locus_start"], s["locus_end"],
                                         5, 3, unphased, names=with_names, check=check)
        codes.append(rc)
        if rc == 0:
            for k in sizes:
                sizes[k] += int(getattr(stats, k))
    return codes, sizes


def _cut(off, raw):
    raw = bytes(raw)
    return [raw[int(off[i]) : int(off[i + 1])] for i in range(len(off) - 1)]


def _names_of(origins, raw):
    """the kept records' names: back to back, record k's begins at the sum of name_len in front of it"""
    return _cut(np.concatenate([[0], np.cumsum(origins["name_len"].astype(np.int64))]), raw)


def _write(path, reads, refs=(("chr1", 100_000),), block=600):
    """reads: (name str | raw record bytes, flag, pos, mapq, cigar, tags, l_seq) in file order"""
    w = bamio.BamWriter(str(path), list(refs), block=block)
    for name, flag, pos, mapq, cigar, tags, l_seq in reads:
        if isinstance(name, bytes):
            w.add_raw(name, 0, pos, pos + bamio.ref_span(cigar), flag)
        else:
            w.add(name, flag, 0, pos, mapq, cigar, tags, l_seq)
    w.close()
    return str(path)


def _bed(path, loci):
    with open(path, "w") as f:
        for s, e in loci:
            f.write(f"chr1\t{s}\t{e}\n")
    return str(path)


def _flush_origins(c, bam, bed, unphased=True, max_comp_bytes=0):
    """a file through the device front end with names: (spans' records, kept_off, records, origins, names of the kept, rows, name_bytes)"""
    spans = _spans(bam, bed, unphased, max_comp_bytes)
    c.call_discard()
    codes, sizes = _append(c, spans, unphased, True)
    assert codes == [0] * len(spans)
    rc, p1, p2, _ties, _ms, _fl, ev, off, rec, org, raw, total = c.call_flush_origins()
    assert rc == 0
    written = [r for s in spans for r in span_records(s)]
    assert len(written) == sizes["n_reads"]
    name_off, all_names = c.span_fetch_names(sizes["n_reads"])
    assert _cut(name_off, all_names) == [r[0] for r in written], "the batch's names"
    assert org.dtype == ORG and len(org) == len(rec) == int(off[-1]) and total == len(raw) == int(org["name_len"].sum())
    return written, off, rec, org, _names_of(org, raw), (p1, p2, ev), total


def _check_origins(written, rec, org, names):
    """every origin and every name is that of the record the Call came from"""
    for k in range(len(rec)):
        name, pos, mapq, flag = written[int(rec["read"][k])]
        assert names[k] == name, (k, names[k], name)
        assert (int(org["pos"][k]), int(org["mapq"][k])) == (pos, mapq), k
        assert bool(org["bits"][k] & B.INQ_READ_REVERSE) == bool(flag & 0x10), k


# ---- 1. the length ladder at span time -----------------------------------------------------------------------------------------------
def test_length_ladder_at_span_time(ctx, tmp_path):
    """One contig, one span, BGZF blocks of 600 bytes: names of every length of the ladder in an order that mixes short and long, `*`, an
    empty name (l_read_name = 1) and a hand-encoded record with l_read_name = 0; the first and the last record of the span have a 1-op
    CIGAR, no SEQ and no aux, so their names end four bytes in front of the record's end - the last one's in front of the inflated bytes'."""
    order = LADDER[::2] + LADDER[1::2][::-1]  # 1, 3, 5, 8, 15, ... 253, 254, 129, ... 4, 2
    edge = [("M", 300)]
    reads = [(_name(9, 0), 0, 1000, 60, edge, [], 0)]
    for k, length in enumerate(order, start=1):
        reads.append((_name(length, k), 0x10 if k % 3 == 0 else 0, 1000 + 10 * k, 20 + k, [("M", 150), ("I", 7), ("M", 150)],
                      [("HP", "C", 1 + k % 2), ("NM", "i", k)], [0, 5, 8][k % 3]))
    k0 = len(reads)
    reads.append(("*", 0, 1000 + 10 * k0, 33, [("M", 300)], [], 3))
    reads.append(("", 0, 1010 + 10 * k0, 34, [("M", 300)], [("NM", "i", 1)], 0))
    core = struct.pack("<iiBBHHHIiii", 0, 1020 + 10 * k0, 0, 35, bamio.reg2bin(1020 + 10 * k0, 1320 + 10 * k0), 1, 0, 0, -1, -1, 0)
    body = core + struct.pack("<I", (300 << 4) | 0)  # l_read_name = 0: the CIGAR begins where the name would
    reads.append((struct.pack("<I", len(body)) + body, 0, 1020 + 10 * k0, 35, edge, [], 0))
    reads.append((_name(17, 99), 0x10, 1030 + 10 * k0, 36, edge, [], 0))
    bam = _write(tmp_path / "ladder.bam", reads)
    bed = _bed(tmp_path / "ladder.bed", [(1100, 1150)])
    spans = _spans(bam, bed, True)
    assert len(spans) == 1 and len(spans[0]["blocks"]) >= 5, "the names straddle block boundaries"
    written = span_records(spans[0])
    want = [(b"" if isinstance(r[0], bytes) else r[0].encode()) for r in reads]
    assert [w[0] for w in written] == want, "the span holds every record of the file, first to last"
    assert sorted(len(w) for w in want) == sorted(LADDER + [0, 0, 1, 9, 17])  # (the ladder; empty, l_read_name = 0, `*`, the two edges)
    ctx.call_discard()
    codes, sizes = _append(ctx, spans, True, True)
    assert codes == [0] and sizes["n_reads"] == len(reads)
    assert sizes["n_pairs"] < len(reads), "reads no locus is offered are named all the same"
    rc, *_rest = ctx.call_flush_origins()
    assert rc == 0
    name_off, raw = ctx.span_fetch_names(sizes["n_reads"])
    assert name_off.dtype == np.uint64 and name_off[0] == 0 and (np.diff(name_off.astype(np.int64)) >= 0).all()
    assert int(name_off[-1]) == sum(len(w) for w in want) == len(raw)
    assert _cut(name_off, raw) == want
    # room for one byte less than the names take is refused
    assert ctx.span_fetch_names(sizes["n_reads"], cap_bytes=len(raw) - 1, check=False)[0] == B.INQ_ERR_ARG


# ---- 2. two spans in one batch -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,unphased", [(41, False), (42, True)])
def test_two_spans_in_one_batch(ctx, tmp_path, seed, unphased):
    from tests.test_host_frontend import _make_case

    bam, bed, _loci, _recs = _make_case(tmp_path, seed, n_loci=40)
    spans = _spans(bam, bed, unphased, max_comp_bytes=8_000)[:2]
    assert len(spans) == 2
    ctx.call_discard()
    codes, sizes = _append(ctx, spans, unphased, False)
    assert codes == [0, 0]
    # a batch appended without names has no origins to give - and stays
    n = ctx.deferred_loci
    assert ctx.call_flush_origins(check=False)[0] == B.INQ_ERR_ARG and ctx.deferred_loci == n
    rc0, p1_0, p2_0, ties0, _ms, flags0, ev0, off0, rec0 = ctx.call_flush_reads()
    assert rc0 == 0
    assert ctx.read_origins_fetch(1, 0, check=False)[0] == B.INQ_ERR_ARG  # a flush without origins offers none
    codes, sizes = _append(ctx, spans, unphased, True)
    assert codes == [0, 0]
    rc, p1, p2, ties, _ms, flags, ev, off, rec, org, raw, total = ctx.call_flush_origins()
    assert rc == 0
    # the rows and every other side output are those of the flush without origins
    assert gen.same_f64(p1, p1_0) and gen.same_f64(p2, p2_0) and ties == ties0 and np.array_equal(flags, flags0)
    assert ev.tobytes() == ev0.tobytes() and np.array_equal(off, off0) and rec.tobytes() == rec0.tobytes()
    assert len(rec) > 0 and sizes["n_pairs"] > len(rec)

    class St:
        n_cigar_words, n_reads, n_pairs = sizes["n_cigar_words"], sizes["n_reads"], sizes["n_pairs"]

    _cigar, reads, _pair_read, _poff = ctx.span_fetch_batch(St, n)
    written = [r for s in spans for r in span_records(s)]
    assert len(written) == len(reads) and len(span_records(spans[0])) not in (0, len(written))
    name_off, all_raw = ctx.span_fetch_names(len(reads))
    all_names = _cut(name_off, all_raw)
    assert all_names == [w[0] for w in written], "the concatenation of the two spans' names"
    assert org.dtype == ORG and len(org) == len(rec) and total == len(raw) == int(org["name_len"].sum())
    r = rec["read"].astype(np.int64)
    assert np.array_equal(org["pos"], reads["pos"][r]) and np.array_equal(org["mapq"], reads["mapq"][r])
    assert np.array_equal(org["bits"], reads["bits"][r])
    assert _names_of(org, raw) == [all_names[i] for i in r]
    _check_origins(written, rec, org, _names_of(org, raw))
    # one origin, or one byte, more than the flush has
    assert ctx.read_origins_fetch(len(org) + 1, total, check=False)[0] == B.INQ_ERR_ARG
    assert ctx.read_origins_fetch(len(org), total + 1, check=False)[0] == B.INQ_ERR_ARG
    few, some = min(2, len(org)), min(3, total)  # ... and a part of them is there for the asking
    rc, org2, raw2 = ctx.read_origins_fetch(few, some, check=False)
    assert rc == 0 and org2.tobytes() == org[:few].tobytes() and bytes(raw2) == bytes(raw[:some])
    # all spans of a batch with names or all without: the offending append appends nothing
    for first in (True, False):
        ctx.call_discard()
        codes, _ = _append(ctx, spans[:1], unphased, first)
        n1 = ctx.deferred_loci
        codes2, _ = _append(ctx, spans[1:], unphased, not first, check=False)
        assert codes == [0] and codes2 == [B.INQ_ERR_ARG] and ctx.deferred_loci == n1 == len(spans[0]["locus_start"])
    ctx.call_discard()


# ---- 3. kept-side shapes ---------------------------------------------------------------------------------------------------------------
SPAN = [("M", 400)]


def _simple(k, pos, mapq=60, flag=0, length=None):
    return (_name(5 + 7 * k % 50 if length is None else length, k), flag, pos, mapq, SPAN, [], 0)


def test_no_read_kept_anywhere(ctx, tmp_path):
    bam = _write(tmp_path / "none.bam", [_simple(k, 900 + k, mapq=5) for k in range(6)])  # fetched by both loci, filtered by all
    bed = _bed(tmp_path / "none.bed", [(1000, 1020), (1100, 1130)])
    written, off, rec, org, names, (p1, p2, ev), total = _flush_origins(ctx, bam, bed)
    assert len(written) == 6 and list(off) == [0, 0, 0] and len(rec) == len(org) == 0 and total == 0 and names == []
    assert list(ev["n_fetched"]) == [6, 6] and np.isnan(p1).all()
    assert ctx.read_origins_fetch(0, 0, check=False)[0] == 0
    assert ctx.read_origins_fetch(1, 0, check=False)[0] == B.INQ_ERR_ARG
    table = tmp_path / "none.tsv"
    with open(tmp_path / "none.inq", "w") as f:
        call.genotype_repeats(bam, None, bed, 5, 3, 1, True, None, None, out=f, frontend="device", read_table=str(table))
    assert table.read_text() == "chrom\tbegin\tend\tgroup\tcall\tkind\tread\tpos\tstrand\tmapq\n"


def test_exactly_one_kept_read(ctx, tmp_path):
    reads = [_simple(0, 900, mapq=5), _simple(1, 905, flag=0x10, length=33), _simple(2, 1015)]  # filtered | kept | starts inside the window
    bam = _write(tmp_path / "one.bam", reads)
    written, off, rec, org, names, _rows, total = _flush_origins(ctx, bam, _bed(tmp_path / "one.bed", [(1000, 1020)]))
    assert list(off) == [0, 1] and list(rec["read"]) == [1] and names == [reads[1][0].encode()] and total == 33
    assert (int(org["pos"][0]), int(org["mapq"][0]), int(org["bits"][0]) & B.INQ_READ_REVERSE) == (905, 60, B.INQ_READ_REVERSE)


def test_three_nested_loci_keep_the_same_read(ctx, tmp_path):
    reads = [_simple(0, 900, length=21), _simple(1, 1004, length=6)]  # spans all three | starts inside the outer two
    bam = _write(tmp_path / "nested.bam", reads)
    written, off, rec, org, names, _rows, total = _flush_origins(ctx, bam, _bed(tmp_path / "nested.bed", [(1000, 1100), (1020, 1080), (1040, 1060)]))
    assert list(np.diff(off.astype(np.int64))) == [1, 2, 2]  # (the second read begins inside the outer locus's window)
    assert names.count(reads[0][0].encode()) == 3 and names.count(reads[1][0].encode()) == 2 and total == 3 * 21 + 2 * 6
    _check_origins(written, rec, org, names)


def test_a_locus_of_filtered_reads_between_two_with_kept_reads(ctx, tmp_path):
    reads = [_simple(k, 900 + k) for k in range(3)] + [_simple(10 + k, 2900 + k, mapq=5) for k in range(4)] + [_simple(20 + k, 4900 + k) for k in range(2)]
    bam = _write(tmp_path / "mid.bam", reads)
    written, off, rec, org, names, (_p1, _p2, ev), total = _flush_origins(ctx, bam, _bed(tmp_path / "mid.bed", [(1000, 1020), (3000, 3020), (5000, 5020)]))
    assert list(off) == [0, 3, 3, 5] and list(ev["n_fetched"]) == [3, 4, 2]
    assert names == [r[0].encode() for r in reads[:3] + reads[7:]]
    _check_origins(written, rec, org, names)


# ---- 4. the tile boundary --------------------------------------------------------------------------------------------------------------
def _tile_counts():
    T = int(hipcall.load().inq_read_name_tile())
    return [("T - 1", T - 1), ("T", T), ("T + 1", T + 1), ("2T + 1", 2 * T + 1),
            # beside the issue's four: the exclusive scans that place the names carry across tiles of 4 096 records
            ("scan tile - 1", SCAN_TILE - 1), ("scan tile + 1", SCAN_TILE + 1)]


@pytest.mark.parametrize("which", range(6), ids=["T-1", "T", "T+1", "2T+1", "scan_tile-1", "scan_tile+1"])
def test_tile_boundary(ctx, tmp_path, which):
    """One locus that keeps every read of the file, each with a name of its own, lengths mixed over 0 .. 254"""
    what, n = _tile_counts()[which]
    assert ctx.read_name_tile >= 8 and n > 0
    lengths = [(37 * k + 11 * (k % 7)) % 255 if k % 5 else [0, 1, 4, 254, 16][k // 5 % 5] for k in range(n)]
    reads = [(_name(length, k), 0x10 if k % 4 == 1 else 0, 900 + k % 90, 11 + k % 50, SPAN, [], 0) for k, length in enumerate(lengths)]
    reads.sort(key=lambda r: r[2])
    bam = _write(tmp_path / "tile.bam", reads, block=bamio.BLOCK if n > 1000 else 600)
    written, off, rec, org, names, _rows, total = _flush_origins(ctx, bam, _bed(tmp_path / "tile.bed", [(1000, 1020)]))
    assert list(off) == [0, n] and list(rec["read"]) == list(range(n)), what
    assert names == [r[0].encode() for r in reads], what
    assert total == sum(len(r[0]) for r in reads) == sum(lengths), what
    assert [(int(p), int(m)) for p, m in zip(org["pos"], org["mapq"])] == [(r[2], r[3]) for r in reads], what
    assert [bool(b & B.INQ_READ_REVERSE) for b in org["bits"]] == [bool(r[1] & 0x10) for r in reads], what


# ---- 5. one context, several calls -----------------------------------------------------------------------------------------------------
def test_one_context_several_calls(tmp_path):
    """With names, without, then with names on a larger input (the scratch grows), then small again: each call is right; after a call
    without names no origin is on offer."""
    small = [_simple(k, 900 + k) for k in range(5)]
    big = [_simple(k, 900 + k % 80, length=(91 * k) % 255) for k in range(700)]
    big.sort(key=lambda r: r[2])
    bam_s, bam_b = _write(tmp_path / "s.bam", small), _write(tmp_path / "b.bam", big)
    bed = _bed(tmp_path / "calls.bed", [(1000, 1020)])
    with hipcall.Context(0) as c:
        def with_names(bam, reads):
            written, off, rec, org, names, _rows, total = _flush_origins(c, bam, bed)
            assert list(off) == [0, len(reads)] and names == [r[0].encode() for r in reads] and total == sum(len(r[0]) for r in reads)
            _check_origins(written, rec, org, names)
            return len(org), total

        n, total = with_names(bam_s, small)
        assert c.read_origins_fetch(n + 1, total, check=False)[0] == B.INQ_ERR_ARG
        spans = _spans(bam_s, bed, True)
        c.call_discard()
        assert _append(c, spans, True, False)[0] == [0]
        rc, _p1, _p2, _t, _ms, _fl, _ev, off, rec = c.call_flush_reads()
        assert rc == 0 and list(off) == [0, 5]
        assert c.read_origins_fetch(1, 0, check=False)[0] == B.INQ_ERR_ARG
        assert c.read_origins_fetch(0, 0, check=False)[0] == 0
        with_names(bam_b, big)
        n, total = with_names(bam_s, small)
        assert c.read_origins_fetch(n, total + 1, check=False)[0] == B.INQ_ERR_ARG
