"""The bases behind each Call on the GPU (inq_read_seq_t; read_seqs.hip): the packed gather at span time
(inq_call_span_deferred_seqs + inq_span_fetch_seqs) and the kept records' slices at flush time (inq_call_flush_seqs), against the
records the BAM was written from and the Q(x) formula of tests/read_seq_case.py.  The files are built around the gather's own
dimensions: both parities of the first base and of the length, every destination alignment, slice lengths on and next to a word, the
eight lanes' step and a byte's two bases, one slice of tens of kilobases, SEQ that straddles BGZF blocks."""
import numpy as np
import pytest

from inquistr_amd import batch as B
from inquistr_amd import call, hipcall
from tests import gen
from tests import read_seq_case as rs
from tools import bamio

pytestmark = pytest.mark.gpu

LADDER = [0, 1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 257]
START, END = 5000, 5300  # the ladder's locus: 319 bases of window, [4990, 5309)
SE, EE = START - 10, END + 10


@pytest.fixture(scope="module")
def ctx():
    c = hipcall.Context(0)
    assert c.backend.startswith("hip:gfx950")
    yield c
    c.close()


def _spans(bam, bed, unphased, max_comp_bytes=0):
    sp = call.Spans(bam, region_file=bed, minlen=5, support=3, threads=2, unphased=unphased, max_comp_bytes=max_comp_bytes)
    spans = [{k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in s.items()} for s in sp.spans()]
    sp.close()
    return spans


def _append(c, spans, unphased, seqs=True, names=True, check=True):
    sizes = {"n_cigar_words": 0, "n_reads": 0, "n_pairs": 0}
    codes = []
    for k, s in enumerate(spans):
        with_seqs = seqs[k] if isinstance(seqs, (list, tuple)) else seqs
        rc, stats = c.call_span_deferred(s["comp"], s["blocks"], s["anchors"], s["anchor_stop"], s["locus_tid"], s["locus_start"], s["locus_end"],
                                         5, 3, unphased, names=names, seqs=with_seqs, check=check)
        codes.append(rc)
        if rc == 0:
            for key in sizes:
                sizes[key] += int(getattr(stats, key))
    return codes, sizes


def _cut(off, raw):
    raw = bytes(raw)
    return [raw[int(off[i]) : int(off[i + 1])] for i in range(len(off) - 1)]


class _Sizes:
    def __init__(self, sizes):
        self.n_cigar_words, self.n_reads, self.n_pairs = sizes["n_cigar_words"], sizes["n_reads"], sizes["n_pairs"]


def _run(c, bam, bed, unphased, max_comp_bytes=0, n_spans=None):
    """A file through the device front end with sequences.  Checks every pair's slice and every kept record's against the written
    records; returns what the flush gave and the per-pair slices."""
    spans = _spans(bam, bed, unphased, max_comp_bytes)
    if n_spans is not None:
        assert len(spans) >= n_spans, len(spans)
        spans = spans[:n_spans]
    c.call_discard()
    codes, sizes = _append(c, spans, unphased)
    assert codes == [0] * len(spans)
    n_loci = c.deferred_loci
    out = c.call_flush_seqs()
    rc, p1, p2, ties, _ms, flags, ev, off, rec, org, raw, name_total, sq, packed, seq_total = out
    assert rc == 0
    written = [r for s in spans for r in rs.span_seq_records(s)]
    assert len(written) == sizes["n_reads"]
    starts = np.concatenate([s["locus_start"] for s in spans])
    ends = np.concatenate([s["locus_end"] for s in spans])
    _cigar, _reads, pair_read, poff = c.span_fetch_batch(_Sizes(sizes), n_loci)
    # span time: every pair of the batch
    want = []  # per pair (q_beg, codes)
    for j in range(n_loci):
        for p in range(int(poff[j]), int(poff[j + 1])):
            words, pos, l_seq, codes_ = written[int(pair_read[p])]
            q, n = rs.window(words, pos, l_seq, int(starts[j]), int(ends[j]))
            want.append((q, codes_[q : q + n]))
    n_pairs = sizes["n_pairs"]
    assert len(want) == n_pairs
    total = sum((len(w[1]) + 1) // 2 for w in want)
    q_beg, n_bases, seq_off, all_packed = c.span_fetch_seqs(n_pairs, total)
    assert [int(x) for x in q_beg] == [w[0] for w in want]
    assert [int(x) for x in n_bases] == [len(w[1]) for w in want]
    assert seq_off[0] == 0 and np.array_equal(np.diff(seq_off.astype(np.int64)), (n_bases.astype(np.int64) + 1) // 2) and int(seq_off[-1]) == total
    got = _cut(seq_off, all_packed)
    for p in range(n_pairs):
        assert got[p] == rs.pack(want[p][1]), (p, want[p][0], len(want[p][1]), int(seq_off[p]) & 3)
    if total:
        assert c.span_fetch_seqs(n_pairs, total - 1, check=False)[0] == B.INQ_ERR_ARG  # room for one byte less is refused
    # flush time: each record's slice is that of the pair the Call came from
    assert sq.dtype == hipcall.SEQ_DTYPE and len(sq) == len(rec) == int(off[-1])
    assert seq_total == len(packed) == int(((sq["n_bases"].astype(np.int64) + 1) // 2).sum())
    rec_off = np.concatenate([[0], np.cumsum((sq["n_bases"].astype(np.int64) + 1) // 2)])
    kept = _cut(rec_off, packed)
    k = 0
    for j in range(n_loci):
        pairs = [p for p in range(int(poff[j]), int(poff[j + 1]))]
        # the records of locus j are its kept pairs in pair order: walk both lists together
        at = 0
        for kk in range(int(off[j]), int(off[j + 1])):
            while int(pair_read[pairs[at]]) != int(rec["read"][kk]) or (want[pairs[at]][0], len(want[pairs[at]][1])) != (int(sq["q_beg"][kk]), int(sq["n_bases"][kk])):
                at += 1
                assert at < len(pairs), (j, kk)
            assert kept[kk] == rs.pack(want[pairs[at]][1]), (j, kk)
            at += 1
            k += 1
    assert k == len(rec)
    return dict(spans=spans, sizes=sizes, n_loci=n_loci, flush=out, want=want, seq_off=seq_off, pair_read=pair_read, poff=poff)


def _write(path, reads, block=600):
    """reads: (name, flag, pos, mapq, cigar, tags, codes[, stored]) in file order, on chr1"""
    w = bamio.BamWriter(str(path), [("chr1", 1_000_000)], block=block)
    for name, flag, pos, mapq, cigar, tags, codes, *stored in reads:
        w.add_raw(rs.seq_record(name, flag, 0, pos, mapq, cigar, tags, codes, stored[0] if stored else None), 0, pos,
                  pos + (bamio.ref_span(cigar) or 1), flag)
    w.close()
    return str(path)


def _bed(path, loci):
    with open(path, "w") as f:
        for s, e in loci:
            f.write(f"chr1\t{s}\t{e}\n")
    return str(path)


def _qlen(cigar):
    return sum(n for o, n in cigar if o in "MIS=X")


def _ladder_reads():
    """Reads whose slice under (START, END) has every length of the ladder, from an even and from an odd first base; spanning reads that
    are kept; one soft clip of 20 000 bases inside the window; a CIGAR of 70 ops held in CG; SEQ `*` and one shorter than its CIGAR"""
    reads = []
    k = 0

    def add(pos, cigar, hp, l_seq=None, cg=False, mapq=60):
        nonlocal k
        codes = rs.seq_codes(k, _qlen(cigar) if l_seq is None else l_seq)
        tags = [("HP", "C", hp)]
        stored = None
        if cg:
            stored, tag = rs.cg_form(cigar, len(codes))
            tags.append(tag)
        reads.append((f"L{k}", 0x10 if k % 3 == 0 else 0, pos, mapq, cigar, tags, codes, stored))
        k += 1

    for rep in range(7):  # (seven rounds: the byte lengths in front of a slice walk its destination through every alignment)
        for i, length in enumerate(LADDER):
            a = (i + rep) % 2 + 2 * ((i + rep) % 3)  # q_beg: 0 .. 5, both parities
            if length:
                add(SE - a, [("M", a + length)], 1 + i % 2)
            else:
                add(SE - a, [("M", a), ("D", 400), ("M", 5)], 1 + i % 2)
    for a in (0, 1, 2, 3, 7):  # kept, phased and unphased: the whole window, 319 bases
        add(SE - a, [("M", a + 319 + 40)], 1 + a % 2)
        add(SE - a, [("M", a + 100), ("I", 36), ("M", 219 + 40)], 1 + a % 2)
    add(SE - 3, [("M", 3 + 319 + 40)], 1, l_seq=0)    # SEQ `*`
    add(SE - 3, [("M", 3 + 319 + 40)], 2, l_seq=150)  # ... and one that ends inside the window
    ops70 = [("M", 5), ("I", 2)] * 35
    add(SE - 20, ops70 + [("M", 400)], 1, cg=True)    # the stored op count (2) places SEQ, the swapped-in CIGAR the window
    add(SE + 5, [("S", 20_000), ("M", 400)], 2)       # kept when phased: the read starts inside the window, the clip is the Call
    reads.sort(key=lambda r: r[2])
    return reads


@pytest.mark.parametrize("unphased", [False, True])
def test_slice_ladder(ctx, tmp_path, unphased):
    reads = _ladder_reads()
    bam = _write(tmp_path / "ladder.bam", reads)
    bed = _bed(tmp_path / "ladder.bed", [(START, END)])
    got = _run(ctx, bam, bed, unphased)
    assert len(got["spans"]) == 1 and len(got["spans"][0]["blocks"]) > 20, "SEQ straddles block boundaries"
    want, seq_off = got["want"], got["seq_off"]
    lengths = sorted(set(len(w[1]) for w in want))
    assert set(LADDER) <= set(lengths) and 20_000 + (EE - 1 - SE - 5) in lengths and 319 + 36 in lengths
    # first-base parity x length parity x destination alignment: all sixteen were met by a slice of more than a word
    combos = {(w[0] & 1, len(w[1]) & 1, int(seq_off[p]) & 3) for p, w in enumerate(want) if len(w[1]) >= 7}
    assert len(combos) == 16, sorted(combos)
    rc, *_rest, sq, packed, seq_total = got["flush"]
    assert len(sq) >= 10 and seq_total > 0
    if not unphased:
        assert 20_000 + (EE - 1 - SE - 5) in [int(x) for x in sq["n_bases"]], "the Clip's slice holds the clip"


@pytest.mark.parametrize("seed,unphased,n_spans", [(81, False, 2), (82, True, 3)])
def test_spans_in_one_batch(ctx, tmp_path, seed, unphased, n_spans):
    bam, bed, _loci, _recs = rs.make_seq_case(tmp_path, seed, n_loci=40)
    got = _run(ctx, bam, bed, unphased, max_comp_bytes=8_000, n_spans=n_spans)
    spans, sizes = got["spans"], got["sizes"]
    rc, p1, p2, ties, _ms, flags, ev, off, rec, org, raw, name_total, sq, packed, seq_total = got["flush"]
    assert len(rec) > 0 and sizes["n_pairs"] > len(rec)
    # a flush without sequences offers none; the same batch through inq_call_flush_origins gives the same bytes of everything else
    codes, _ = _append(ctx, spans, unphased)
    assert codes == [0] * n_spans
    rc0, p1_0, p2_0, ties0, _ms, flags0, ev0, off0, rec0, org0, raw0, total0 = ctx.call_flush_origins()
    assert rc0 == 0 and ctx.read_seqs_fetch(1, 0, check=False)[0] == B.INQ_ERR_ARG
    assert gen.same_f64(p1, p1_0) and gen.same_f64(p2, p2_0) and ties == ties0 and np.array_equal(flags, flags0)
    assert ev.tobytes() == ev0.tobytes() and np.array_equal(off, off0) and rec.tobytes() == rec0.tobytes()
    assert org.tobytes() == org0.tobytes() and bytes(raw) == bytes(raw0) and name_total == total0
    # a batch appended without sequences has none to give - and stays
    codes, _ = _append(ctx, spans, unphased, seqs=False)
    assert codes == [0] * n_spans
    n = ctx.deferred_loci
    assert ctx.call_flush_seqs(check=False)[0] == B.INQ_ERR_ARG and ctx.deferred_loci == n
    assert ctx.call_flush_origins()[0] == 0
    # one record, or one byte, more than the flush has; a part of them is there for the asking
    codes, _ = _append(ctx, spans, unphased)
    out = ctx.call_flush_seqs()
    assert out[0] == 0 and out[-3].tobytes() == sq.tobytes() and bytes(out[-2]) == bytes(packed)
    assert ctx.read_seqs_fetch(len(sq) + 1, seq_total, check=False)[0] == B.INQ_ERR_ARG
    assert ctx.read_seqs_fetch(len(sq), seq_total + 1, check=False)[0] == B.INQ_ERR_ARG
    few, some = min(2, len(sq)), min(3, seq_total)
    rc2, sq2, raw2 = ctx.read_seqs_fetch(few, some, check=False)
    assert rc2 == 0 and sq2.tobytes() == sq[:few].tobytes() and bytes(raw2) == bytes(packed[:some])
    # all spans of a batch with sequences or all without: the offending append appends nothing
    for first in (True, False):
        ctx.call_discard()
        codes, _ = _append(ctx, spans[:2], unphased, seqs=[first, not first], check=False)
        assert codes == [0, B.INQ_ERR_ARG], first
        assert ctx.deferred_loci == len(spans[0]["locus_start"])
    ctx.call_discard()


@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_kept_pairs_across_tiles(ctx, tmp_path, n):
    """one locus of n kept reads (the compaction's tile is 4096 pairs) and a second one behind it: every record finds its pair"""
    reads = []
    for k in range(n):
        a = k % 7
        reads.append((f"t{k}", 0, SE - a, 60, [("M", a + 330)], [("HP", "C", 1 + k % 2)], rs.seq_codes(k, 40)))
    for k in range(3):
        reads.append((f"u{k}", 0, 19_990 - k, 60, [("M", 30), ("I", 4), ("M", 170)], [("HP", "C", 1)], rs.seq_codes(n + k, 204)))
    reads.sort(key=lambda r: r[2])
    bam = _write(tmp_path / "tiles.bam", reads, block=bamio.BLOCK)
    bed = _bed(tmp_path / "tiles.bed", [(START, END), (20_000, 20_050)])
    got = _run(ctx, bam, bed, True)
    sq = got["flush"][-3]
    assert got["sizes"]["n_pairs"] == n + 3 == len(sq)
    assert sorted(set(int(x) for x in sq["q_beg"][:n])) == list(range(7)) and (sq["n_bases"][:n] == 40 - sq["q_beg"][:n]).all()
    assert (sq["n_bases"][n:] == 69 + 4).all()


def test_no_kept_read(ctx, tmp_path):
    reads = [(f"w{k}", 0, SE - k, 5, [("M", k + 400)], [("HP", "C", 1)], rs.seq_codes(k, k + 400)) for k in range(9)]
    reads.sort(key=lambda r: r[2])
    bam = _write(tmp_path / "none.bam", reads)
    bed = _bed(tmp_path / "none.bed", [(START, END), (START + 20, END)])
    got = _run(ctx, bam, bed, True)
    rc, *_x, off, rec, org, raw, name_total, sq, packed, seq_total = got["flush"]
    assert got["sizes"]["n_pairs"] == 18 and int(off[-1]) == 0 and len(sq) == 0 and seq_total == 0 and name_total == 0
    assert all(len(w[1]) == 319 or len(w[1]) == 299 for w in got["want"])
    assert ctx.read_seqs_fetch(0, 0, check=False)[0] == 0
