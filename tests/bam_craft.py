"""A byte-level writer for BAM records and spans no well-behaved writer emits: what tests/deflate_craft.py is to the
inflate kernel, for the device record scan (csrc/bam_scan.hip).

record()  one record from explicit fields; declared lengths may disagree with the bytes
span()    records -> the arrays inq_call_span takes (no file, no index), as the dict tests.test_host_spans.emulate_span reads
to_bam()  the records of a BAM-expressible case as a sorted file with a .bai, through BamWriter.add_raw
verdict() what the scan must report for a span that is not clean, restated from the comments of csrc/front_kernels.h
"""
from __future__ import annotations

import struct
import zlib
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

from inquistr_amd import batch as B
from inquistr_amd import hipcall
from oracle import pyoracle as py
from tools import bamio

SEG_END = hipcall.ANCHOR_SEGMENT_END
OPS = "MIDNSHP=X"
# csrc/front_kernels.h
FS_CHAIN, FS_RECORD, FS_UNSORTED, FS_HP_TYPE, FS_SA_TYPE, FS_SA_FORMAT = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
NO_RECORD = (1 << 64) - 1  # first_bad_record of a span no record of which raised a bit


def op(code, n: int) -> int:
    """One CIGAR word; code: an op character or any number 0-15."""
    return (n << 4) | (OPS.index(code) if isinstance(code, str) else code)


def words(cigar) -> List[int]:
    return [w if isinstance(w, int) else op(*w) for w in cigar]


def record(tid: int = 0, pos: int = 0, name: bytes = b"r", mapq: int = 60, flag: int = 0, cigar: Sequence = (), l_seq: int = 0,
           tags: Sequence[Tuple[str, str, object]] = (), aux: bytes = b"", l_read_name: Optional[int] = None,
           n_cigar: Optional[int] = None, l_seq_declared: Optional[int] = None, block_size_override: Optional[int] = None) -> bytes:
    """block_size + one record.  name: the bytes between the fixed fields and the CIGAR as they stand (a terminator is the
    caller's business), l_read_name their count unless declared otherwise; cigar: raw words or (op, length) pairs; l_seq: the
    bases actually written ('*' nibbles, 0xff qualities); tags go through bamio.encode_aux in front of the raw `aux` bytes."""
    w = words(cigar)
    body = struct.pack("<iiBBHHHIiii", tid, pos, len(name) if l_read_name is None else l_read_name, mapq, 0,
                       len(w) if n_cigar is None else n_cigar, flag, l_seq if l_seq_declared is None else l_seq_declared, -1, -1, 0)
    body += name + struct.pack("<%dI" % len(w), *w) + b"\0" * ((l_seq + 1) // 2) + b"\xff" * l_seq + bamio.encode_aux(tags) + aux
    return struct.pack("<I", len(body) if block_size_override is None else block_size_override) + body


def _deflate(data: bytes, level: int) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def block_table(u: bytes, cuts: Iterable[int] = (), level: int = 1, block: int = bamio.BLOCK):
    """The inflated bytes cut into BGZF payloads at `cuts` (any offsets: the middle of a block_size word is one) and wherever a
    piece would pass `block` bytes; (compressed buffer, block table), the table as test_gpu_inflate_crafted._table builds it."""
    edges = sorted({0, len(u)} | {c for c in cuts if 0 < c < len(u)})
    comp, rows = bytearray(), []
    for lo, hi in zip(edges, edges[1:]):
        for o in range(lo, hi, block):
            piece = u[o : min(o + block, hi)]
            payload = _deflate(piece, level)
            rows.append((len(comp), len(payload), len(piece), o))
            comp += payload + struct.pack("<II", zlib.crc32(piece), len(piece))
    return bytes(comp), np.array(rows, dtype=hipcall.BGZF_BLOCK_DTYPE)


def span(segments, loci, anchors="every", cuts: Iterable[int] = (), minlen: int = 5, support: int = 3, unphased: bool = False,
         level: int = 1, anchor_at_end: bool = False, segment_end: Optional[Sequence[bool]] = None) -> dict:
    """segments: lists of record() bytes; a segment may end with a cut record given as ("cut", bytes), which gets no anchor.
    anchors: "every" record start, every k-th (an int) or "segment" (one per segment); anchor_stop is the next anchor, or the
    segment's end with SEG_END - unless segment_end says False for it, then the bare end (a chain that must land there).
    anchor_at_end: one more anchor at the very end of the last segment, equal to its stop.
    loci: (tid, start, end).  Besides the keys emulate_span reads: "u" (inflated bytes) and "rec_start" (all record starts)."""
    u, a_list, s_list, starts = bytearray(), [], [], []
    for k, seg in enumerate(segments):
        mine = []
        for r in seg:
            if isinstance(r, tuple):
                u += r[1]
            else:
                mine.append(len(u))
                u += r
        end = len(u)
        pick = mine if anchors == "every" else mine[:1] if anchors == "segment" else mine[:: int(anchors)]
        if anchor_at_end and k == len(segments) - 1:
            pick = pick + [end]
        flag = SEG_END if segment_end is None or segment_end[k] else 0
        a_list += pick
        s_list += pick[1:] + [end | flag]
        starts += mine
    comp, blocks = block_table(bytes(u), cuts, level)
    return dict(comp=comp, blocks=blocks, anchors=np.array(a_list, dtype=np.uint64), anchor_stop=np.array(s_list, dtype=np.uint64),
                locus_tid=np.array([l[0] for l in loci], dtype=np.int32), locus_start=np.array([l[1] for l in loci], dtype=np.uint32),
                locus_end=np.array([l[2] for l in loci], dtype=np.uint32), minlen=minlen, support=support, unphased=unphased,
                u=bytes(u), rec_start=starts)


def call_args(sp: dict):
    """The positional arguments of Context.call_span / call_span_deferred."""
    return (sp["comp"], sp["blocks"], sp["anchors"], sp["anchor_stop"], sp["locus_tid"], sp["locus_start"], sp["locus_end"],
            sp["minlen"], sp["support"], sp["unphased"])


def fields(rec: bytes) -> dict:
    """The declared fields of one record() (block_size first)."""
    bs, tid, pos, l_rn, mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<IiiBBHHHI", rec, 0)
    return dict(block_size=bs, tid=tid, pos=pos, l_read_name=l_rn, mapq=mapq, n_cigar=n_cig, flag=flag, l_seq=l_seq)


def to_bam(path: str, records: Sequence[bytes], refs: Sequence[Tuple[str, int]]) -> None:
    """The records (placed, sorted, each one whole) as a BAM with its .bai; the index only needs where each one lies."""
    w = bamio.BamWriter(path, refs)
    parsed = list(bamio.read_records(b"".join(records), 0))
    assert len(parsed) == len(records)
    for raw, r in zip(records, parsed):
        ops = [("MIDNSHP=X???????"[x & 15], x >> 4) for x in r["cigar"]]
        end = py.reference_end(py.Record(pos=r["pos"], cigar=ops, flag=r["flag"]))
        w.add_raw(raw, r["tid"], r["pos"], end, r["flag"])
    w.close()


# ---------------------------------------------------------------- the verdict on a span that is not clean
def _chain(u: bytes, x: int, stop: int, seg_end: bool):
    """chain rule of front_kernels.h (FS_CHAIN): a chain lands on the next anchor exactly, or ends at its segment's end where
    the last record may be cut; no record is shorter than its fixed part.  -> (record starts, ok)"""
    out = []
    if x > stop or stop > len(u):
        return out, False
    while x < stop:
        if x + 4 > stop:
            break
        (bs,) = struct.unpack_from("<I", u, x)
        if bs < 32:
            return out, False
        if x + 4 + bs > stop:
            break
        out.append(x)
        x += 4 + bs
    return out, seg_end or x == stop


def verdict(sp: dict):
    """(FS_* bits, smallest offending record index, INQ_ERR_* code) the scan must report for the span, (0, NO_RECORD, 0) for a
    clean one.  The stages stop where span.hip's front_fail stops them: a broken chain hides the records, a record or order
    fault hides the aux faults, which only the reads offered to a locus raise (src/call.rs:288-358: get_phase runs for every
    fetched record in phased mode; is_accidental_2d's panics are the locus kernel's business, not this verdict's)."""
    u = sp["u"] if "u" in sp else bamio.inflate_span(sp["comp"], sp["blocks"])
    starts, ok = [], True
    for a, st in zip(sp["anchors"], sp["anchor_stop"]):
        s, good = _chain(u, int(a), int(st) & ~SEG_END, bool(int(st) & SEG_END))
        starts += s
        ok &= good
    if not ok:
        return FS_CHAIN, 0, B.INQ_ERR_BAM
    bits, first = 0, NO_RECORD
    recs, prev = [], None
    for i, x in enumerate(starts):
        bs, tid, pos, l_rn, _mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<IiiBBHHHI", u, x)
        if tid < 0:  # unplaced records close the file: nothing is checked on them
            recs.append(None)
            prev = (tid, pos)
            continue
        bad = 0
        if 32 + l_rn + 4 * n_cig + (l_seq + 1) // 2 + l_seq > bs:
            bad |= FS_RECORD  # (such a record is not looked at any further)
        elif prev is not None and (prev[0] < 0 or (prev[0], prev[1] + 1 & 0xFFFFFFFF) > (tid, pos + 1 & 0xFFFFFFFF) or pos < -1):
            bad |= FS_UNSORTED
        if bad:
            bits |= bad
            first = min(first, i)
        recs.append((tid, pos))
        prev = (tid, pos)
    if bits:
        return bits, first, B.INQ_ERR_BAM
    if not sp["unphased"]:  # FS_HP_TYPE: the HP of a read offered to a locus is neither C nor i
        reads = [r for r in (next(bamio.read_records(u[: x + 4 + struct.unpack_from("<I", u, x)[0]], x)) for x in starts) if r["tid"] >= 0]
        for i, r in enumerate(reads):
            if r["hp"] is None or r["hp"][0] in "Ci":
                continue
            ops = [("MIDNSHP=X???????"[w & 15], w >> 4) for w in r["cigar"]]
            end = py.reference_end(py.Record(pos=r["pos"], cigar=ops, flag=r["flag"]))
            if any(int(t) == r["tid"] and r["pos"] < int(e) + 10 and end > int(s) - 10
                   for t, s, e in zip(sp["locus_tid"], sp["locus_start"], sp["locus_end"])):
                bits |= FS_HP_TYPE
                first = min(first, i)
    return (bits, first, B.INQ_ERR_AUX) if bits else (0, NO_RECORD, 0)


# ---------------------------------------------------------------- spans of millions of records, built and restated with numpy
STANZA = 8
LONG_RECORD, LONG_M = 5, 300_000  # record 5 of a stanza span: its first op is one long M


def _stanza():
    """Eight records: record k has k CIGAR ops (3M 7I 3M ...), a name of k bytes (l_read_name k, no terminator) and, when k is
    odd, HP:C:1 or 2."""
    recs = []
    for k in range(STANZA):
        cig = [("M", 3) if j % 2 == 0 else ("I", 7) for j in range(k)]
        recs.append(record(tid=0, pos=0, name=b"abcdefg"[:k], mapq=20 + k, cigar=cig, tags=[("HP", "C", 1 + (k >> 1) % 2)] if k % 2 else ()))
    return recs


def stanza_span(n: int, loci, anchors=1, minlen: int = 5, support: int = 3, unphased: bool = True) -> dict:
    """n records of the stanza back to back, record i at position i // 4, anchors at every `anchors`-th record; one segment."""
    recs = _stanza()
    size = np.array([len(r) for r in recs], dtype=np.int64)
    one = np.frombuffer(b"".join(recs), dtype=np.uint8)
    reps = (n + STANZA - 1) // STANZA
    start = (np.arange(reps, dtype=np.int64)[:, None] * len(one) + np.concatenate([[0], np.cumsum(size)[:-1]])[None, :]).ravel()[:n]
    total = int(start[-1] + size[(n - 1) % STANZA])
    u = np.tile(one, reps)[:total].copy()
    pos = (np.arange(n, dtype=np.int64) // 4).astype("<i4")
    u[(start + 8)[:, None] + np.arange(4)[None, :]] = pos.view(np.uint8).reshape(n, 4)
    if n > LONG_RECORD:
        at = int(start[LONG_RECORD]) + 36 + LONG_RECORD
        u[at : at + 4] = np.frombuffer(struct.pack("<I", op("M", LONG_M)), dtype=np.uint8)
    ub = u.tobytes()
    comp, blocks = block_table(ub)
    a = start[::anchors].astype(np.uint64)
    stop = np.concatenate([a[1:], np.array([total | SEG_END], dtype=np.uint64)])
    return dict(comp=comp, blocks=blocks, anchors=a, anchor_stop=stop,
                locus_tid=np.zeros(len(loci), dtype=np.int32), locus_start=np.array([l[0] for l in loci], dtype=np.uint32),
                locus_end=np.array([l[1] for l in loci], dtype=np.uint32), minlen=minlen, support=support, unphased=unphased,
                u=ub, n_records=n)


def stanza_expect(sp: dict):
    """The batch of a stanza_span, from the stanza's own numbers: cumulative sums for cigar_off4 and the name offsets, searchsorted
    for the lists.  -> (Batch with promise set, name_off [n + 1], names bytes)"""
    n = sp["n_records"]
    k = np.arange(n, dtype=np.int64) % STANZA
    units = (k + 3) // 4
    off4 = np.concatenate([[0], np.cumsum(units)])
    reads = np.zeros(n, dtype=B.READ_DTYPE)
    reads["cigar_off4"], reads["n_cigar"], reads["pos"], reads["mapq"] = off4[:-1], k, np.arange(n) // 4, 20 + k
    reads["bits"] = np.where(k % 2 == 1, B.INQ_READ_HAS_HP, 0)
    reads["phase"] = np.where(k % 2 == 1, 1 + (k >> 1) % 2, 0)
    reads["promise"] = B.INQ_READ_CHECKED
    cigar = np.zeros(int(off4[-1]) * 4, dtype=np.uint32)
    for j in range(STANZA - 1):
        sel = np.flatnonzero(k > j)
        cigar[off4[sel] * 4 + j] = op("M", 3) if j % 2 == 0 else op("I", 7)
    rlen = np.maximum(3 * ((k + 1) // 2), 1)
    if n > LONG_RECORD:
        cigar[int(off4[LONG_RECORD]) * 4] = op("M", LONG_M)
        rlen[LONG_RECORD] = LONG_M + 6
    pos = np.arange(n, dtype=np.int64) // 4
    end = pos + rlen
    short_max = 3 * 4
    lists, offs = [], [0]
    for s, e in zip(sp["locus_start"].astype(np.int64), sp["locus_end"].astype(np.int64)):
        lo = int(np.searchsorted(pos, s - 10 - short_max, "left"))
        hi = int(np.searchsorted(pos, e + 10, "left"))
        idx = np.arange(lo, hi)
        idx = idx[end[idx] > s - 10]
        if n > LONG_RECORD and LONG_RECORD < lo and LONG_RECORD < hi and end[LONG_RECORD] > s - 10:
            idx = np.concatenate([[LONG_RECORD], idx])
        lists.append(idx)
        offs.append(offs[-1] + len(idx))
    batch = B.Batch(cigar=cigar, reads=reads, pair_read=(np.concatenate(lists) if lists else np.zeros(0)).astype(np.uint32),
                    locus_pair_off=np.array(offs, dtype=np.uint64), locus_start=sp["locus_start"].copy(), locus_end=sp["locus_end"].copy(),
                    minlen=sp["minlen"], support=sp["support"], unphased=sp["unphased"])
    name_len = np.maximum(k, 1) - 1
    name_off = np.concatenate([[0], np.cumsum(name_len)]).astype(np.uint64)
    names = b"".join(b"abcdefg"[: max(x, 1) - 1] for x in range(STANZA))
    return batch, name_off, (names * (n // STANZA + 1))[: int(name_off[-1])]
