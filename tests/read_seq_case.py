"""What the read-seqs tests share (no test lives here): the slice contract of inq_read_seq_t restated from its Q(x) formula in plain
numpy - independent of the host library's sequential walk and of the kernel's scan -, BAM records with real SEQ bytes, the packed
slice and the file's text restated on the records a BAM was written from."""
import random
import struct

import numpy as np

from oracle import pyoracle as py
from tests import gen
from tests.test_host_frontend import REFS
from tests.test_read_calls_host import split_calls
from tests.test_tie_report import row_order
from tools import bamio

U32 = 0xFFFFFFFF
SEQS_HEADER = "chrom\tbegin\tend\tgroup\tcall\tkind\tread\tqbeg\tlen\tseq"
CODES = "=ACMGRSVTWYHKDBN"
OPS = "MIDNSHP=X"
M_OPS, IS_OPS, REF_OPS = (0, 7, 8), (1, 4), (0, 2, 3, 7, 8)


# locus counts at which the kernels' sixteen-probe search for "the j with off[j] <= x < off[j + 1]" takes 1, 2, 3 and 4 steps
# (n <= 16, <= 256, <= 4 096, above), on and next to each threshold
SEARCH_LOCUS_COUNTS = [1, 2, 15, 16, 17, 255, 256, 257, 4096, 4097]


def search_probe_loci(n):
    """The loci of n that a test of that search fills, every other one staying empty: the first, the last, and one on each side of every
    boundary between two probes of the first step (step = ceil(n / 16): the loci k step - 1, k step, k step + 1) and of the first and
    the last boundary of the second step inside the interval behind probe 7.  Ascending, at most 53"""
    step = -(-n // 16)
    want = {0, n - 1}
    for k in range(1, 16):
        want |= {k * step - 1, k * step, k * step + 1}
    lo2, step2 = 7 * step + 1, -(-step // 16)  # the second step's interval is [lo2, lo2 + step)
    for m in (1, 15):
        want |= {lo2 + m * step2 - 1, lo2 + m * step2, lo2 + m * step2 + 1}
    return sorted(j for j in want if 0 <= j < n)


def words_of(cigar):
    """[(op letter or code, len)] -> packed ops"""
    return np.array([(n << 4) | (OPS.index(o) if isinstance(o, str) else o) for o, n in cigar], dtype=np.uint32)


def Q(words, pos, x):
    """Q(x) of the contract: sum over I and S ops of len * [r_op < x] + sum over M, = and X ops of clamp(x - r_op, 0, len)"""
    op, ln = (np.asarray(words, dtype=np.int64) & 15), (np.asarray(words, dtype=np.int64) >> 4)
    r_op = pos + np.cumsum(np.where(np.isin(op, REF_OPS), ln, 0)) - np.where(np.isin(op, REF_OPS), ln, 0)
    m, i = np.isin(op, M_OPS), np.isin(op, IS_OPS)
    return int(ln[i][r_op[i] < x].sum() + np.clip(x - r_op[m], 0, ln[m]).sum())


def window(words, pos, l_seq, start, end):
    """(q_beg, n_bases) of one (locus, read) pair; l_seq None = no cut but the one to the 32 bits of the results"""
    se, ee = (start - 10) & U32, (end + 10) & U32
    if ee - 1 <= se:
        return 0, 0
    cut = lambda q: min(q, U32 if l_seq is None else l_seq)
    q_beg, q_end = cut(Q(words, pos, se)), cut(Q(words, pos, ee - 1))
    return q_beg, q_end - q_beg


def read_words(batch, r):
    o, n = int(batch.reads["cigar_off4"][r]), int(batch.reads["n_cigar"][r])
    return batch.cigar[4 * o : 4 * o + n]


def batch_windows(batch, l_seq=None):
    """(q_beg, n_bases) u32 [n_pairs] of a Batch by the formula; a (read, window) met before is not computed again"""
    q = np.zeros(batch.n_pairs, dtype=np.uint32)
    n = np.zeros(batch.n_pairs, dtype=np.uint32)
    seen = {}
    for j in range(batch.n_loci):
        s, e = int(batch.locus_start[j]), int(batch.locus_end[j])
        for p in range(int(batch.locus_pair_off[j]), int(batch.locus_pair_off[j + 1])):
            r = int(batch.pair_read[p])
            if (r, s, e) not in seen:
                if r >= batch.n_reads:
                    seen[(r, s, e)] = (0, 0)
                else:
                    seen[(r, s, e)] = window(read_words(batch, r), int(batch.reads["pos"][r]), None if l_seq is None else int(l_seq[r]), s, e)
            q[p], n[p] = seen[(r, s, e)]
    return q, n


def window_sums(words, pos, start, end):
    """(matched bases at reference coordinates [se, ee - 1), I + S bases of ops with se <= r_op <= ee - 2, D bases of such ops) by a
    walk base by base and op by op: what n_bases and the Call are made of"""
    se, ee = start - 10, end + 10
    r, matched, ins, dele = pos, 0, 0, 0
    for w in words:
        op, ln = int(w) & 15, int(w) >> 4
        if op in M_OPS:
            matched += max(0, min(r + ln, ee - 1) - max(r, se))
        elif op in IS_OPS and se <= r <= ee - 2:
            ins += ln
        elif op == 2 and se <= r <= ee - 2:
            dele += ln
        if op in REF_OPS:
            r += ln
    return matched, ins, dele


def seq_codes(k, l_seq):
    """the 4-bit codes of record k's SEQ: every code occurs, no two records of a file agree, no short period"""
    i = np.arange(l_seq, dtype=np.int64)
    return ((i * 7 + (i >> 4) * 3 + k * 5 + (i * i) % 11) % 16).astype(np.uint8)


def pack(codes):
    """4-bit codes two to a byte, the first in the high nibble, a last odd low nibble 0"""
    c = np.asarray(codes, dtype=np.uint8)
    if len(c) & 1:
        c = np.concatenate([c, np.zeros(1, np.uint8)])
    return ((c[0::2] << 4) | c[1::2]).astype(np.uint8).tobytes()


def text_of(codes):
    return "".join(CODES[int(c)] for c in codes)


def seq_record(name, flag, tid, pos, mapq, cigar, tags, codes, stored=None):
    """One BAM record WITH its block_size, for BamWriter.add_raw, whose SEQ is `codes` (QUAL 0xff).  cigar: [(op letter, len)], the
    read's real CIGAR; stored: the ops the record's CIGAR field holds when they differ (a long CIGAR in CG:B,I)."""
    words = [(n << 4) | OPS.index(o) for o, n in (cigar if stored is None else stored)]
    rn = name.encode("latin1") + b"\0"
    end = pos + (bamio.ref_span(cigar) or 1)
    core = struct.pack("<iiBBHHHIiii", tid, pos, len(rn), mapq, bamio.reg2bin(max(pos, 0), max(end, 1)), len(words), flag, len(codes), -1, -1, 0)
    body = core + rn + struct.pack("<%dI" % len(words), *words) + pack(codes) + b"\xff" * len(codes) + bamio.encode_aux(tags)
    return struct.pack("<I", len(body)) + body


def seq_lines(chrom, start, end, kept, unphased):
    """the lines of one target; kept: (kind, value, HP, name, q_beg, codes of the slice) in file order"""
    text = ""
    for group, part in zip(("h1", "h2", "other"), split_calls(kept, unphased)):
        for kind, value, _hp, name, q_beg, codes in part:
            name = name.split("\0")[0] or "*"
            text += f"{chrom}\t{start}\t{end}\t{group}\t{value}\t{kind}\t{name}\t{q_beg}\t{len(codes)}\t{text_of(codes) or '*'}\n"
    return text


def seqs_text(loci, reads, unphased, threads):
    return SEQS_HEADER + "\n" + "".join(seq_lines(loci[i][0], loci[i][1], loci[i][2], reads[i], unphased) for i in row_order(loci, threads))


def cg_form(cigar, l_seq):
    """(stored ops, tag) of a CIGAR kept in CG:B,I: the record's own field says `<l_seq>S<span>N`"""
    return [("S", l_seq), ("N", bamio.ref_span(cigar))], ("CG", "B", ("I", [(n << 4) | OPS.index(o) for o, n in cigar]))


def make_seq_case(tmp_path, seed, n_loci=24):
    """tests.test_host_frontend._make_case whose records carry real SEQ: (bam, bed, loci, records by tid); a record's name is
    r.tags["name"], its SEQ codes r.tags["seq"].  Some SEQ are `*`, some shorter than the CIGAR says, every eleventh CIGAR sits in CG."""
    rng = random.Random(seed)
    loci, recs = [], {t: [] for t in range(len(REFS))}
    for _ in range(n_loci):
        t = rng.choice([0, 0, 1, 2])
        start = rng.randint(2000, REFS[t][1] - 4000)
        end = start + rng.randint(0, 250)
        loci.append((REFS[t][0], start, end, t))
        recs[t] += gen.random_locus_reads(rng, start, end, rng.choice([0, 2, 5, 9, 20]), long_every=7)
    loci += [("chr1", 100_000, 100_400, 0), ("chr1", 100_050, 100_060, 0)]  # nested loci that keep the same reads
    recs[0] += gen.random_locus_reads(rng, 100_000, 100_400, 12, long_every=5)
    bam = str(tmp_path / f"seqs{seed}.sorted.bam")
    w = bamio.BamWriter(bam, REFS, block=rng.choice([600, bamio.BLOCK]))
    k = 0
    for t in range(len(REFS)):
        recs[t].sort(key=lambda r: r.pos)
        for r in recs[t]:
            qlen = sum(n for o, n in r.cigar if o in "MIS=X")
            l_seq = rng.choice([qlen, qlen, qlen, 0, max(0, qlen - 5)])
            tags = [("HP", r.hp[0], r.hp[1])] if r.hp else []
            if r.sa:
                tags.append(("SA", "Z", r.sa[1]))
            stored = None
            if k % 11 == 3 and r.cigar and not r.flag & 4:
                stored, cg = cg_form(r.cigar, l_seq)
                tags.append(cg)
            r.tid, r.tags["name"], r.tags["seq"] = t, f"q{k}" + "y" * (k % 9), seq_codes(k, l_seq)
            w.add_raw(seq_record(r.tags["name"], r.flag, t, r.pos, r.mapq, r.cigar, tags, r.tags["seq"], stored), t, r.pos,
                      r.pos + (bamio.ref_span(r.cigar) or 1), r.flag)
            k += 1
    w.close()
    rng.shuffle(loci)
    bed = str(tmp_path / f"seqs{seed}.bed")
    with open(bed, "w") as f:
        for c, s, e, _ in loci:
            f.write(f"{c}\t{s}\t{e}\n")
    return bam, bed, loci, recs


def file_seq_reads(loci, recs, unphased, minlen):
    """per BED line the kept reads in file order as (kind, value, HP, name, q_beg, codes of the slice), as tests.read_table_case.file_reads
    finds them"""
    out = []
    for _chrom, s, e, t in loci:
        se, ee = s - 10, e + 10
        kept = []
        for r in py._fetch(recs[t], t, se, ee):
            if unphased:
                if se < (r.pos & py.U32) or (py.reference_end(r) & py.U32) < ee or r.mapq <= 10:
                    continue
                phase = 0
            else:
                phase = py.get_phase(r)
                if phase is None or (se < (r.pos & py.U32) and (py.reference_end(r) & py.U32) < ee) or r.mapq <= 10:
                    continue
            q_beg, n = window(words_of(r.cigar), r.pos, len(r.tags["seq"]), s, e)
            kept.append(py.call_from_cigar(r, minlen, se, ee) + (phase, r.tags["name"], q_beg, r.tags["seq"][q_beg : q_beg + n]))
        out.append(kept)
    return out


def span_seq_records(span):
    """The placed records of a span in the device front end's order (tests.read_table_case.span_records), each as
    (CIGAR words with CG swapped in, pos, l_seq, SEQ codes)"""
    u = bamio.inflate_span(span["comp"], span["blocks"])
    out = []
    for a, stop in zip(span["anchors"], span["anchor_stop"]):
        off, stop = int(a), int(stop) & ~(1 << 63)
        while off + 4 <= stop:
            (bs,) = struct.unpack_from("<I", u, off)
            if off + 4 + bs > stop:
                break
            tid, pos, l_rn, _mapq, _bin, n_cig, _flag, l_seq = struct.unpack_from("<iiBBHHHI", u, off + 4)
            if tid < 0:
                return out
            rec = next(bamio.read_records(u[: off + 4 + bs], off))
            s0 = off + 36 + l_rn + 4 * n_cig
            raw = np.frombuffer(u[s0 : s0 + (l_seq + 1) // 2], dtype=np.uint8)
            codes = np.stack((raw >> 4, raw & 15), axis=1).reshape(-1)[:l_seq]
            out.append((np.array(rec["cigar"], dtype=np.uint32), pos, l_seq, codes))
            off += 4 + bs
    return out
