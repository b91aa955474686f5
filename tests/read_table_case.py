"""What the read-table tests share (no test lives here): a `_make_case`-style BAM whose read names vary in length, the table restated in
plain Python on the records the BAM was written from, and the records of a span read back out of its inflated bytes."""
import random
import struct

from oracle import pyoracle as py
from tests import gen
from tests.test_host_frontend import REFS
from tests.test_read_calls_host import split_calls
from tests.test_tie_report import row_order
from tools import bamio

TABLE_HEADER = "chrom\tbegin\tend\tgroup\tcall\tkind\tread\tpos\tstrand\tmapq"


def read_name(k):
    return f"r{k}" + "x" * (k % 40)


def make_named_case(tmp_path, seed, n_loci=40, block=bamio.BLOCK):
    """tests.test_host_frontend._make_case with names of 2 to 45 bytes: (bam, bed, loci, records by tid); a record's name is r.tags["name"]"""
    rng = random.Random(seed)
    loci = []
    recs = {t: [] for t in range(len(REFS))}
    for _ in range(n_loci):
        t = rng.choice([0, 0, 1, 2, 3, 4])
        start = rng.randint(2000, REFS[t][1] - 4000)
        end = start + rng.randint(0, 250)
        loci.append((REFS[t][0], start, end, t))
        if t == 4:
            continue  # a contig with loci but no reads
        recs[t] += gen.random_locus_reads(rng, start, end, rng.choice([0, 2, 5, 9, 30]), long_every=7)
    # nested loci that keep the same reads, and a far-away pair on chr2
    loci += [("chr1", 100_000, 100_400, 0), ("chr1", 100_050, 100_060, 0), ("chr2", 10_000, 10_020, 1), ("chr2", 290_000, 290_030, 1)]
    for t, s, e in ((0, 100_000, 100_400), (1, 10_000, 10_020), (1, 290_000, 290_030)):
        recs[t] += gen.random_locus_reads(rng, s, e, 12, long_every=5)
    for t in (0, 1):  # background reads nowhere near a locus
        for _ in range(40):
            recs[t].append(py.Record(pos=rng.randint(0, REFS[t][1] - 2000), cigar=gen.random_cigar(rng, 9), mapq=60, hp=("C", rng.choice([1, 2]))))
    bam = str(tmp_path / f"named{seed}.sorted.bam")
    w = bamio.BamWriter(bam, REFS, block=block)
    k = 0
    for t in range(len(REFS)):
        recs[t].sort(key=lambda r: r.pos)  # stable: file order among equal positions = insertion order
        for r in recs[t]:
            tags = [("HP", r.hp[0], r.hp[1])] if r.hp else []
            if r.sa:
                tags.append(("SA", "Z", r.sa[1]))
            r.tid = t
            r.tags["name"] = read_name(k)
            w.add(r.tags["name"], r.flag, t, r.pos, r.mapq, r.cigar, tags, l_seq=rng.choice([0, 0, 7]))
            k += 1
    for _ in range(3):
        w.add(f"unplaced{k}", 4, -1, -1, 0, [], [], l_seq=4)
        k += 1
    w.close()
    rng.shuffle(loci)
    bed = str(tmp_path / f"named{seed}.bed")
    with open(bed, "w") as f:
        for c, s, e, _ in loci:
            f.write(f"{c}\t{s}\t{e}\n")
    return bam, bed, loci, recs


def file_reads(loci, recs, unphased, minlen):
    """tests.test_gpu_read_calls.file_calls extended by who each read is: per BED line the kept reads in file order as
    (kind, value, HP, name, pos, flag, mapq), and how many records fetch() yields"""
    out = []
    for _chrom, s, e, t in loci:
        se, ee = s - 10, e + 10
        fetched = py._fetch(recs[t], t, se, ee)
        kept = []
        for r in fetched:
            if unphased:
                if se < (r.pos & py.U32) or (py.reference_end(r) & py.U32) < ee or r.mapq <= 10:
                    continue
                phase = 0
            else:
                phase = py.get_phase(r)
                if phase is None or (se < (r.pos & py.U32) and (py.reference_end(r) & py.U32) < ee) or r.mapq <= 10:
                    continue
            kept.append(py.call_from_cigar(r, minlen, se, ee) + (phase, r.tags["name"], r.pos, r.flag, r.mapq))
        out.append((kept, len(fetched)))
    return out


def table_lines(chrom, start, end, kept, unphased):
    """the lines of one target: h1 in its list's order, then h2, then other"""
    text = ""
    for group, part in zip(("h1", "h2", "other"), split_calls(kept, unphased)):
        for kind, value, _hp, name, pos, flag, mapq in part:
            name = name.split("\0")[0] or "*"
            text += f"{chrom}\t{start}\t{end}\t{group}\t{value}\t{kind}\t{name}\t{pos + 1}\t{'-' if flag & 0x10 else '+'}\t{mapq}\n"
    return text


def table_text(loci, reads, unphased, threads):
    return TABLE_HEADER + "\n" + "".join(table_lines(loci[i][0], loci[i][1], loci[i][2], reads[i][0], unphased) for i in row_order(loci, threads))


def span_records(span):
    """The placed records of a span in the device front end's order - every anchor's chain up to its stop, until the first unplaced
    record - read out of the zlib-inflated bytes: [(name bytes without terminator, pos, mapq, flag)]"""
    u = bamio.inflate_span(span["comp"], span["blocks"])
    out = []
    for a, stop in zip(span["anchors"], span["anchor_stop"]):
        off, stop = int(a), int(stop) & ~(1 << 63)
        while off + 4 <= stop:
            (bs,) = struct.unpack_from("<I", u, off)
            if off + 4 + bs > stop:
                break  # the last record of a segment may be cut: it lies behind everything the segment's loci need
            tid, pos, l_rn, mapq, _bin, _n_cig, flag = struct.unpack_from("<iiBBHHH", u, off + 4)
            if tid < 0:
                return out
            out.append((bytes(u[off + 36 : off + 36 + max(l_rn, 1) - 1]), pos, mapq, flag))
            off += 4 + bs
    return out
