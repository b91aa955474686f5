"""What the read-motifs tests share (no test lives here): the run contract of inq_read_motif_t restated from its rotation definition in
plain numpy - independent of the host library's sequential walk and of the kernel's word steps -, the contract's known answers, BAM
records whose SEQ is built from their locus's motif, and the file's text restated on the records a BAM was written from."""
import random

import numpy as np

from inquistr_amd import hipcall
from tests import gen
from tests import read_seq_case as rs
from tests.test_host_frontend import REFS
from tests.test_read_calls_host import split_calls
from tests.test_tie_report import row_order
from tools import bamio

MOTIFS_HEADER = "chrom\tbegin\tend\tgroup\tcall\tkind\tread\tqbeg\tlen\tmotif\trun_beg\trun_len\tunits\tmotif_bases\truns"
CODE = {"A": 1, "C": 2, "G": 4, "T": 8}

# (slice, motif, run_beg, run_len, motif_bases, n_runs): the contract's hand-derived answers
KNOWN = [
    ("CAGCAGCAGCAG", "CAG", 0, 12, 12, 1),
    ("TTCAGCAGCAACAGCAGTT", "CAG", 2, 8, 14, 2),
    ("CAGCAGAGCAGCAG", "CAG", 6, 8, 14, 2),
    ("GCAGCAGC", "AGC", 0, 8, 8, 1),
    ("CAGNCAG", "CAG", 0, 3, 6, 2),
    ("CACACAGAGAG", "CA", 0, 6, 6, 1),
    ("ACGT", "CAG", 0, 1, 0, 0),
    ("CA", "CAG", 0, 2, 0, 0),
    ("TTTTT", "CAG", 0, 0, 0, 0),
    ("AAAA", "A", 0, 4, 4, 1),
    ("", "CAG", 0, 0, 0, 0),
    ("CAGCAGCAG", "CAGCAG", 0, 9, 9, 1),  # reduced to CAG by the encoder
]


def literal_word(text):
    """the motif word of `text` taken as it stands: no reduction to the primitive root (the device takes a word literally)"""
    return len(text) << 60 | sum(CODE[ch] << (4 * i) for i, ch in enumerate(text))


def codes_of(text):
    return np.array([rs.CODES.index(ch) for ch in text], dtype=np.uint8)


def motif_of(word):
    """(k, the k codes) of a motif word, (0, []) for a word that is no motif"""
    k = word >> 60
    m = [(word >> (4 * i)) & 15 for i in range(k)]
    return (k, m) if k and all(x in (1, 2, 4, 8) for x in m) else (0, [])


def motif_runs(codes, word):
    """(run_beg, run_len, motif_bases, n_runs) of a slice's codes by the definition: the hits of every rotation, their maximal runs"""
    codes = np.asarray(codes, dtype=np.int64)
    k, m = motif_of(int(word))
    n = len(codes)
    if not k or not n:
        return 0, 0, 0, 0
    runs = []
    for r in range(k):
        hit = codes == np.array(m)[(np.arange(n) + r) % k]
        edge = np.diff(np.concatenate([[0], hit.astype(np.int8), [0]]))
        runs += list(zip(np.flatnonzero(edge == 1).tolist(), np.flatnonzero(edge == -1).tolist()))
    if not runs:
        return 0, 0, 0, 0
    a, b = max(runs, key=lambda ab: (ab[1] - ab[0], -ab[0]))
    inside = np.zeros(n, dtype=bool)
    whole = [(a_, b_) for a_, b_ in runs if b_ - a_ >= k]
    for a_, b_ in whole:
        inside[a_:b_] = True
    return a, b - a, int(inside.sum()), len(whole)


def records_of(slices, words):
    """MOTIF_DTYPE records of slices[i] (codes) under words[i]"""
    out = np.zeros(len(slices), dtype=hipcall.MOTIF_DTYPE)
    for i, (c, w) in enumerate(zip(slices, words)):
        out[i] = motif_runs(c, w)
    return out


def seq_arrays(slices):
    """(SEQ_DTYPE records with q_beg 0, the packed bytes back to back) of slices, as inq_read_seqs_fetch returns them"""
    sq = np.zeros(len(slices), dtype=hipcall.SEQ_DTYPE)
    sq["n_bases"] = [len(c) for c in slices]
    packed = np.frombuffer(b"".join(rs.pack(c) for c in slices), dtype=np.uint8)
    return sq, packed


def repeat_codes(motif, n, phase=0):
    """n bases of the pure repeat of `motif` (text), beginning at its base `phase`"""
    m = [CODE[ch] for ch in motif]
    return np.array([m[(i + phase) % len(m)] for i in range(n)], dtype=np.uint8)


def noisy_repeat(rng, motif, n):
    """a repeat of `motif` with interruptions: substituted bases (any of the sixteen codes), dropped bases (phase shifts), flanks"""
    out, i = [], rng.randrange(len(motif))
    while len(out) < n:
        x = rng.random()
        if x < 0.04:
            out.append(rng.randrange(16))
        elif x < 0.06:
            i += 1  # a deletion inside the repeat
            continue
        elif x < 0.07:
            out += [rng.randrange(16) for _ in range(rng.randrange(1, 20))]
        else:
            out.append(CODE[motif[i % len(motif)]])
        i += 1
    return np.array(out[:n], dtype=np.uint8)


COLUMN4 = ["CAG", "cag", "A", "AAG", "CAGCAG", "GGCCCC", "CCCCGCCCCGCG", "ACGTACGTACGTAAA", ".", "GCN", "CAG,CCG", "TTTTTTTTTTTTTTTTG"]


def make_motif_case(tmp_path, seed, n_loci=24):
    """tests.read_seq_case.make_seq_case with a motif per locus: (bam, bed, loci, records by tid, column 4 by locus).  The BED has four
    columns, the fourth one of COLUMN4 (some do not encode); a record's SEQ is a noisy repeat of the motif of the locus it was made for
    (CAG where that does not encode).  Some SEQ are `*`, some shorter than the CIGAR says, every eleventh CIGAR sits in CG."""
    rng = random.Random(seed)
    loci, recs, col4 = [], {t: [] for t in range(len(REFS))}, []
    made = []  # (record, motif text) in the order made

    def add(t, start, end, depth, long_every):
        text = COLUMN4[len(loci) % len(COLUMN4)]
        loci.append((REFS[t][0], start, end, t))
        col4.append(text)
        new = gen.random_locus_reads(rng, start, end, depth, long_every=long_every)
        recs[t] += new
        made.extend((r, text.upper() if hipcall.encode_motif(text) else "CAG") for r in new)

    for _ in range(n_loci):
        t = rng.choice([0, 0, 1, 2])
        start = rng.randint(2000, REFS[t][1] - 4000)
        add(t, start, start + rng.randint(0, 250), rng.choice([0, 2, 5, 9, 20]), 7)
    add(0, 100_000, 100_400, 12, 5)
    loci.append(("chr1", 100_050, 100_060, 0))  # a nested locus that keeps the same reads, under another motif
    col4.append("AGC")
    motif_by_rec = {id(r): text for r, text in made}
    bam = str(tmp_path / f"motifs{seed}.sorted.bam")
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
                stored, cg = rs.cg_form(r.cigar, l_seq)
                tags.append(cg)
            r.tid, r.tags["name"], r.tags["seq"] = t, f"m{k}" + "y" * (k % 9), noisy_repeat(rng, motif_by_rec[id(r)], l_seq)
            w.add_raw(rs.seq_record(r.tags["name"], r.flag, t, r.pos, r.mapq, r.cigar, tags, r.tags["seq"], stored), t, r.pos,
                      r.pos + (bamio.ref_span(r.cigar) or 1), r.flag)
            k += 1
    w.close()
    order = list(range(len(loci)))
    rng.shuffle(order)
    loci, col4 = [loci[i] for i in order], [col4[i] for i in order]
    bed = str(tmp_path / f"motifs{seed}.bed")
    with open(bed, "w") as f:
        for (c, s, e, _), text in zip(loci, col4):
            f.write(f"{c}\t{s}\t{e}\t{text}\n")
    return bam, bed, loci, recs, col4


def motif_lines(chrom, start, end, kept, unphased, word):
    """the lines of one target; kept: (kind, value, HP, name, q_beg, codes of the slice) in file order (read_seq_case.file_seq_reads)"""
    k, m = motif_of(word)
    motif = "".join(rs.CODES[x] for x in m) or "."
    text = ""
    for group, part in zip(("h1", "h2", "other"), split_calls(kept, unphased)):
        for kind, value, _hp, name, q_beg, codes in part:
            name = name.split("\0")[0] or "*"
            beg, length, bases, runs = motif_runs(codes, word)
            tail = f"{beg}\t{length}\t{length // k}\t{bases}\t{runs}" if k else ".\t.\t.\t.\t."
            text += f"{chrom}\t{start}\t{end}\t{group}\t{value}\t{kind}\t{name}\t{q_beg}\t{len(codes)}\t{motif}\t{tail}\n"
    return text


def motifs_text(loci, reads, words, unphased, threads):
    return MOTIFS_HEADER + "\n" + "".join(
        motif_lines(loci[i][0], loci[i][1], loci[i][2], reads[i], unphased, words[i]) for i in row_order(loci, threads))
