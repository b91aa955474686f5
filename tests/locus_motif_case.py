"""What the locus-motifs tests share (no test lives here): the contract of inq_locus_motif_t restated by its definition in plain numpy
and Python - shifted-array equality for the lag counts, a dictionary of p-mers, `min` over rotations; independent of the host library's
base-by-base walk and of the kernel's words -, the contract's known answers, and the locus-motifs file's text restated on the records a
BAM was written from.  Builds on tests/read_motif_case.py."""
import numpy as np

from inquistr_amd import hipcall
from tests import read_motif_case as rm
from tests import read_seq_case as rs
from tests.test_tie_report import row_order

LOCUS_MOTIFS_HEADER = "chrom\tbegin\tend\treads\tbases\tmotif\tperiod\ttandem\tcopies\tcatalogue\tagrees"
MAX_PERIOD = 6
LETTER = {1: "A", 2: "C", 4: "G", 8: "T"}

# (slice, T_1 .. T_6 or None, p, motif or None, copies): the contract's hand-derived answers
KNOWN = [
    ("CAGCAGCAGCAG", (0, 0, 9, 0, 0, 6), 3, "AGC", 7),
    ("TTCAGCAGCAACAGCAGTT", (3, 1, 10, 1, 1, 7), 3, "AGC", 4),
    ("AAAA", (3, 2, 1, 0, 0, 0), 1, "A", 3),
    ("ACGT", (0, 0, 0, 0, 0, 0), 0, None, 0),
    ("CACACAGAGAG", (0, 8, 0, 5, 0, 2), 2, "AC", 3),  # AC and AG both count 3: the class tie
    # lag hits without a full copy.  The N moves the second CAG to lag 4 (i = 4, 5, 6 equal i - 4), so by the definition the period is
    # 4, not the 3 the feature request's table has for this slice; i + 8 <= 7 holds for no i
    ("CAGNCAG", (0, 0, 0, 3, 0, 0), 4, None, 0),
]


def lag_counts(slices):
    """[T_1 .. T_6] over the slices (arrays of 4-bit codes)"""
    t = [0] * MAX_PERIOD
    for s in slices:
        s = np.asarray(s, dtype=np.int64)
        base = np.isin(s, (1, 2, 4, 8))
        for k in range(1, MAX_PERIOD + 1):
            if len(s) > k:
                t[k - 1] += int(((s[k:] == s[:-k]) & base[k:]).sum())
    return t


def class_counts(slices, p):
    """{smallest rotation: count} of the tandem copies at period p"""
    out = {}
    for s in slices:
        text = "".join(LETTER.get(int(c), "n") for c in s)
        for i in range(len(text) - 2 * p + 1):
            a = text[i : i + p]
            if "n" not in a and a == text[i + p : i + 2 * p]:
                least = min(a[r:] + a[:r] for r in range(p))
                out[least] = out.get(least, 0) + 1
    return out


def find(slices):
    """(word, period, bases, tandem, copies) of a locus whose kept records' slices are `slices`"""
    bases = sum(len(s) for s in slices)
    t = lag_counts(slices)
    if max(t) == 0:
        return 0, 0, bases, 0, 0
    p = 1 + t.index(max(t))
    classes = class_counts(slices, p)
    if not classes:
        return 0, p, bases, t[p - 1], 0
    win = min(classes, key=lambda c: (-classes[c], c))
    d = next(d for d in range(1, p + 1) if p % d == 0 and win[:d] * (p // d) == win)
    return rm.literal_word(win[:d]), p, bases, t[p - 1], classes[win]


def records_of(slices, kept_off):
    """LOCUS_MOTIF_DTYPE [n_loci]: locus j's records are slices[kept_off[j] : kept_off[j + 1]]"""
    out = np.zeros(len(kept_off) - 1, dtype=hipcall.LOCUS_MOTIF_DTYPE)
    for j in range(len(out)):
        out[j] = find(slices[int(kept_off[j]) : int(kept_off[j + 1])])
    return out


def word_ok(word):
    return rm.motif_of(int(word))[0] != 0


def words_in_use(given, found_words):
    """what the motif kernel is handed: the given word where it names a motif, else the found one"""
    if given is None:
        return np.array(found_words, dtype=np.uint64)
    return np.array([g if word_ok(g) else f for g, f in zip(given, found_words)], dtype=np.uint64)


def motif_text(word):
    _k, m = rm.motif_of(int(word))
    return "".join(rs.CODES[x] for x in m) or "."


def locus_line(chrom, start, end, reads, found, catalogue_word):
    word, period, bases, tandem, copies = (int(x) for x in found)
    motif, cat = motif_text(word), motif_text(catalogue_word)
    agrees = "." if cat == "." else str(int(motif != "." and len(motif) == len(cat) and cat in motif + motif))
    return f"{chrom}\t{start}\t{end}\t{reads}\t{bases}\t{motif}\t{period}\t{tandem}\t{copies}\t{cat}\t{agrees}\n"


def found_of(reads):
    """find() of every target; reads[i]: the target's kept reads as read_seq_case.file_seq_reads gives them (the slice's codes last)"""
    return [find([x[5] for x in kept]) for kept in reads]


def locus_motifs_text(loci, reads, catalogue_words, threads):
    found = found_of(reads)
    return LOCUS_MOTIFS_HEADER + "\n" + "".join(
        locus_line(loci[i][0], loci[i][1], loci[i][2], len(reads[i]), found[i], catalogue_words[i]) for i in row_order(loci, threads))
