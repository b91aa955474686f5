"""What the side-geometry tests share (no test lives here): inputs that make a side kernel's workgroups take more than one trip round
their grid-stride loop - under the context option "grid_side" at 1, 2, 3 and 7 workgroups, and at the launchers' own cap of 65 536 -
and that take the compaction's scan (read_call_scan of read_calls.hip) past its first step of 256 tiles.  Every expected output comes
from the restatements the kernels' own tests use: tests/locus_motif_case.py, read_motif_case.py, read_seq_case.py, and the C oracle
through the helpers of tests/test_gpu_read_calls.py.  tests/test_side_geometry_cases.py pins what each case claims, on the CPU."""
import random

import numpy as np

from inquistr_amd import batch as B
from inquistr_amd import hipcall
from tests import locus_motif_case as lm
from tests import read_motif_case as rm
from tests import read_seq_case as rs
from tests.test_gpu_read_calls import KEPT, _oracle, _pool, _tiled

# items a workgroup takes per trip (the library's constants, repeated: test_gpu_side_geometry.py holds them to the inq_*_tile entries)
READ_MOTIF_TILE = 16   # records of read_motif_kernel
SEQ_WINDOW_TILE = 16   # pairs of seq_window_kernel
READ_NAME_TILE = 32    # segments of name_copy_kernel
SEQ_SLICE_TILE = 32    # segments of seq_slice_kernel
RECORD_TILE = 256      # records of read_seq_record_kernel and read_origin_kernel: one per lane
READ_CALL_TILE = 4096  # pairs of the compaction's count and scatter launches; its scan takes 256 tiles a step
GRID_CAP = 1 << 16     # kGridCap: workgroups of a side launch at most; locus_motif_kernel takes one locus per workgroup and trip
SCAN_STEP = 256        # tiles per step of read_call_scan

CAPS = (1, 2, 3, 7)          # "grid_side" of the small-grid cases
GRID_SIDES = CAPS + (0,)     # ... and 0 last: each launcher's own cap
POOL = 499                   # distinct items of a real-cap case, repeated: GRID_CAP * k is no multiple of it
KINDS = "abcde"

_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---- loci of five kinds (locus_motif_kernel) -------------------------------------------------------------------------------------------
SIX_MERS = ["ACGTCG", "ATGCTC", "AGTCTG", "TCAGCA", "GATCTC"]  # primitive, no base beside its like: lag 6 has the most hits


def _draw_locus(rng, kind, max_bases, max_depth):
    if kind == "a":
        if max_depth == 1:  # one record: two copies each of two 6-mers
            one, two = rng.sample(SIX_MERS, 2)
            return [np.concatenate([rm.repeat_codes(one, max_bases // 2, rng.randrange(6)), rm.repeat_codes(two, max_bases // 2, rng.randrange(6))])]
        deep = [rm.noisy_repeat(rng, "GGCCCC", max_bases) for _ in range(rng.randint(3, max_depth))]
        return deep + [rm.repeat_codes(m, rng.randint(13, 20), rng.randrange(6)) for m in rng.sample(SIX_MERS, 2)]
    if kind == "b":
        motif = rng.choice(["A", "C", "G", "T", "CA", "GT", "AG", "CT", "AT", "CG"])
        return [rm.repeat_codes(motif, rng.randint(8, min(24, max_bases)), rng.randrange(2)) for _ in range(rng.randint(1, min(3, max_depth)))]
    if kind == "c":
        return [rm.codes_of(rng.choice(["CAGNCAG", "ACGTNACGT", "GATTNGATTN"]))]
    if kind == "d":
        return [rm.codes_of("ACGT") if rng.random() < 0.5 else np.full(rng.randint(1, 20), 15, dtype=np.uint8)]
    return []


def kind_of(slices, rec, min_classes=3):
    """the kind a locus's expected record (lm.find) puts it in, None where it is none of the five:
    a  period 6, at least min_classes rotation classes filled (a noisy GGCCCC several records deep beside two other 6-mers)
    b  period 1 or 2, a copy
    c  lag hits but no whole copy: period != 0, copies == 0
    d  bases, every lag count 0
    e  no record"""
    word, period, bases, tandem, copies = (int(x) for x in rec)
    if not slices:
        return "e" if (word, period, bases, tandem, copies) == (0, 0, 0, 0, 0) else None
    if period == 0:
        return "d" if bases > 0 and word == 0 else None
    if copies == 0:
        return "c" if word == 0 else None
    if period == 6:
        return "a" if len(lm.class_counts(slices, 6)) >= min_classes else None
    return "b" if period in (1, 2) else None


def locus_of_kind(rng, kind, max_bases=60, max_depth=5, min_classes=3):
    """the slices (arrays of 4-bit codes) of one locus that the restatement puts in `kind`"""
    for _ in range(50):
        slices = _draw_locus(rng, kind, max_bases, max_depth)
        if kind_of(slices, lm.find(slices), min_classes) == kind:
            return slices
    raise AssertionError(kind)


def given_words(rng, n):
    """given words of n loci: none, a motif, a word that names none"""
    return np.array([rng.choice([0, 0, hipcall.encode_motif("CAG"), rm.literal_word("GGCCCC"), 3 << 60 | 0x321, rm.literal_word("T")]) for _ in range(n)],
                    dtype=np.uint64)


def trip_pairs(kinds, cap):
    """the ordered pairs of kinds that one workgroup of a grid of `cap` meets in consecutive trips: (kinds[j], kinds[j + cap])"""
    return {(kinds[j], kinds[j + cap]) for j in range(len(kinds) - cap)}


def small_locus_case():
    """C1a: (slices, kept_off, kinds, given, expected records) of 400 loci of the five kinds in random order"""
    def make():
        rng = random.Random(2501)
        kinds = [KINDS[i % 5] for i in range(400)]
        rng.shuffle(kinds)
        per_locus = [locus_of_kind(rng, k) for k in kinds]
        slices = [s for loc in per_locus for s in loc]
        kept_off = np.concatenate([[0], np.cumsum([len(loc) for loc in per_locus])]).astype(np.uint64)
        return slices, kept_off, kinds, given_words(rng, 400), lm.records_of(slices, kept_off)
    return _once("small loci", make)


# ---- a pool of items repeated (the real cap) ---------------------------------------------------------------------------------------------
def tiled_offsets(period_counts, n_loci):
    """kept_off u64 [n_loci + 1] of loci whose record counts repeat period_counts"""
    reps = -(-n_loci // len(period_counts))
    counts = np.tile(np.asarray(period_counts, dtype=np.int64), reps)[:n_loci]
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)


def tiled_slices(period_slices, n):
    """(SEQ_DTYPE records, packed bytes) of n slices that repeat period_slices, as rm.seq_arrays gives them - the period's bytes tiled"""
    sq1, packed1 = rm.seq_arrays(period_slices)
    reps, rest = divmod(n, len(period_slices))
    _sq, tail = rm.seq_arrays(period_slices[:rest]) if rest else (None, np.zeros(0, np.uint8))
    return np.concatenate([np.tile(sq1, reps), sq1[:rest]]), np.concatenate([np.tile(packed1, reps), tail])


def tiled_records(period, n):
    return np.concatenate([np.tile(period, n // len(period)), period[: n % len(period)]])


def big_locus_case(n_loci):
    """C2a: n_loci loci that repeat a pool of POOL loci of the five kinds, each of 0 or 1 record of at most 24 bases.  Returns
    (seqs, packed, kept_off, given, expected found, expected use, the pool's kinds)"""
    def pool():
        rng = random.Random(2502)
        kinds = [KINDS[i % 5] for i in range(POOL)]
        rng.shuffle(kinds)
        per_locus = [locus_of_kind(rng, k, max_bases=24, max_depth=1, min_classes=2) for k in kinds]
        slices = [s for loc in per_locus for s in loc]
        counts = [len(loc) for loc in per_locus]
        found = lm.records_of(slices, np.concatenate([[0], np.cumsum(counts)]))
        given = given_words(rng, POOL)
        return kinds, slices, counts, given, found, lm.words_in_use(given, found["word"])
    kinds, slices, counts, given, found, use = _once("locus pool", pool)
    kept_off = tiled_offsets(counts, n_loci)
    sq, packed = tiled_slices(slices, int(kept_off[-1]))
    return sq, packed, kept_off, tiled_records(given, n_loci), tiled_records(found, n_loci), tiled_records(use, n_loci), kinds


# ---- records dealt over loci with a motif of their own (read_motif_kernel) ---------------------------------------------------------------
MOTIFS = ["CAG", "A", "GGCCCC", "AAG", "CA", "ACGTACGTACGTAAA", "T", "CCG", "AT", "TTTTA"]
N_SMALL = READ_MOTIF_TILE * (3 * 7 + 1) + 5  # 357: a partial last tile at every cap, as many full ones as make 1, 2, 3 and 7 uneven


def motif_period(n, seed, max_bases, behind):
    """n records dealt over loci that each have a motif word of their own, empty loci between them, the last `behind` records behind the
    last locus.  Record i is a pure repeat of its locus's motif but for one N, its length a function of i // 16 and i, so that the
    records one, two, three and seven tiles apart differ.  Returns (slices, per-locus counts, locus words, expected records)"""
    rng = random.Random(seed)
    counts, at = [], 0
    while at < n - behind:
        if rng.random() < 0.3:
            counts.append(0)
        take = min(rng.choice([1, 2, 5, 16, 17, 30]), n - behind - at)
        counts.append(take)
        at += take
    counts += [0, 0]
    filled = 0
    words, slices, rec_words = [], [], []
    for cnt in counts:
        motif = MOTIFS[filled % len(MOTIFS)]
        filled += cnt > 0
        words.append(rm.literal_word(motif))
        for _ in range(cnt):
            i = len(slices)
            length = max_bases - 23 + (i // READ_MOTIF_TILE) % 23 + (1 if i % 2 else 0) - 1
            codes = rm.repeat_codes(motif, length, i % 5)
            codes[(3 * i) % length] = 15
            slices.append(codes)
            rec_words.append(words[-1])
    for _ in range(behind):
        slices.append(rm.repeat_codes("CAG", 18))
        rec_words.append(0)  # no locus: four zeros
    return slices, counts, np.array(words, dtype=np.uint64), rm.records_of(slices, rec_words)


def small_motif_case():
    """C1b: (seqs, packed, kept_off, locus words, expected records) of N_SMALL records"""
    def make():
        slices, counts, words, want = motif_period(N_SMALL, 2503, 60, behind=3)
        sq, packed = rm.seq_arrays(slices)
        return sq, packed, np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64), words, want
    return _once("small motifs", make)


N_BIG = READ_MOTIF_TILE * GRID_CAP + READ_MOTIF_TILE + 1  # the second trip: one whole tile and one of one item


def big_motif_case():
    """C2b: N_BIG records that repeat a pool of POOL records in loci that repeat with them; slices of at most 40 bases"""
    def make():
        slices, counts, words, want = motif_period(POOL, 2504, 40, behind=0)
        assert sum(counts) == POOL
        n_loci = -(-N_BIG // POOL) * len(counts)
        kept_off = np.minimum(tiled_offsets(counts, n_loci), N_BIG).astype(np.uint64)
        sq, packed = tiled_slices(slices, N_BIG)
        return sq, packed, kept_off, tiled_records(words, n_loci), tiled_records(want, N_BIG)
    return _once("big motifs", make)


# ---- pairs whose windows differ from tile to tile (seq_window_kernel) --------------------------------------------------------------------
def small_window_case():
    """C1c: (Batch, l_seq, q_beg, n_bases) of N_SMALL pairs in loci of 0 to 16 pairs, every locus with a window of its own over reads that
    all span it: two pairs a tile or more apart lie in different loci, so their q_beg differ"""
    def make():
        rng = random.Random(2505)
        bb = B.BatchBuilder(minlen=5, support=3, unphased=True)
        cigars = [[("M", 3000)], [("M", 700), ("I", 9), ("M", 2300)], [("S", 25), ("M", 3000)], [("M", 400), ("D", 30), ("M", 2600)],
                  [("M", 5), ("I", 2)] * 40 + [("M", 2800)]]
        reads, l_seq = [], []
        for k, cig in enumerate(cigars):
            reads.append(bb.add_read(500 + 7 * k, rs.words_of(cig)))
            l_seq.append(sum(n for o, n in cig if o in "MIS") - (40 if k == 3 else 0))
        left, j = N_SMALL, 0
        while left:
            size = min(left, rng.choice([0, 1, 4, 5, 15, 16, 16, 9]))
            start = 1000 + 11 * j
            bb.add_locus(start, start + 10 + j % 40, [rng.choice(reads) for _ in range(size)])
            left -= size
            j += 1
        bb.add_locus(1000, 1050, [])
        batch, l_seq = bb.build(), np.array(l_seq, dtype=np.uint32)
        return (batch, l_seq) + rs.batch_windows(batch, l_seq)
    return _once("small windows", make)


WINDOWS = [(1000, 1050), (975, 1025), (1015, 1065), (1049, 1050), (1000, 1000)]
POOL_L_SEQ = np.array([300, 312, 280, 150, 300, 50, 307, 0], dtype=np.uint32)


def big_window_case():
    """C2c: N_BIG pairs, built as test_gpu_read_calls._tiled builds its batches - the pool of eight reads, loci of about 30 pairs - over
    the five WINDOWS; the expected (q_beg, n_bases) is computed per (window, read) and gathered.  The pairs of the second trip are given
    a read under which they differ from the pair one trip before them"""
    def make():
        rng = np.random.default_rng(2506)
        base = _pool(True)
        table = np.array([[rs.window(rs.read_words(base, r), int(base.reads["pos"][r]), int(POOL_L_SEQ[r]), s, e) for r in range(8)] for s, e in WINDOWS],
                         dtype=np.uint32)  # [window, read, (q_beg, n_bases)]
        sizes = []
        while sum(sizes) < N_BIG:
            sizes += [int(x) for x in rng.integers(0, 61, size=4096)]
        sizes = np.array(sizes, dtype=np.int64)
        n_loci = int(np.searchsorted(np.cumsum(sizes), N_BIG)) + 1
        sizes = sizes[:n_loci]
        sizes[-1] -= int(sizes.sum()) - N_BIG
        win = rng.integers(0, len(WINDOWS), size=n_loci)
        locus = np.repeat(np.arange(n_loci), sizes)
        pair_read = rng.integers(0, 8, size=N_BIG)
        trip = SEQ_WINDOW_TILE * GRID_CAP
        for p in range(trip, N_BIG):
            before = tuple(table[win[locus[p - trip]], pair_read[p - trip]])
            pair_read[p] = next(r for r in range(8) if tuple(table[win[locus[p]], r]) != before)
        starts, ends = np.array([w[0] for w in WINDOWS], dtype=np.uint32), np.array([w[1] for w in WINDOWS], dtype=np.uint32)
        batch = B.Batch(cigar=base.cigar, reads=base.reads, pair_read=pair_read.astype(np.uint32),
                        locus_pair_off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64), locus_start=starts[win], locus_end=ends[win],
                        minlen=5, support=3, unphased=True)
        want = table[win[locus], pair_read]
        return batch, POOL_L_SEQ, np.ascontiguousarray(want[:, 0]), np.ascontiguousarray(want[:, 1]), table
    return _once("big windows", make)


# ---- the compaction's scan past its first step (read_call_scan) --------------------------------------------------------------------------
FIRST_STEP = SCAN_STEP * READ_CALL_TILE  # pairs of the scan's first step: 2^20
SCAN_TOTALS = {"256T": FIRST_STEP, "256T+1": FIRST_STEP + 1, "256T+T+5": FIRST_STEP + READ_CALL_TILE + 5}
SCAN_CASES = list(SCAN_TOTALS) + ["carry=2^20"]


def scan_batch(name, unphased):
    """C3: the pool of test_gpu_read_calls offered to loci of 0 to 60 pairs.  The three totals: a locus begins seven pairs in front of pair
    256 T and ends at it, one past it, or 23 past it.  "carry=2^20": 256 T + T + 5 pairs whose first 256 T are all kept reads, with a
    locus boundary at pair 256 T, so that the second step begins with the largest carry the first can hand on"""
    def make():
        total = SCAN_TOTALS.get(name, FIRST_STEP + READ_CALL_TILE + 5)
        rng = np.random.default_rng(2507 + len(name))
        edge = FIRST_STEP - (0 if name.startswith("carry") else 7)
        sizes, at = [], 0
        while at < edge:  # the loci in front of the edge, the last one cut to end on it
            s = min(int(rng.integers(0, 61)), edge - at)
            sizes.append(s)
            at += s
        sizes.append(min(30, total - at))  # from the edge on: 7, 8 and 30 pairs; 30 behind the boundary of the carry case
        at += sizes[-1]
        while at < total:
            s = min(int(rng.integers(0, 61)), total - at)
            sizes.append(s)
            at += s
        sizes += [0, 0]
        pair_read = rng.integers(0, 8, size=total)
        if name.startswith("carry"):
            pair_read[:FIRST_STEP] = rng.choice(np.array(KEPT), size=FIRST_STEP)
        else:  # kept pairs on both sides of the step's edge
            pair_read[FIRST_STEP - 1 : FIRST_STEP + 1] = [3, 1][: total - FIRST_STEP + 1]
        return _tiled(unphased, pair_read, sizes)
    return _once(("scan", name, unphased), make)


def scan_expected(orc, name, unphased):
    """(Batch, oracle Result, expected kept_off, expected records)"""
    batch = scan_batch(name, unphased)
    return (batch,) + _oracle(orc, ("side geometry scan", name, unphased), batch)


# ---- kept_pair past index 2^20: a flush with sequences -----------------------------------------------------------------------------------
# Pairs are (read, locus): 4 500 reads under 257 overlapping BED lines are 1 156 500 pairs of one deferred batch, and the 4 091 reads
# that pass the filter give 1 051 387 kept records, so the compaction's second step writes kept_pair, and the kernels behind it read it
PAIR_READS, PAIR_LOCI = 4500, 257
PAIR_WINDOW = (5000, 5100)  # the first locus; locus i is (5000 + i % 16, 5100 + i // 16)
PAIR_SEQ = 40               # bases of every SEQ: each slice is cut by it


def kept_pair_loci():
    return [(PAIR_WINDOW[0] + i % 16, PAIR_WINDOW[1] + i // 16) for i in range(PAIR_LOCI)]


def kept_pair_reads():
    """(name, flag, pos, mapq, cigar, tags, SEQ codes) in file order, as tests.test_gpu_read_seqs._write takes them: every read spans
    every locus's window from one of seven starts; every eleventh has mapq 5 and is kept by no locus"""
    def make():
        se = PAIR_WINDOW[0] - 10
        reads = [(f"p{k}" + "z" * (k % 5), 0x10 if k % 3 == 0 else 0, se - k % 7, 5 if k % 11 == 5 else 60, [("M", k % 7 + 330)], [("HP", "C", 1 + k % 2)],
                  rs.seq_codes(k, PAIR_SEQ)) for k in range(PAIR_READS)]
        reads.sort(key=lambda r: r[2])
        return reads
    return _once("kept pair reads", make)


def kept_pair_expected(pair_read, pair_off, starts, ends):
    """What the flush must give for the pairs the device front end formed (pair_read u32 [n_pairs] indexes kept_pair_reads(); pair_off
    [n_loci + 1]; the loci's windows): per pair (q_beg, n_bases) by read_seq_case.window, computed once per distinct (CIGAR, pos) and locus
    and gathered; which pairs are kept, by the unphased filter restated; kept_off"""
    reads = kept_pair_reads()
    shapes, shape_of = {}, np.zeros(len(reads), dtype=np.int64)
    for r, (_name, _flag, pos, _mapq, cigar, _tags, codes) in enumerate(reads):
        shape_of[r] = shapes.setdefault((pos, tuple(cigar), len(codes)), len(shapes))
    n_loci = len(starts)
    table = np.zeros((len(shapes), n_loci, 2), dtype=np.uint32)
    spans_all = np.zeros((len(shapes), n_loci), dtype=bool)
    for (pos, cigar, l_seq), s in shapes.items():
        for j in range(n_loci):
            table[s, j] = rs.window(rs.words_of(list(cigar)), pos, l_seq, int(starts[j]), int(ends[j]))
            se, ee = int(starts[j]) - 10, int(ends[j]) + 10
            spans_all[s, j] = pos <= se and pos + sum(n for _o, n in cigar) >= ee
    locus = np.repeat(np.arange(n_loci), np.diff(np.asarray(pair_off).astype(np.int64)))
    pr = np.asarray(pair_read).astype(np.int64)
    mapq = np.array([r[3] for r in reads])
    kept = (mapq[pr] > 10) & spans_all[shape_of[pr], locus]
    qn = table[shape_of[pr], locus]
    before = np.concatenate([[0], np.cumsum(kept)]).astype(np.uint64)
    return qn[:, 0].copy(), qn[:, 1].copy(), kept, before[np.asarray(pair_off).astype(np.int64)]


def packed_slices(read, q_beg, n_bases, chunk=1 << 17):
    """the packed bytes of the slices [q_beg, q_beg + n_bases) of kept_pair_reads()[read]'s SEQ, back to back: read_seq_case.pack of each,
    as one gather"""
    reads = kept_pair_reads()
    width = PAIR_SEQ + 2
    codes = np.zeros((len(reads), 2 * width), dtype=np.uint8)
    for r, rd in enumerate(reads):
        codes[r, : len(rd[6])] = rd[6]
    out = []
    for a in range(0, len(read), chunk):
        r, q, n = (np.asarray(x[a : a + chunk]).astype(np.int64) for x in (read, q_beg, n_bases))
        col = np.arange(width)
        bases = np.where(col < n[:, None], codes[r[:, None], q[:, None] + col], 0).astype(np.uint8)
        both = (bases[:, 0::2] << 4) | bases[:, 1::2]
        out.append(both[np.arange(width // 2) < ((n + 1) // 2)[:, None]])
    return np.concatenate(out) if out else np.zeros(0, np.uint8)


def names_of(read):
    """the names of kept_pair_reads()[read], back to back, and their lengths"""
    reads = kept_pair_reads()
    names = [r[0].encode() for r in reads]
    lens = np.array([len(x) for x in names])
    table = np.zeros((len(names), int(lens.max())), dtype=np.uint8)
    for r, x in enumerate(names):
        table[r, : len(x)] = np.frombuffer(x, dtype=np.uint8)
    r = np.asarray(read).astype(np.int64)
    return table[r][np.arange(table.shape[1]) < lens[r][:, None]], lens[r]
