"""read_motif_kernel alone (inq_motif_runs; read_motifs.hip) against the numpy restatement of tests/read_motif_case.py.  The shapes are
the kernel's own: slices on and next to its 16-base word, runs that cross a word boundary and the coverage it defers, the odd last
nibble and the neighbouring segment, rotations that overlap, every motif length, a slice of tens of kilobases, and records per launch
on and next to the row, wave, workgroup and grid tile with empty loci between them."""
import numpy as np
import pytest

from inquistr_amd import batch as B
from inquistr_amd import hipcall
from tests import read_motif_case as rm
from tests import read_seq_case as rs

pytestmark = pytest.mark.gpu

CAG = hipcall.encode_motif("CAG")


@pytest.fixture(scope="module")
def ctx():
    c = hipcall.Context(0)
    assert c.backend.startswith("hip:gfx950")
    yield c
    c.close()


def run(ctx, slices, words, kept_off=None, locus_words=None):
    """slices[i] under words[i], each record a locus of its own unless kept_off / locus_words say otherwise; checked against the
    restatement record by record, returned as tuples"""
    sq, packed = rm.seq_arrays(slices)
    if kept_off is None:
        kept_off, locus_words = np.arange(len(slices) + 1, dtype=np.uint64), np.array(words, dtype=np.uint64)
    got = ctx.motif_runs(sq, packed, kept_off, locus_words)
    want = rm.records_of(slices, words)
    assert got.dtype == hipcall.MOTIF_DTYPE and len(got) == len(slices)
    for i in range(len(slices)):
        assert tuple(got[i]) == tuple(want[i]), (i, len(slices[i]), hex(int(words[i])), tuple(got[i]), tuple(want[i]))
    return [tuple(int(x) for x in g) for g in got]


def test_known_answers(ctx):
    slices = [rm.codes_of(k[0]) for k in rm.KNOWN]
    words = [hipcall.encode_motif(k[1]) for k in rm.KNOWN]
    assert run(ctx, slices, words) == [k[2:] for k in rm.KNOWN]


@pytest.mark.parametrize("motif", ["A", "CA", "CAG", "AAG", "GGCCCC", "ACGTACGTACGTAAA"])
def test_segment_lengths(ctx, motif):
    """pure, interrupted and random slices of every length around the motif and around the word"""
    k = len(motif)
    rng = np.random.default_rng(k)
    lengths = sorted({0, 1, k - 1, k, k + 1, 2 * k - 1, 15, 16, 17, 31, 32, 33, 127, 128, 129})
    slices = []
    for n in lengths:
        for phase in (0, k // 2):
            pure = rm.repeat_codes(motif, n, phase)
            slices.append(pure)
            cut = pure.copy()
            if n:
                cut[rng.integers(0, n, size=max(1, n // 9))] = rng.integers(0, 16, size=max(1, n // 9))
            slices.append(cut)
        slices.append(rng.integers(0, 16, size=n).astype(np.uint8))
    got = run(ctx, slices, [rm.literal_word(motif)] * len(slices))
    at = 5 * lengths.index(16)
    assert got[at][:2] == (0, 16) and got[at][2] == 16


def _placed(n, motif, runs, fill=15):
    """n bases of `fill` (N) with pure runs of motif at (start, length, phase)"""
    codes = np.full(n, fill, dtype=np.uint8)
    for start, length, phase in runs:
        codes[start : start + length] = rm.repeat_codes(motif, length, phase)
    return codes


@pytest.mark.parametrize("motif", ["CAG", "GGCCCC", "ACGTACGTACGTAAA", "A"])
def test_run_placement(ctx, motif):
    k = len(motif)
    slices = []
    for phase in range(min(k, 4)):
        slices.append(_placed(40, motif, [(15, 2, phase)]))            # begins on a word's last base, ends on the next one's first
        slices.append(_placed(48, motif, [(16 - (k - 1), k, phase)]))  # exactly k, split k - 1 | 1 over a word boundary ...
        slices.append(_placed(48, motif, [(31, k, phase)]))            # ... and 1 | k - 1: the coverage of the first word waits
        slices.append(_placed(48, motif, [(16 - (k - 1), k - 1, phase)]) if k > 1 else _placed(48, motif, []))  # one short: never covered
        slices.append(_placed(64, motif, [(16 - (k - 1), k - 1 + 16 + 3, phase)]))  # over a whole word and on
        for n in (37, 38, 47, 48, 49):  # reaches the slice's last base: n odd, n even, on and next to a word
            slices.append(_placed(n, motif, [(n - k - 2, k + 2, phase)]))
            slices.append(_placed(n, motif, [(n - 1, 1, phase)]))
    got = run(ctx, slices, [rm.literal_word(motif)] * len(slices))
    assert got[0][:2] == (15, 2)
    assert got[1] == (16 - (k - 1), k, k, 1) and got[2] == (31, k, k, 1)
    if k > 1:
        assert got[3] == (16 - (k - 1), k - 1, 0, 0)


def test_neighbouring_segments_do_not_see_each_other(ctx):
    """back-to-back segments whose second begins with the bases that would carry the first one's run on - also across the odd last
    nibble, whose byte the segments do not share"""
    a_odd, a_even = rm.repeat_codes("CAG", 17), rm.repeat_codes("CAG", 18)
    slices = [a_odd, rm.repeat_codes("CAG", 9, 17 % 3), a_even, rm.repeat_codes("CAG", 9, 18 % 3), rm.repeat_codes("CAG", 1), rm.repeat_codes("CAG", 30, 1)]
    got = run(ctx, slices, [CAG] * len(slices))
    assert got == [(0, 17, 17, 1), (0, 9, 9, 1), (0, 18, 18, 1), (0, 9, 9, 1), (0, 1, 0, 0), (0, 30, 30, 1)]
    # a last odd low nibble that is NOT zero (a caller's own packing) is not compared either: C continues ...CAG
    sq, packed = rm.seq_arrays([rm.repeat_codes("CAG", 15)])
    dirty = packed.copy()
    dirty[-1] |= rm.CODE["C"]
    assert tuple(ctx.motif_runs(sq, dirty, [0, 1], [CAG])[0]) == (0, 15, 15, 1)


@pytest.mark.parametrize("motif", ["CAG", "GGCCCC", "ACGTACGTACGTAAA"])
def test_phase_shift_overlaps_by_k_minus_1(ctx, motif):
    """a one-base deletion inside a pure repeat: two runs at different rotations that share k - 1 bases; motif_bases is the union"""
    k = len(motif)
    for cut_at in (20, 31, 32, 33):
        pure = rm.repeat_codes(motif, 70)
        codes = np.delete(pure, cut_at)
        got = run(ctx, [codes], [rm.literal_word(motif)])[0]
        assert got[2] == 69 and got[3] == 2, (motif, cut_at, got)


def test_motif_shapes(ctx):
    rng = np.random.default_rng(5)
    noise = rng.integers(0, 16, size=200).astype(np.uint8)
    every = np.concatenate([rm.repeat_codes(m, 40, 1) for m in ("A", "CCCCGCCCCGCG", "AAG", "ACGTACGTACGTAAA")] + [noise])
    words = [rm.literal_word(m) for m in ("A", "T", "AAG", "CCCCGCCCCGCG", "AAAAAAAAAAAAAAC", "ACGTACGTACGTAAA", "CAGCAG", "CACA")]
    words += [0, 3 << 60 | 0x321, 3 << 60 | 0x021, 2 << 60 | 0xF1, 15 << 60, CAG | 0xABC << 12, 0xFFFFFFFFFFFFFFFF]
    got = run(ctx, [every] * len(words), words)
    assert got[8:13] == [(0, 0, 0, 0)] * 5 and got[14] == (0, 0, 0, 0), "no motif, a bad nibble: four zeros"
    # a literal non-primitive word counts its runs once per equivalent rotation
    codes = rm.codes_of("CAGCAGCAGCAGTTCAGCAGCAG")
    assert run(ctx, [codes, codes], [rm.literal_word("CAGCAG"), CAG]) == [(0, 12, 21, 4), (0, 12, 21, 2)]


def test_long_slice_among_short_ones(ctx):
    """40 000 bases, pure but for an interruption every 997: the open run's length travels from word to word"""
    long = rm.repeat_codes("CAG", 40_000, 2)
    long[996::997] = 15
    short = [rm.repeat_codes("CAG", n, n % 3) for n in (5, 0, 33, 16)]
    slices = short[:2] + [long] + short[2:] + [long[:39_999], rm.repeat_codes("GGCCCC", 20_011)]
    words = [CAG] * 6 + [rm.literal_word("GGCCCC")]
    got = run(ctx, slices, words)
    n_cut = len(range(996, 40_000, 997))
    assert got[2] == (0, 996, 40_000 - n_cut, n_cut + 1) and got[6] == (0, 20_011, 20_011, 1)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 257])
def test_records_per_launch_and_loci(ctx, n):
    """n records dealt among loci with runs of empty loci at the start, in the middle and at the end, a locus of one record and - for
    257 - one of the rest; every locus has a motif of its own, so a record that took a neighbour's locus shows"""
    rng = np.random.default_rng(n)
    motifs = ["CAG", "A", "GGCCCC", "AAG", "CA", "ACGTACGTACGTAAA", "T"]
    counts = [0, 0, 0, 1, 0, min(2, n - 1), 0, 0] + [0] * 17 + [max(0, n - 1 - min(2, n - 1)), 0, 0]
    assert sum(counts) == n
    kept_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    locus_words = np.array([rm.literal_word(motifs[j % len(motifs)]) for j in range(len(counts))], dtype=np.uint64)
    slices, words = [], []
    for j, cnt in enumerate(counts):
        for _ in range(cnt):
            length = int(rng.integers(0, 70))
            codes = rm.repeat_codes(motifs[j % len(motifs)], length, int(rng.integers(0, 15)))
            if length:
                codes[rng.integers(0, length, size=2)] = 15
            slices.append(codes)
            words.append(int(locus_words[j]))
    run(ctx, slices, words, kept_off, locus_words)


@pytest.mark.parametrize("n_loci", rs.SEARCH_LOCUS_COUNTS)
def test_locus_search_steps(ctx, n_loci):
    """a record's locus where the sixteen-probe search takes one to four steps: one record in the first locus, the last and on each side
    of the probes' boundaries (read_seq_case.search_probe_loci), every other locus empty.  A slice is a pure repeat of its own locus's
    motif, which differs from both non-empty neighbours': under a neighbour's word the run comes out shorter"""
    motifs = ["CAG", "A", "GGCCCC", "AAG", "CA", "ACGTACGTACGTAAA", "T"]
    filled = rs.search_probe_loci(n_loci)
    assert len(filled) <= 60 and filled[0] == 0 and filled[-1] == n_loci - 1
    counts = np.zeros(n_loci, dtype=np.uint64)
    counts[filled] = 1
    kept_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    locus_words = np.array([rm.literal_word(motifs[j % len(motifs)]) for j in range(n_loci)], dtype=np.uint64)
    slices, words = [], []
    for i, j in enumerate(filled):  # (by rank: neighbours among the filled loci never share a word, whatever lies between them)
        locus_words[j] = rm.literal_word(motifs[i % len(motifs)])
        slices.append(rm.repeat_codes(motifs[i % len(motifs)], 20 + i % 21, i % 3))
        words.append(int(locus_words[j]))
    got = run(ctx, slices, words, kept_off, locus_words)
    assert all(g[:3] == (0, len(s), len(s)) for g, s in zip(got, slices))


def test_a_locus_of_300_records(ctx):
    rng = np.random.default_rng(300)
    counts = [5, 300, 0, 7]
    kept_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    locus_words = np.array([CAG, rm.literal_word("AAG"), 0, rm.literal_word("T")], dtype=np.uint64)
    slices = [rng.choice(np.array([1, 2, 4, 8, 15], dtype=np.uint8), size=int(rng.integers(0, 90)), p=[0.4, 0.1, 0.4, 0.05, 0.05]) for _ in range(312)]
    words = [int(locus_words[j]) for j, cnt in enumerate(counts) for _ in range(cnt)]
    run(ctx, slices, words, kept_off, locus_words)


def test_degenerate_launches(ctx):
    none = np.zeros(0, dtype=hipcall.SEQ_DTYPE)
    rc, got = ctx.motif_runs(none, np.zeros(0, np.uint8), [0, 0, 0], [CAG, CAG], check=False)
    assert rc == 0 and len(got) == 0
    rc, got = ctx.motif_runs(none, np.zeros(0, np.uint8), [0], [], check=False)
    assert rc == 0 and len(got) == 0
    sq, packed = rm.seq_arrays([rm.repeat_codes("CAG", 12)] * 3)
    assert ctx.motif_runs(sq, packed, [0, 2, 4], [CAG, CAG], check=False)[0] == B.INQ_ERR_ARG, "kept_off ends past the records"
    assert ctx.motif_runs(sq, packed, [0, 3, 2], [CAG, CAG], check=False)[0] == B.INQ_ERR_ARG, "kept_off does not ascend"
    # records behind the last locus, and no locus at all: four zeros
    rc, got = ctx.motif_runs(sq, packed, [0, 2], [CAG], check=False)
    assert rc == 0 and [tuple(g) for g in got] == [(0, 12, 12, 1), (0, 12, 12, 1), (0, 0, 0, 0)]
    rc, got = ctx.motif_runs(sq, packed, [0], [], check=False)
    assert rc == 0 and [tuple(g) for g in got] == [(0, 0, 0, 0)] * 3
    # a record whose slice does not fit into the bytes handed over reads none of them
    rc, got = ctx.motif_runs(sq, packed[:13], [0, 3], [CAG], check=False)
    assert rc == 0 and [tuple(g) for g in got] == [(0, 12, 12, 1), (0, 12, 12, 1), (0, 0, 0, 0)]
    assert ctx.read_motif_tile == 16
