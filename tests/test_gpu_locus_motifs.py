"""locus_motif_kernel alone (inq_locus_motifs_find) against the numpy restatement, field by field: the known answers, every slice length
around the 16-base word and the i + 2p <= n edge, copies across word boundaries, neighbouring segments, the ties, loci of every depth,
the given words, the argument checks."""
import random

import numpy as np
import pytest

from inquistr_amd import batch as B
from inquistr_amd import hipcall
from tests import locus_motif_case as lm
from tests import read_motif_case as rm

pytestmark = pytest.mark.gpu

MOTIF_OF_LENGTH = {1: "A", 2: "CA", 3: "CAG", 4: "AAAG", 5: "TTTTA", 6: "GGCCCC"}


@pytest.fixture(scope="module")
def ctx():
    c = hipcall.Context(0)
    assert c.backend.startswith("hip:gfx950")
    yield c
    c.close()


def run(ctx, slices, kept_off=None, given=None, use=True):
    """(found, use) of the kernel over slices (one locus each unless kept_off says otherwise)"""
    sq, packed = rm.seq_arrays(slices)
    off = np.arange(len(slices) + 1, dtype=np.uint64) if kept_off is None else np.asarray(kept_off, dtype=np.uint64)
    return ctx.locus_motifs_find(sq, packed, off, given, use=use)


def check(ctx, slices, kept_off=None):
    off = np.arange(len(slices) + 1, dtype=np.uint64) if kept_off is None else np.asarray(kept_off, dtype=np.uint64)
    found, use = run(ctx, slices, off)
    want = lm.records_of(slices, off)
    bad = [(j, tuple(int(x) for x in found[j]), tuple(int(x) for x in want[j])) for j in range(len(want)) if found[j] != want[j]]
    assert not bad, bad[:5]
    assert found.tobytes() == want.tobytes() and np.array_equal(use, want["word"])
    return want


def test_known_answers(ctx):
    want = check(ctx, [rm.codes_of(k[0]) for k in lm.KNOWN])
    for w, (_text, _lags, p, motif, copies) in zip(want, lm.KNOWN):
        assert (int(w["word"]), int(w["period"]), int(w["copies"])) == (rm.literal_word(motif) if motif else 0, p, copies)


@pytest.mark.parametrize("p", range(1, 7))
def test_slice_lengths(ctx, p):
    """every length around the period, the copy edge and the 16-base word, as pure, interrupted and random codes"""
    rng = random.Random(40 + p)
    motif = MOTIF_OF_LENGTH[p]
    lengths = sorted({0, 1, p - 1, p, 2 * p - 1, 2 * p, 2 * p + 1, 15, 16, 17, 31, 32, 33, 127, 128, 129})
    slices = []
    for n in lengths:
        for phase in range(p):
            slices.append(rm.repeat_codes(motif, n, phase))
        slices.append(rm.noisy_repeat(rng, motif, n))
        broken = rm.repeat_codes(motif, n)
        if n:
            broken[rng.randrange(n)] = rng.choice([0, 15, 3, 5])
        slices.append(broken)
        slices.append(np.array([rng.randrange(16) for _ in range(n)], dtype=np.uint8))
    want = check(ctx, slices)
    assert (want["copies"] > 0).any() and (want["period"] == p).any() and ((want["period"] != 0) & (want["copies"] == 0)).any()


@pytest.mark.parametrize("p", range(1, 7))
def test_a_copy_across_the_word_boundary(ctx, p):
    """exactly one would-be copy (2p bases) among N, beginning at every offset around positions 16 and 32; then with an N or an
    ambiguity code in each of its places"""
    motif = {1: "A", 2: "CA", 3: "CAG", 4: "ACGT", 5: "ACGTA", 6: "ACGTCA"}[p]  # (two copies of it have their most lag hits at lag p)
    slices = []
    for beg in range(16 - 2 * p - 1, 34):
        if beg < 0:
            continue
        s = np.full(50, 15, dtype=np.uint8)
        s[beg : beg + 2 * p] = rm.repeat_codes(motif, 2 * p)
        slices.append(s)
        for hole in range(2 * p):
            for code in (15, 3):
                t = s.copy()
                t[beg + hole] = code
                slices.append(t)
    want = check(ctx, slices)
    assert ((want["copies"] == 1) & (want["period"] == p)).sum() >= 18 and (want["copies"] == 0).sum() > 18 * p


def test_neighbouring_segments_do_not_see_each_other(ctx):
    """back to back, the second continuing the first one's repeat: odd and even lengths, a dirty last nibble; each is a locus of its own
    and must come out as if the other were not there"""
    for motif in ("CAG", "CA", "GGCCCC", "A"):
        k = len(motif)
        for n_first in (5, 6, 15, 16, 17, 31, 33):
            first, second = rm.repeat_codes(motif, n_first), rm.repeat_codes(motif, 2 * k, phase=n_first % k)
            sq, packed = rm.seq_arrays([first, second])
            packed = packed.copy()
            if n_first % 2:
                packed[(n_first - 1) // 2] |= rm.CODE[motif[n_first % k]]  # the unused nibble holds the repeat's next base
            found, _ = ctx.locus_motifs_find(sq, packed, np.array([0, 1, 2], dtype=np.uint64))
            assert found.tobytes() == lm.records_of([first, second], [0, 1, 2]).tobytes(), (motif, n_first)
            # ... and as two records of one locus: still no copy across the seam
            both, _ = ctx.locus_motifs_find(sq, packed, np.array([0, 2], dtype=np.uint64))
            assert both.tobytes() == lm.records_of([first, second], [0, 2]).tobytes(), (motif, n_first)


def test_ties_and_the_primitive_root(ctx):
    c = rm.codes_of
    two = [c("ACAC"), c("ACGTAC")]  # T_2 == T_4
    tie = [c("CACACAGAGAG")]  # AC and AG both count 3
    root = [c("AC" * 6), c("ACGT" * 2 + "A"), c("AGGT" * 2 + "A")]  # the winner at period 4 is ACAC
    want = check(ctx, two + tie + root, [0, 2, 3, 6])
    assert [int(x) for x in want["period"]] == [2, 2, 4]
    assert [int(x) for x in want["word"]] == [rm.literal_word("AC")] * 3 and int(want["copies"][2]) == 5
    # T_3 == T_6 over long pure repeats is no tie (T_3 is larger); equal counts at 1 and 2: homopolymer pairs
    check(ctx, [c("AAGGAAGG" * 3), c("AACCAACC")], [0, 2])
    rng = random.Random(77)
    for alphabet in ([1, 4], [1, 2, 4, 8]):  # few letters: many equal counts
        slices = [np.array([rng.choice(alphabet) for _ in range(rng.choice([3, 6, 9, 14, 20]))], dtype=np.uint8) for _ in range(400)]
        check(ctx, slices)
        check(ctx, slices, np.arange(0, 401, 4))


def test_locus_depths(ctx):
    """0, 1, 15, 16, 17, 63, 64, 65, 257 and 300 records, with empty loci between them"""
    rng = random.Random(5)
    slices, off = [], [0]
    for depth in (0, 1, 15, 16, 17, 63, 64, 65, 257, 300):
        motif = rng.choice(["CAG", "GGCCCC", "AT", "TTTTA"])
        slices += [rm.noisy_repeat(rng, motif, rng.choice([0, 9, 40, 163])) for _ in range(depth)]
        off += [len(slices), len(slices)]  # ... and an empty locus behind each
    want = check(ctx, slices, off)
    assert (want["bases"][1::2] == 0).all() and (want["word"][2::2] != 0).sum() >= 7


def test_a_deep_locus_and_a_long_slice(ctx):
    rng = random.Random(6)
    deep = [rm.noisy_repeat(rng, "CCG", rng.choice([12, 13, 30])) for _ in range(5000)]
    want = check(ctx, deep, [0, 5000])
    assert int(want["word"][0]) == rm.literal_word("CCG") and int(want["copies"][0]) > 20_000
    mixed = [rm.noisy_repeat(rng, "AAG", 30) for _ in range(9)]
    mixed.insert(4, rm.noisy_repeat(rng, "AAG", 40_000))
    want = check(ctx, mixed, [0, 3, 10])
    assert int(want["bases"][1]) > 40_000 and int(want["word"][1]) == rm.literal_word("AAG")


def test_given_words(ctx):
    c = rm.codes_of
    slices = [c("CAGCAGCAGCAG"), c("ACGT"), c("AAAA"), c("CACACACA"), c("TTTTTT")]
    cag, ccg = hipcall.encode_motif("CAG"), hipcall.encode_motif("CCG")
    given = np.array([ccg, cag, 0, 3 << 60 | 0x321, ccg | 0xABC << 12], dtype=np.uint64)  # valid, valid, k = 0, two bits in a nibble, valid
    found, use = run(ctx, slices, given=given)
    want = lm.records_of(slices, np.arange(6))
    assert found.tobytes() == want.tobytes()
    assert [int(x) for x in use] == [ccg, cag, rm.literal_word("A"), rm.literal_word("AC"), int(given[4])]
    assert np.array_equal(use, lm.words_in_use(given, want["word"]))
    found2, none = run(ctx, slices, given=given, use=False)
    assert none is None and found2.tobytes() == want.tobytes()
    found3, use3 = run(ctx, slices)
    assert found3.tobytes() == want.tobytes() and np.array_equal(use3, want["word"])


def test_degenerate_launches_and_argument_errors(ctx):
    sq, packed = rm.seq_arrays([rm.codes_of("CAGCAGCAG")])
    L, h = ctx._L, ctx._h
    off = np.array([0, 1], dtype=np.uint64)
    out = np.zeros(1, dtype=hipcall.LOCUS_MOTIF_DTYPE)
    good = (sq.ctypes.data, 1, packed.ctypes.data, packed.size, off.ctypes.data, 1, None, out.ctypes.data, None)
    assert L.inq_locus_motifs_find(h, *good) == 0 and int(out["period"][0]) == 3

    def with_(i, v):
        a = list(good)
        a[i] = v
        return a

    assert L.inq_locus_motifs_find(h, *with_(0, None)) == B.INQ_ERR_ARG  # records without their array
    assert L.inq_locus_motifs_find(h, *with_(2, None)) == B.INQ_ERR_ARG  # bytes without theirs
    assert L.inq_locus_motifs_find(h, *with_(4, None)) == B.INQ_ERR_ARG  # no offsets
    assert L.inq_locus_motifs_find(h, *with_(7, None)) == B.INQ_ERR_ARG  # loci without their records
    assert L.inq_locus_motifs_find(h, *with_(1, 1 << 40)) == B.INQ_ERR_ARG
    down = np.array([1, 0], dtype=np.uint64)
    assert L.inq_locus_motifs_find(h, *with_(4, down.ctypes.data)) == B.INQ_ERR_ARG  # offsets that descend
    past = np.array([0, 2], dtype=np.uint64)
    assert L.inq_locus_motifs_find(h, *with_(4, past.ctypes.data)) == B.INQ_ERR_ARG  # more records than there are
    # no locus: nothing is written; no record: every locus is zeros; a slice that does not fit into the bytes contributes nothing
    assert L.inq_locus_motifs_find(h, sq.ctypes.data, 1, packed.ctypes.data, packed.size, np.zeros(1, dtype=np.uint64).ctypes.data, 0, None, None, None) == 0
    found, use = ctx.locus_motifs_find(sq[:0], packed[:0], np.zeros(4, dtype=np.uint64))
    assert found.tobytes() == bytes(3 * 40) and not use.any()
    found, _ = ctx.locus_motifs_find(sq, packed[:-1], off)
    assert found.tobytes() == bytes(40)
    assert ctx.read_motifs_fetch(1, check=False)[0] == B.INQ_ERR_ARG, "the kernel alone offers no read-motif record"
