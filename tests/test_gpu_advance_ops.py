"""The reference advance of one CIGAR op as the walks take it from the packed word (csrc/cigar_walk.h ref_advance_raw: the op's
entry of a consume table, looked up with the word's low five bits - op | (len & 1) << 4 -, is the width of a bit-field extract of
the length): every op code 0 .. 8 at the lengths 0, 1, 2, 15, 16, 2^28 - 2 and 2^28 - 1 (both parities of every size), at each of the
four positions of a 16-byte group.

A read is `t` one-base M ops, the op under test, M 30, I 6, M 5; its start is chosen so that the I op stands at reference position R
whatever the op under test consumes, R the same for every read.  Four windows then tell an exact advance from every other one: in A
position R is the lowest that counts, in B the highest - the I op is inside both only if the advance is exact -, A' and B' are those
moved on by one base, where it is outside.  The oracle's per-pair Calls say so before the kernels are asked: 6, 6, 0, 0.

t puts the op under test into head lines 1, 2, 3 and 4 of the window-bounded walk and into the 16-lane rows behind them (a read of
more than four lines); the promise variants take the same reads through the whole walk (`none`) and both at once; a locus of 65 reads
goes through locus_call_mid_walk.  One read per op code 9 .. 15, unpromised as its producer must leave it: the oracle's status.
Everything equal to the oracle, bit for bit."""
import numpy as np
import pytest

from inquistr_amd import batch as B
from inquistr_amd.window_bytes import checked_mask
from tests.walkutil import _all_variants, open_ctx

pytestmark = pytest.mark.gpu

R = (1 << 28) + 5000  # where every read's counted I op stands
MINLEN, COUNTED = 2, 6
LENGTHS = (0, 1, 2, 15, 16, (1 << 28) - 2, (1 << 28) - 1)
ZONES = {"head line 1": 8, "head line 2": 40, "head line 3": 72, "head line 4": 104, "16-lane rows": 168}  # op index of a group's first op
CONSUMES = (0, 2, 3, 7, 8)  # M D N = X
# locus (start, end) -> the positions that count are start - 9 .. end + 9
WINDOWS = {"A": (R + 9, R + 9), "B": (R - 9, R - 9), "A'": (R + 10, R + 10), "B'": (R - 10, R - 10)}
INSIDE = {"A": True, "B": True, "A'": False, "B'": False}


@pytest.fixture(scope="module")
def ctx():
    yield from open_ctx()


def _read(code, length, t):
    """(pos, words): the op (code, length) as op t of the read, the counted I op at reference position R."""
    words = np.concatenate([np.full(t, (1 << 4) | 0, dtype=np.uint32), np.array([(length << 4) | code], dtype=np.uint32),
                            B.encode_cigar([("M", 30), ("I", COUNTED), ("M", 5)])])
    consumed = t + (length if code in CONSUMES else 0) + 30
    return R - 1 - consumed, words  # the first op stands at pos + 1


def _add_at_line_start(bb, pos, words):
    """The read at the start of a 128-byte line of the batch's CIGAR (a filler read no locus is offered in front), so that op t of
    the read is op t of its first line."""
    fill = -bb._off4 % 8
    if fill:
        bb.add_read(0, B.encode_cigar([("M", 1)] * (4 * fill)), phase=1)
    i = bb.add_read(pos, words, phase=1 + len(bb._reads) % 2)
    assert bb._reads[i][0] % 8 == 0
    return i


def _batch(unphased, zone):
    bb = B.BatchBuilder(minlen=MINLEN, support=1, unphased=unphased)
    idx = [_add_at_line_start(bb, *_read(code, length, ZONES[zone] + at)) for code in range(9) for length in LENGTHS for at in range(4)]
    inside = []
    for name, (start, end) in WINDOWS.items():
        blocks = [idx[lo : lo + 64] for lo in range(0, len(idx), 64)] + [idx[:65]] + [[i] for i in idx[::37]]
        for block in blocks:
            bb.add_locus(start, end, block)
            inside += [INSIDE[name]] * len(block)
    batch = bb.build()
    assert checked_mask(batch)[idx].all(), "every read may be promised: the spans stay far below 2^31"
    return batch, np.array(inside)


@pytest.mark.parametrize("unphased", [False, True], ids=("phased", "unphased"))
@pytest.mark.parametrize("zone", list(ZONES))
def test_every_op_and_length_in_front_of_the_window(ctx, orc, unphased, zone):
    batch, inside = _batch(unphased, zone)
    oc, want = orc.call_batch(batch, debug=True)
    assert oc == B.INQ_OK
    assert np.array_equal(want.pair_call, np.where(inside, COUNTED, 0)), "the I op counts in A and B and in neither A' nor B'"
    _all_variants(ctx, orc, batch, zone)


@pytest.mark.parametrize("code", range(9, 16))
def test_an_op_code_no_cigar_has_is_the_oracles_status(ctx, orc, code):
    """The op codes 9 .. 15 in an unpromised read: both length parities, every position of a group, in front of a counted op."""
    bb = B.BatchBuilder(minlen=MINLEN, support=1, unphased=True)
    idx = []
    for length in (16, 15):
        for at in range(4):
            idx.append(_add_at_line_start(bb, *_read(code, length, ZONES["head line 1"] + at)))
    good = _add_at_line_start(bb, *_read(0, 16, 9))
    for i in idx:
        bb.add_locus(*WINDOWS["A"], [i, good])
    bb.add_locus(*WINDOWS["A"], idx + [good])
    batch = bb.build()
    ok = checked_mask(batch)
    assert not ok[idx].any() and ok[good]
    assert _all_variants(ctx, orc, batch, f"op code {code}", code=B.INQ_ERR_CIGAR_OP) == B.INQ_ERR_CIGAR_OP
