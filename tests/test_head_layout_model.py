"""`head_layout` of inquistr_amd/window_bytes.py, the model of the row walk's head phase (csrc/cigar_walk.h): its figures on
config #3, and the premise of the window-bounded walk for it on the oracle alone."""
import numpy as np
import pytest

from inquistr_amd import batch as B
from inquistr_amd import synth
from inquistr_amd import window_bytes as wb
from tests import gen


@pytest.fixture(scope="module")
def unphased4000():
    return synth.generate_numpy(synth.WORKLOADS["unphased100k"], 0, 4000)


def test_head_figures_on_config_3(unphased4000):
    """Lines of 128 bytes per locus, head steps per locus, and no read past the head's four lines: the figures DESIGN.md
    and profiles/r15_head_lines/summary.md quote.  11 096 is the floor test_line_pieces_model.py holds for "line_half" with
    a rule that knows every stop in advance: one line at a time, the stop tested after each, reaches it without a rule."""
    b = unphased4000
    groups, lines, head, steps = wb.head_layout(b)
    assert round(128 * int(lines.sum()) / b.n_loci) == 11096
    assert steps / b.n_loci == pytest.approx(14.27, abs=0.005)
    assert int(lines.max()) <= wb.HEAD_LINES and np.array_equal(head, lines), "every read ends inside the head"
    # the same groups as a read walked in half pieces from the start of its line, whatever the rule would have said
    _, groups_half, _, _ = wb._walked_pieces(b, 64, "line_half", (1 << 20, 1))
    assert np.array_equal(groups, groups_half)


def test_head_steps_follow_the_static_assignment():
    """Pair k of a 32-pair pass is row k % 8 of slot k // 8: a slot costs the most lines any of its eight reads needs."""
    bb = B.BatchBuilder(minlen=2, support=1, unphased=True)
    long_ = bb.add_read(900, B.encode_cigar([("M", 1)] * 128))  # 32 groups from group 0: four lines
    short = bb.add_read(900, B.encode_cigar([("M", 1)] * 32))  # one line
    empty = bb.add_read(900, np.zeros(0, dtype=np.uint32))
    bb.add_locus(1010, 1090, [short] * 8 + [long_] + [short] * 7 + [empty] * 8)  # slots of 1, 4 and 0 steps
    bb.add_locus(1010, 1090, [short] * 33)  # a second pass for pair 32: 4 + 1 slots of one step
    bb.add_locus(1010, 1090, [long_] * 65)  # blocks of 64 and 1 pairs: 8 + 1 slots of four steps
    batch = bb.build()
    gen.set_promise(batch, "none")
    groups, lines, head, steps = wb.head_layout(batch)
    assert steps == (1 + 4 + 0) + (4 + 1) + 4 * (8 + 1)
    assert groups.tolist()[:9] == [8] * 8 + [32] and lines.tolist()[8] == 4 and head.tolist()[8] == 4


def test_a_read_past_the_head_goes_on_in_two_line_pieces():
    """Reads of 60 groups of one-base ops at every start offset, stopped inside the head, behind it, and not at all."""
    def build(pos):
        bb = B.BatchBuilder(minlen=2, support=1, unphased=True)
        idx = []
        for skip in range(8):
            fill = (skip - bb._off4) % 8
            if fill:
                bb.add_read(0, B.encode_cigar([("M", 1)] * (4 * fill)))
            idx.append(bb.add_read(pos, B.encode_cigar([("M", 1)] * 240)))
        bb.add_locus(1010, 1090, idx)
        return bb.build()

    skips = np.arange(8)
    # pos + 1 + ops > end_ext = 1100 first at op 99 of the read, its group 24: the line that holds it is the last
    batch = build(1000)
    gen.set_promise(batch, "all")
    groups, lines, head, steps = wb.head_layout(batch)
    assert np.array_equal(groups, 8 * ((skips + 24) // 8 + 1) - skips) and np.array_equal(lines, (skips + 24) // 8 + 1)
    assert np.array_equal(head, lines) and steps == 4
    # ... at op 149, group 37: the head takes lines 0 - 3, one piece of two lines behind it the rest
    batch = build(950)
    gen.set_promise(batch, "all")
    groups, lines, head, steps = wb.head_layout(batch)
    assert np.array_equal(groups, 48 - skips) and lines.tolist() == [6] * 8 and head.tolist() == [4] * 8 and steps == 4
    gen.set_promise(batch, "none")
    groups, lines, head, steps = wb.head_layout(batch)
    assert groups.tolist() == [60] * 8 and head.tolist() == [4] * 8 and steps == 4
    assert np.array_equal(lines, (skips + 60 + 7) // 8)


def _cut_to_the_head_layout(batch):
    """tests/test_line_pieces_model.py _truncated_copy for `head_layout`: every pair's read cut to the groups the walk loads."""
    groups = wb.head_layout(batch)[0]
    r = batch.pair_read.astype(np.int64)
    reads = batch.reads[r].copy()
    g0 = reads["cigar_off4"].astype(np.int64)
    n_was = reads["n_cigar"].astype(np.int64)
    n = np.minimum(n_was, 4 * groups)
    off4 = np.concatenate([[0], np.cumsum((n + 3) // 4)])
    cig = np.zeros(4 * int(off4[-1]), dtype=np.uint32)
    for k in range(batch.n_pairs):
        cig[4 * off4[k] : 4 * off4[k] + n[k]] = batch.cigar[4 * g0[k] : 4 * g0[k] + n[k]]
    reads["cigar_off4"] = off4[:-1].astype(np.uint32)
    reads["n_cigar"] = n.astype(np.uint32)
    short = B.Batch(cigar=cig, reads=reads, pair_read=np.arange(batch.n_pairs, dtype=np.uint32), locus_pair_off=batch.locus_pair_off.copy(),
                    locus_start=batch.locus_start.copy(), locus_end=batch.locus_end.copy(), minlen=batch.minlen,
                    support=batch.support, unphased=batch.unphased)
    return short, int((n < n_was).sum())


def test_cutting_where_the_head_layout_stops_changes_nothing(orc):
    """Every pair's read, cut where `head_layout` says, gives the same rows, Calls, bits and ties."""
    cases = [(f"random_case {s}", gen.random_case(300 + s, n_loci=25, unphased=bool(s & 1), long_every=5)[0]) for s in range(3)]
    cases += [(f"row_walk_case {s}", gen.row_walk_case(s, max_depth=300)[0]) for s in range(8)]
    total_cut = 0
    for name, batch in cases:
        gen.set_promise(batch, "all")
        code, want = orc.call_batch(batch, debug=True)
        short, cut = _cut_to_the_head_layout(batch)
        assert wb.checked_mask(short).all()
        code2, got = orc.call_batch(short, debug=True)
        assert code == code2 == B.INQ_OK
        assert np.array_equal(got.pair_call, want.pair_call) and np.array_equal(got.pair_bits, want.pair_bits), name
        assert gen.same_f64(got.phase1, want.phase1) and gen.same_f64(got.phase2, want.phase2) and got.n_tie_loci == want.n_tie_loci, name
        total_cut += cut
    assert total_cut > 1000
