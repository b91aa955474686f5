"""The piece layouts of inquistr_amd/window_bytes.py: their byte and row-step counts on config #3, and the premise of the
window-bounded walk for each of them on the oracle alone."""
import numpy as np
import pytest

from inquistr_amd import batch as B
from inquistr_amd import synth
from inquistr_amd import window_bytes as wb
from tests import gen


@pytest.fixture(scope="module")
def unphased4000():
    return synth.generate_numpy(synth.WORKLOADS["unphased100k"], 0, 4000)


def _per_locus(batch, layout, **kw):
    return wb.window_bounded_line_bytes(batch, layout=layout, **kw) / batch.n_loci


def test_layout_read_is_what_the_functions_gave(unphased4000):
    b = unphased4000
    g0, groups = wb._walked_groups(b, 64)
    g0r, groupsr = wb._walked_groups(b, 64, "read")
    g0s, groupss, pieces, _ = wb._walked_pieces(b, 64, "read")  # the piece-by-piece walk against the closed form
    assert np.array_equal(g0, g0r) and np.array_equal(groups, groupsr)
    assert np.array_equal(g0, g0s) and np.array_equal(groups, groupss) and np.array_equal(pieces, (groups + 15) // 16)
    assert wb.window_bounded_line_bytes(b) == wb.window_bounded_line_bytes(b, layout="read")
    assert wb.window_bounded_cigar_bytes(b) == wb.window_bounded_cigar_bytes(b, layout="read") == 16 * int(groups.sum())


def test_table_counts_on_config_3(unphased4000):
    """Bytes per locus in whole 128-byte lines and row-steps per locus, to the figures that
    profiles/r08_line_pieces/summary.md and DESIGN.md quote.  The issue's rows A (14 589), B (13 696) and C (11 096: every
    later piece a half piece, the stop known in advance) reproduce.  Its row D (11 889 at factor 0.85) does not: the rule
    as the issue writes it gives 11 393 there, which is what is held."""
    b = unphased4000

    def lines(layout, factor=(wb.HALF_NUM, wb.HALF_DEN)):
        g0, groups, _, _ = wb._walked_pieces(b, 64, layout, factor)
        n = np.where(groups > 0, ((g0 + groups) * 16 + 127) // 128 - (g0 * 16) // 128, 0)
        return round(128 * int(n.sum()) / b.n_loci)

    assert lines("read") == round(_per_locus(b, "read")) == 14589
    assert lines("line") == round(_per_locus(b, "line")) == 13696
    assert lines("line_half", (1 << 20, 1)) == 11096
    assert lines("line_half", (17, 20)) == 11393
    assert lines("line_half") == round(_per_locus(b, "line_half")) == 11354
    assert lines("tail") == round(_per_locus(b, "tail")) == 13035  # what the kernel does
    assert lines("tail_half") == round(_per_locus(b, "tail_half")) == 11764
    assert round(wb.window_bounded_cigar_bytes(b, layout="tail") / b.n_loci) == 10451
    steps = {layout: wb.row_steps(b, layout) / b.n_loci for layout in wb.LAYOUTS}
    quoted = {"read": 11.46, "line": 13.87, "line_half": 13.94, "tail": 11.46, "tail_half": 11.53}  # to two decimals
    assert steps == pytest.approx(quoted, abs=0.005)
    assert steps["tail"] == steps["read"]


def test_half_piece_rule_is_integer_and_saturates():
    d = np.array([0, 100, 280, 281, 1 << 30], dtype=np.int64)
    assert list(wb.half_piece_next(d, 16, 640)) == [True, True, True, False, False]  # d * 128 <= 7 * 640 * 8
    assert list(wb.half_piece_next(d, 16, 1 << 40)) == [True, True, True, True, False]  # rtot saturates at 2^24 - 1
    assert bool(wb.half_piece_next(5, 16, 100, c=1)) and not bool(wb.half_piece_next(6, 16, 100, c=1))


def _truncated_copy(batch, layout):
    """tests/test_window_bytes.py _truncated_copy for a layout: every pair's read cut to the groups the walk loads."""
    g0, groups = wb._walked_groups(batch, 64, layout)
    r = batch.pair_read.astype(np.int64)
    reads = batch.reads[r].copy()
    n = np.minimum(reads["n_cigar"].astype(np.int64), 4 * groups)
    n4 = (n + 3) // 4
    off4 = np.concatenate([[0], np.cumsum(n4)])
    cig = np.zeros(4 * int(off4[-1]), dtype=np.uint32)
    for k in range(batch.n_pairs):
        cig[4 * off4[k] : 4 * off4[k] + n[k]] = batch.cigar[4 * g0[k] : 4 * g0[k] + n[k]]
    reads["cigar_off4"] = off4[:-1].astype(np.uint32)
    reads["n_cigar"] = n.astype(np.uint32)
    short = B.Batch(cigar=cig, reads=reads, pair_read=np.arange(batch.n_pairs, dtype=np.uint32), locus_pair_off=batch.locus_pair_off.copy(),
                    locus_start=batch.locus_start.copy(), locus_end=batch.locus_end.copy(), minlen=batch.minlen,
                    support=batch.support, unphased=batch.unphased)
    return short, int((n < reads_n(batch, r)).sum())


def reads_n(batch, r):
    return batch.reads["n_cigar"].astype(np.int64)[r]


@pytest.mark.parametrize("layout", ["line", "line_half", "tail", "tail_half"])
def test_cutting_where_the_layout_stops_changes_nothing(orc, layout):
    """Every pair's read, cut where `_walked_groups` of the layout says, gives the same rows, Calls, bits and ties."""
    cases = [(f"random_case {s}", gen.random_case(300 + s, n_loci=25, unphased=bool(s & 1), long_every=5)[0]) for s in range(3)]
    cases += [(f"row_walk_case {s}", gen.row_walk_case(s, max_depth=300)[0]) for s in range(8)]
    total_cut = 0
    for name, batch in cases:
        gen.set_promise(batch, "all")
        code, want = orc.call_batch(batch, debug=True)
        short, cut = _truncated_copy(batch, layout)
        assert wb.checked_mask(short).all()
        code2, got = orc.call_batch(short, debug=True)
        assert code == code2 == B.INQ_OK
        assert np.array_equal(got.pair_call, want.pair_call) and np.array_equal(got.pair_bits, want.pair_bits), name
        assert gen.same_f64(got.phase1, want.phase1) and gen.same_f64(got.phase2, want.phase2) and got.n_tie_loci == want.n_tie_loci, name
        total_cut += cut
    assert total_cut > 1000
