"""The window walk on the GPU (seq_window_kernel of read_seqs.hip through inq_seq_windows): q_beg and n_bases of every (locus, read)
pair of hand-built batches against the Q(x) formula of tests/read_seq_case.py.  The shapes are the kernel's own: CIGARs around the
64-op piece, window edges on ops and on pieces, loci around the four pairs of a wave and the sixteen of a workgroup."""
import numpy as np
import pytest

from inquistr_amd import batch as B
from inquistr_amd import hipcall
from inquistr_amd.batch import BatchBuilder
from tests import gen
from tests import read_seq_case as rs
from tests.test_read_seqs_host import EDGE

pytestmark = pytest.mark.gpu

START, END = 1000, 1050
SE, EE = START - 10, END + 10


@pytest.fixture(scope="module")
def ctx():
    c = hipcall.Context(0)
    assert c.backend.startswith("hip:gfx950")
    yield c
    c.close()


def _check(c, batch, l_seq=None, what=""):
    want_q, want_n = rs.batch_windows(batch, l_seq)
    q, n = c.seq_windows(batch, l_seq)
    assert q.dtype == np.uint32 and n.dtype == np.uint32 and len(q) == len(n) == batch.n_pairs
    bad = np.nonzero((q != want_q) | (n != want_n))[0]
    assert len(bad) == 0, (what, int(bad[0]), int(q[bad[0]]), int(n[bad[0]]), int(want_q[bad[0]]), int(want_n[bad[0]]))
    return q, n


def _ops(n, first=0):
    """n ops, M runs of 1 - 3 bases between I, D and S ops of 1 - 4: (words, reference span, query length)"""
    k = np.arange(first, first + n)
    op = np.where(k % 2 == 0, 0, np.array([1, 2, 4, 1, 2])[(k // 2) % 5])
    ln = np.where(op == 0, 1 + k % 3, 1 + k % 4)
    words = ((ln << 4) | op).astype(np.uint32)
    return words, int(ln[np.isin(op, rs.REF_OPS)].sum()), int(ln[np.isin(op, rs.M_OPS + rs.IS_OPS)].sum())


def _edge_batch():
    """Every read of the CPU edge list, CIGARs of every length around the piece, reads whose 64th op ends exactly on se or on ee - 1,
    and loci of 0, 1, 4, 5, 64, 65 and 300 pairs over them: the main window, shifted and narrow ones, one without width."""
    bb = BatchBuilder(minlen=5, support=3, unphased=True)
    l_seq = []
    reads = []

    def add(words, pos, ls):
        reads.append(bb.add_read(pos, words))
        l_seq.append(ls)
        return reads[-1]

    for _name, cigar, pos, ls in EDGE:
        add(rs.words_of(cigar), pos, ls)
    for n in (0, 1, 63, 64, 65, 128, 129, 5000):
        w, span, qlen = _ops(n)
        add(w, SE - span // 2, qlen)       # the window somewhere in the middle of the read
        add(w, EE - 1 - span, qlen)        # the read ends exactly on ee - 1
        add(w, SE - span, max(0, qlen - 3))  # ... on se, SEQ a little short
    for n_first in (64, 128):  # r = se, and r = ee - 1, after exactly one and two pieces; ops follow that must (not) count
        w, span, _q = _ops(n_first)
        tail = rs.words_of([("I", 7), ("M", 30), ("S", 11), ("M", 200)])
        both = np.concatenate([w, tail])
        qlen = int((both >> 4)[np.isin(both & 15, rs.M_OPS + rs.IS_OPS)].sum())
        add(both, SE - span, qlen)
        add(both, EE - 1 - span, qlen)
        add(both, EE - 2 - span, qlen)
    big = (1 << 28) - 1
    # sixteen N of 2^28 - 1 take the position 16 short of 2^32 past its start inside one piece: in 32 bits the I behind them would lie
    # in front of the window; twenty S of that length in front of it take Q(se) past 2^32
    add(rs.words_of([("M", 100)] + [("N", big)] * 16 + [("I", 5), ("M", 50)]), 500, 155)
    add(rs.words_of([("S", big)] * 20 + [("M", 5000)]), 10, 4_000_000_000)
    add(rs.words_of([("M", 100)] * 200), -1, 20_000)
    pool = list(reads)
    rng = np.random.default_rng(7)
    windows = [(START, END), (START - 25, END - 25), (START + 15, END + 15), (EE - 15, EE - 14), (START, START)]
    bb.add_locus(START, END, pool)  # every read once under the main window
    bb.add_locus(START, END, [])
    for k, depth in enumerate((1, 4, 5, 64, 65, 300, 0, 16, 17)):
        s, e = windows[k % len(windows)]
        idx = [int(x) for x in rng.choice(pool, size=depth)]  # with replacement: a read may be offered twice to one locus
        if depth >= 4:
            idx[1] = idx[0]
        bb.add_locus(s, e, idx)
    bb.add_locus(5, 4294967290, pool[:7])  # end + 10 wraps
    bb.add_locus(9, 60, pool[:5])          # start < 10
    bb.add_locus(0, 5, pool[:5])
    bb.add_locus(START, END, pool[-3:])    # the batch's last pairs
    return bb.build(), np.array(l_seq, dtype=np.uint32)


def test_edge_batch(ctx):
    batch, l_seq = _edge_batch()
    depths = np.diff(batch.locus_pair_off.astype(np.int64))
    assert {0, 1, 4, 5, 64, 65, 300} <= set(int(d) for d in depths)
    q, n = _check(ctx, batch, l_seq, "with l_seq")
    assert (q.astype(np.int64) + n <= l_seq[batch.pair_read]).all()
    assert n.max() > 0 and (n == 0).any()
    # a window without width gives (0, 0) whatever the read
    for j in np.nonzero((batch.locus_start < 10) | (batch.locus_end > 4294967285))[0]:
        p0, p1 = int(batch.locus_pair_off[j]), int(batch.locus_pair_off[j + 1])
        assert p1 > p0 and not q[p0:p1].any() and not n[p0:p1].any()
    # no cut: what the CIGAR alone says
    q2, n2 = _check(ctx, batch, None, "without l_seq")
    assert (n2 >= n).all() and (n2 > n).any()


def test_promise_changes_nothing(ctx):
    batch, l_seq = _edge_batch()
    base = ctx.seq_windows(batch, l_seq)
    for name in gen.promise_variants(batch, ("all", "half", "none")):
        got = ctx.seq_windows(batch, l_seq)
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1]), name


def test_indices_outside_the_batch(ctx):
    """a pair whose read index lies outside the batch, and a read whose CIGAR extent does, give (0, 0); their neighbours are untouched"""
    batch, l_seq = _edge_batch()
    want_q, want_n = rs.batch_windows(batch, l_seq)
    batch.pair_read = batch.pair_read.copy()
    batch.reads = batch.reads.copy()
    hit = [3, 40, batch.n_pairs - 1]
    for p in hit:
        batch.pair_read[p] = batch.n_reads + (p % 2) * 1000
    victim = int(batch.pair_read[10])
    batch.reads["cigar_off4"][victim] = batch.cigar.shape[0] // 4  # one group past the end (the read has ops)
    assert batch.reads["n_cigar"][victim] > 0
    gone = np.zeros(batch.n_pairs, dtype=bool)
    gone[hit] = True
    gone |= batch.pair_read == victim
    q, n = ctx.seq_windows(batch, l_seq)
    assert not q[gone].any() and not n[gone].any()
    assert np.array_equal(q[~gone], want_q[~gone]) and np.array_equal(n[~gone], want_n[~gone])


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4, 7])
def test_row_walk_cases(ctx, seed):
    """tests.gen.row_walk_case: reads that stop on every multiple of 64 ops, every op code, pos = -1, windows of width 0 to 40 000"""
    batch, _info = gen.row_walk_case(seed)
    _check(ctx, batch, None, f"row_walk_case {seed}")
    qlen = np.array([int((w >> 4)[np.isin(w & 15, rs.M_OPS + rs.IS_OPS)].sum()) for w in (rs.read_words(batch, r) for r in range(batch.n_reads))],
                    dtype=np.int64)
    l_seq = np.where(np.arange(batch.n_reads) % 5 == 0, qlen // 2, qlen).astype(np.uint32)
    _check(ctx, batch, l_seq, f"row_walk_case {seed} with l_seq")


@pytest.mark.parametrize("n_loci", rs.SEARCH_LOCUS_COUNTS)
def test_locus_search_steps(ctx, n_loci):
    """a pair's locus where the sixteen-probe search takes one to four steps: one or two pairs in the first locus, the last and on each
    side of the probes' boundaries (read_seq_case.search_probe_loci), every other locus empty.  All pairs are one read of 200M; every
    locus has a window of its own inside it, so a pair that took a neighbour's locus shows in q_beg and in n_bases"""
    bb = BatchBuilder(minlen=5, support=3, unphased=True)
    read = bb.add_read(950, rs.words_of([("M", 200)]))
    filled = rs.search_probe_loci(n_loci)
    rank = {j: i for i, j in enumerate(filled)}
    for j in range(n_loci):
        start = START + 3 * j % 97
        bb.add_locus(start, start + 10 + rank.get(j, 0) % 7, [read] * (1 + rank[j] % 2) if j in rank else [])
    batch = bb.build()
    assert batch.n_loci == n_loci and len(filled) <= batch.n_pairs <= 2 * len(filled)
    q, n = _check(ctx, batch, np.array([200], dtype=np.uint32), f"{n_loci} loci")
    first = batch.locus_pair_off[filled].astype(np.int64)  # a filled locus's first pair
    assert n.min() >= 29 and (np.diff(q[first].astype(np.int64)) != 0).all(), "neighbours among the filled loci differ in q_beg"


def test_empty_batches(ctx):
    bb = BatchBuilder(unphased=True)
    q, n = ctx.seq_windows(bb.build())
    assert len(q) == 0 and len(n) == 0
    bb.add_read(100, rs.words_of([("M", 50)]))
    bb.add_locus(START, END, [])
    q, n = ctx.seq_windows(bb.build())
    assert len(q) == 0 and len(n) == 0
    batch, _ = _edge_batch()
    off = batch.locus_pair_off.copy()
    off[1] = off[2] + 1  # offsets that do not ascend
    batch.locus_pair_off = off
    assert ctx.seq_windows(batch, check=False)[0] == B.INQ_ERR_ARG
