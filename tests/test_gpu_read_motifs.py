"""The motif runs of the kept records at flush time (inq_call_flush_motifs, inq_read_motifs_fetch; read_motifs.hip launched behind
the slices' records): a SEQ-bearing BAM whose reads repeat their locus's motif with interruptions, through the device front end, against
the numpy restatement on the records the BAM was written from and against the kernel alone fed with what inq_read_seqs_fetch returned."""
import numpy as np
import pytest

from inquistr_amd import batch as B
from inquistr_amd import hipcall
from tests import gen
from tests import read_motif_case as rm
from tests import read_seq_case as rs
from tests.test_gpu_read_seqs import _append, _spans

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = hipcall.Context(0)
    assert c.backend.startswith("hip:gfx950")
    yield c
    c.close()


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("read_motifs")
    bam, bed, loci, recs, col4 = rm.make_motif_case(tmp, 93, n_loci=40)
    return bam, bed, [hipcall.encode_motif(t) for t in col4]


@pytest.mark.parametrize("unphased", [False, True])
def test_flush_with_motifs(ctx, case, unphased):
    bam, bed, target_words = case
    spans = _spans(bam, bed, unphased, 8_000)
    n_spans = len(spans)
    assert n_spans >= 2, "several spans in one batch"
    words = np.array([target_words[int(i)] for s in spans for i in s["locus_index"]], dtype=np.uint64)
    assert (words == 0).any() and len(set(int(w) for w in words)) > 4, "loci without a motif among those of several motifs"
    ctx.call_discard()
    codes, sizes = _append(ctx, spans, unphased)
    assert codes == [0] * n_spans
    n_loci = ctx.deferred_loci
    assert n_loci == len(words)
    out = ctx.call_flush_motifs(words)
    rc, p1, p2, ties, _ms, flags, ev, off, rec, org, raw, name_total, sq, packed, seq_total, mt = out
    assert rc == 0 and mt.dtype == hipcall.MOTIF_DTYPE and len(mt) == len(rec) == int(off[-1]) > 20
    # the restatement on the written records: record kk of locus j is a kept pair of j, its slice the window's
    written = [r for s in spans for r in rs.span_seq_records(s)]
    starts = np.concatenate([s["locus_start"] for s in spans])
    ends = np.concatenate([s["locus_end"] for s in spans])
    slices, rec_words = [], []
    for j in range(n_loci):
        for kk in range(int(off[j]), int(off[j + 1])):
            wds, pos, l_seq, codes_ = written[int(rec["read"][kk])]
            q, n = rs.window(wds, pos, l_seq, int(starts[j]), int(ends[j]))
            assert (q, n) == (int(sq["q_beg"][kk]), int(sq["n_bases"][kk]))
            slices.append(codes_[q : q + n])
            rec_words.append(int(words[j]))
    want = rm.records_of(slices, rec_words)
    assert mt.tobytes() == want.tobytes(), [(k, tuple(mt[k]), tuple(want[k])) for k in range(len(mt)) if tuple(mt[k]) != tuple(want[k])][:5]
    # what the case must hold for that to say anything
    assert any(len(c) == 0 for c in slices) and any(len(c) > 300 for c in slices), "SEQ `*` or an empty window; a long slice"
    assert (want["n_runs"] > 1).any() and (want["run_len"] >= 48).any(), "interruptions; a run over several words"
    assert any(w == 0 and len(c) for w, c in zip(rec_words, slices)), "a kept read with bases under a locus without a motif"
    # ... and the kernel alone, fed with what inq_read_seqs_fetch returned
    alone = ctx.motif_runs(sq, packed, off, words)
    assert alone.tobytes() == mt.tobytes()

    # motif NULL is exactly inq_call_flush_seqs, and offers no record
    codes, _ = _append(ctx, spans, unphased)
    a = ctx.call_flush_motifs(None)
    assert a[0] == 0 and len(a[15]) == 0 and ctx.read_motifs_fetch(1, check=False)[0] == B.INQ_ERR_ARG
    assert ctx.read_motifs_fetch(0, check=False)[0] == 0
    codes, _ = _append(ctx, spans, unphased)
    b = ctx.call_flush_seqs()
    for got in (a, b):
        rc_, p1_, p2_, ties_, _ms, flags_, ev_, off_, rec_, org_, raw_, total_, sq_, packed_, seq_total_ = got[:15]
        assert rc_ == 0 and gen.same_f64(p1, p1_) and gen.same_f64(p2, p2_) and ties == ties_ and np.array_equal(flags, flags_)
        assert ev.tobytes() == ev_.tobytes() and np.array_equal(off, off_) and rec.tobytes() == rec_.tobytes()
        assert org.tobytes() == org_.tobytes() and bytes(raw) == bytes(raw_) and name_total == total_
        assert sq.tobytes() == sq_.tobytes() and bytes(packed) == bytes(packed_) and seq_total == seq_total_
    assert ctx.read_motifs_fetch(1, check=False)[0] == B.INQ_ERR_ARG, "a flush without motifs offers none"

    # the records are there for the asking, in part; one more than the flush has is refused
    codes, _ = _append(ctx, spans, unphased)
    again = ctx.call_flush_motifs(words)
    assert again[0] == 0 and again[15].tobytes() == mt.tobytes()
    rc2, few = ctx.read_motifs_fetch(3, check=False)
    assert rc2 == 0 and few.tobytes() == mt[:3].tobytes()
    assert ctx.read_motifs_fetch(len(mt) + 1, check=False)[0] == B.INQ_ERR_ARG

    # a batch appended without sequences has no bases to measure - and stays
    codes, _ = _append(ctx, spans, unphased, seqs=False)
    assert codes == [0] * n_spans
    n = ctx.deferred_loci
    assert ctx.call_flush_motifs(words, check=False)[0] == B.INQ_ERR_ARG and ctx.deferred_loci == n
    assert ctx.call_flush_origins()[0] == 0
    ctx.call_discard()
