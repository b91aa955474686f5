"""The device record scan (csrc/bam_scan.hip) on hand-built BAM records and spans no writer emits.

The spans come from tests/test_bam_craft.py (corpus(), tile_span(), big_span()), where what each one reaches and what three CPU
parsers make of it are pinned without a GPU.  Here every span goes through inq_call_span.  A clean span must come back with the
restatement's batch - every descriptor with its bits, phase and promise, every CIGAR word with its zero padding, every
locus' list - and with the rows the C oracle computes on that batch; a span the scan refuses with the code, the FS_* bits and
the record index of bam_craft.verdict, after which the same context calls a clean span.
"""
import time

import numpy as np
import pytest

from inquistr_amd import batch as B
from inquistr_amd import hipcall
from tests import bam_craft as bc
from tests import gen
from tests import test_bam_craft as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = hipcall.Context(0)
    yield c
    c.close()


def _same_batch(dev, b: B.Batch, per_locus: bool):
    cigar, reads, pair_read, off = dev
    assert np.array_equal(cigar, b.cigar)  # the zero padding of every read's last unit included
    for f in ("cigar_off4", "n_cigar", "pos", "mapq", "bits", "promise"):
        bad = np.flatnonzero(reads[f] != b.reads[f])
        assert not len(bad), (f, bad[:8], reads[f][bad[:8]], b.reads[f][bad[:8]])
    has_hp = (b.reads["bits"] & B.INQ_READ_HAS_HP) != 0
    assert np.array_equal(reads["phase"][has_hp], b.reads["phase"][has_hp])
    assert np.array_equal(off, b.locus_pair_off)
    if per_locus:
        ref = T.batch_arrays(b)
        for j in range(b.n_loci):
            assert T.locus_view(dev, j) == T.locus_view(ref, j), j
    assert np.array_equal(pair_read, b.pair_read)


def _check_clean(ctx, sp, w: T.Want, per_locus: bool = True):
    rc, p1, p2, _ties, stats = ctx.call_span(*bc.call_args(sp), check=False)
    b = w.batch
    assert rc == w.code, (rc, hex(stats.front_status), int(stats.first_bad_record))
    assert (int(stats.n_reads), int(stats.n_pairs), int(stats.n_cigar_words)) == (b.n_reads, b.n_pairs, len(b.cigar))
    _same_batch(ctx.span_fetch_batch(stats, b.n_loci), b, per_locus)
    if w.code == 0:
        assert gen.same_f64(p1, w.phase1) and gen.same_f64(p2, w.phase2)


@pytest.mark.parametrize("name", T.CLEAN)
def test_clean_crafted_span(ctx, name):
    """One call per case; the gather group under both store policies of cigar_gather_kernel."""
    c = T.case(name)
    t0 = time.perf_counter()
    try:
        for nt in (1, 0) if c.group == "gather" else (1,):
            ctx.set_option("gather_nt", nt)
            _check_clean(ctx, c.span, T.want(c))
    finally:
        ctx.set_option("gather_nt", 1)
    print(f"{name}: {time.perf_counter() - t0:.3f} s")


@pytest.mark.parametrize("name", T.REFUSED)
def test_refused_crafted_span(ctx, name):
    c = T.case(name)
    bits, first, code = bc.verdict(c.span)
    rc, _p1, _p2, _ties, stats = ctx.call_span(*bc.call_args(c.span), check=False)
    assert rc == code and int(stats.front_status) == bits, (rc, hex(stats.front_status))
    if bits != bc.FS_CHAIN:
        assert int(stats.first_bad_record) == first
    clean = T.case("join_edges")  # the context is not left behind in the refused span's state
    _check_clean(ctx, clean.span, T.want(clean))


@pytest.mark.parametrize("n", T.TILE_SIZES)
def test_scans_at_the_tile_edges(ctx, n):
    sp = T.tile_span(n)
    batch, _off, _names = bc.stanza_expect(sp)
    _check_clean(ctx, sp, T.want_of_span(f"tiles_{n}", sp, batch), per_locus=n < 4097)


def test_scans_beyond_256_tiles_anchor_per_record(ctx):
    """256 * 4096 + 4097 records with an anchor each: scan_totals carries a running value into its second chunk in the scans over
    anchors, records (CIGAR units, the running maximum of the end keys) alike."""
    t0 = time.perf_counter()
    sp = T.big_span(1)
    batch, _off, _names = bc.stanza_expect(sp)
    w = T.want_of_span("big_anchor_per_record", sp, batch)
    t1 = time.perf_counter()
    _check_clean(ctx, sp, w, per_locus=False)
    print(f"big span: host build {t1 - t0:.2f} s, device call and comparison {time.perf_counter() - t1:.2f} s")


def test_scans_beyond_256_tiles_deferred_with_names(ctx):
    """The same records with an anchor at every 4097th, appended with names: the scan over the name lengths and the gather of
    the names ride along; name_off is the cumulative sum of max(l_read_name, 1) - 1."""
    t0 = time.perf_counter()
    sp = T.big_span(4097)
    batch, name_off, names = bc.stanza_expect(sp)
    w = T.want_of_span("big_anchor_every_4097th", sp, batch)
    t1 = time.perf_counter()
    ctx.call_discard()
    rc, stats = ctx.call_span_deferred(*bc.call_args(sp), check=False, names=True)
    assert rc == 0, (rc, hex(stats.front_status))
    assert (int(stats.n_reads), int(stats.n_pairs), int(stats.n_cigar_words)) == (batch.n_reads, batch.n_pairs, len(batch.cigar))
    rc, p1, p2, _ties, _ms = ctx.call_flush(check=False)
    assert rc == w.code == 0 and gen.same_f64(p1, w.phase1) and gen.same_f64(p2, w.phase2)
    got_off, got_names = ctx.span_fetch_names(batch.n_reads, cap_bytes=len(names))
    assert np.array_equal(got_off, name_off)
    assert got_names.tobytes() == names
    _same_batch(ctx.span_fetch_batch(stats, batch.n_loci), batch, per_locus=False)
    print(f"big span, deferred with names: host build {t1 - t0:.2f} s, device calls and comparison {time.perf_counter() - t1:.2f} s")
