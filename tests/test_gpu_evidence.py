"""Per-locus read evidence on the GPU (inq_locus_evidence_t): the *_evidence entry points against records derived from the ORACLE's
per-pair outputs (hand-written ones for a hand-built locus) over every path of the counting kernels, and `--evidence` end to end
through both front ends and several devices against a plain-Python restatement."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from inquistr_amd import batch as B
from inquistr_amd import call, hipcall
from oracle import pyoracle as py
from tests import gen
from tests.test_tie_report import row_order

pytestmark = pytest.mark.gpu

EV = hipcall.EVIDENCE_DTYPE
HEADER = "chrom\tbegin\tend\tfetched\tkept\th1\th2\tclipped\tmin\tmax"


@pytest.fixture(scope="module")
def ctx():
    c = hipcall.Context(0)
    assert c.backend.startswith("hip:gfx950")
    yield c
    c.close()


# ---- expected records: from the oracle's per-pair outputs, never from the library ------------------------------------------------
def expected_evidence(batch, want):
    """inq_locus_evidence_t of every locus from pair_bits / pair_call of an oracle run (debug=True) and the descriptors' phase."""
    ev = np.zeros(batch.n_loci, dtype=EV)
    off = batch.locus_pair_off.astype(np.int64)
    bits = want.pair_bits.astype(np.int64)
    phase = batch.reads["phase"][batch.pair_read].astype(np.int64)
    for j in range(batch.n_loci):
        a, b = off[j], off[j + 1]
        bj, cj = bits[a:b], want.pair_call[a:b]
        kept = (bj & 4) != 0
        n_kept = int(kept.sum())
        if batch.unphased:
            g1, g2, grouped = n_kept // 2, n_kept - n_kept // 2, kept
        else:
            pj = phase[a:b]
            g1, g2 = int((kept & (pj == 1)).sum()), int((kept & (pj == 2)).sum())
            grouped = kept & ((pj == 1) | (pj == 2))
        some = bool(grouped.any())
        ev[j] = (int(((bj & 2) != 0).sum()), n_kept, g1, g2, int((grouped & ((bj & 1) != 0)).sum()), 0,
                 int(cj[grouped].min()) if some else 0, int(cj[grouped].max()) if some else 0)
    return ev


_ORACLE = {}


def _oracle(orc, key, batch):
    """(oracle Result with per-pair outputs, expected records) of a batch, computed once per module"""
    if key not in _ORACLE:
        oc, want = orc.call_batch(batch, debug=True, threads=8)
        assert oc == 0
        _ORACLE[key] = (want, expected_evidence(batch, want))
    return _ORACLE[key]


def _assert_records(got_ev, exp, what=""):
    assert got_ev.dtype == EV and got_ev.shape == exp.shape
    if got_ev.tobytes() != exp.tobytes():
        bad = [j for j in range(len(exp)) if got_ev[j].tobytes() != exp[j].tobytes()]
        raise AssertionError(f"{what}: {len(bad)} records differ, first {bad[0]}: got {got_ev[bad[0]]}, want {exp[bad[0]]}")


def _assert_properties(batch, res, ev):
    """phaseN is NaN exactly when n_groupN < support; the counts nest"""
    assert np.array_equal(np.isnan(res.phase1), ev["n_group1"] < batch.support)
    assert np.array_equal(np.isnan(res.phase2), ev["n_group2"] < batch.support)
    g = ev["n_group1"].astype(np.int64) + ev["n_group2"]
    assert np.all(ev["n_fetched"] >= ev["n_kept"]) and np.all(ev["n_kept"] >= g) and np.all(g >= ev["n_clip"])
    assert not ev["reserved"].any()
    assert np.all((g > 0) | ((ev["call_min"] == 0) & (ev["call_max"] == 0))) and np.all(ev["call_min"] <= ev["call_max"])


def _device_call(ctx, batch, evidence=True, pair_outputs=True, check=True):
    """The batch through inq_call_batch_device_evidence with torch tensors, on torch's stream.  Returns (code of the enqueue, status
    code, Result, flags, evidence); the evidence and the flags start as 0xFF bytes."""
    import torch

    dev = torch.device("cuda:0")

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)

    t = {k: up(getattr(batch, k)) for k in ("cigar", "reads", "pair_read", "locus_pair_off", "locus_start", "locus_end")}
    n = max(batch.n_loci, 1)
    p1 = torch.full((n,), 7.0, dtype=torch.float64, device=dev)
    p2 = torch.full((n,), 7.0, dtype=torch.float64, device=dev)
    pc = torch.zeros(max(batch.n_pairs, 1), dtype=torch.int64, device=dev)
    pb = torch.zeros(max(batch.n_pairs, 1), dtype=torch.uint8, device=dev)
    fl = torch.full((n,), 0xFF, dtype=torch.uint8, device=dev)
    ev = torch.full((n * EV.itemsize,), 0xFF, dtype=torch.uint8, device=dev)
    b = B.InqBatchC()
    b.n_reads, b.n_cigar_words, b.n_pairs, b.n_loci = batch.n_reads, int(batch.cigar.shape[0]), batch.n_pairs, batch.n_loci
    for k, v in t.items():
        setattr(b, k, v.data_ptr())
    b.minlen, b.support, b.unphased, b.reserved = int(batch.minlen), int(batch.support), int(batch.unphased), 0
    r = B.InqResultC(p1.data_ptr(), p2.data_ptr(), pc.data_ptr() if pair_outputs else None, pb.data_ptr() if pair_outputs else None, 0)
    torch.cuda.synchronize()  # the uploads and fills are there: the enqueue below does not wait for torch's own work
    code = ctx.call_batch_device_evidence(b, r, fl.data_ptr(), ev.data_ptr() if evidence else None, torch.cuda.current_stream().cuda_stream,
                                          check=check)
    rc, ties = ctx.status()  # (waits for the device)
    res = B.Result(phase1=p1.cpu().numpy()[: batch.n_loci], phase2=p2.cpu().numpy()[: batch.n_loci], pair_call=pc.cpu().numpy()[: batch.n_pairs],
                   pair_bits=pb.cpu().numpy()[: batch.n_pairs], n_tie_loci=ties)
    return code, rc, res, fl.cpu().numpy()[: batch.n_loci], ev.cpu().numpy().view(EV)[: batch.n_loci]


def _check_both_entries(ctx, batch, want, exp, what):
    """Host entry and device entry with evidence: the oracle-derived records, every byte written; rows, flags and tie count those of
    the same call without evidence."""
    rc0, plain, flags0 = ctx.call_batch_flags(batch, debug=True)
    assert rc0 == 0
    rc, got, flags, ev = ctx.call_batch_evidence(batch, debug=True)
    assert rc == 0, what
    _assert_records(ev, exp, what + " host entry")
    code, rc2, got2, flags2, ev2 = _device_call(ctx, batch)
    assert code == 0 and rc2 == 0, what
    _assert_records(ev2, exp, what + " device entry")
    for g, f in ((got, flags), (got2, flags2)):
        assert gen.same_f64(g.phase1, plain.phase1) and gen.same_f64(g.phase2, plain.phase2), what
        assert np.array_equal(f, flags0) and g.n_tie_loci == plain.n_tie_loci == int(flags0.sum()), what
        assert np.array_equal(g.pair_call, want.pair_call) and np.array_equal(g.pair_bits, want.pair_bits), what
        _assert_properties(batch, g, exp)
    # without flags, without per-pair outputs of the caller's: the same records
    rc3, got3, none, ev3 = ctx.call_batch_evidence(batch, debug=False, flags=False)
    assert rc3 == 0 and none is None and got3.pair_call is None
    _assert_records(ev3, exp, what + " host entry, nothing else asked for")
    assert gen.same_f64(got3.phase1, plain.phase1) and gen.same_f64(got3.phase2, plain.phase2)


# ---- a hand-built locus -----------------------------------------------------------------------------------------------------------
def _hand_built(unphased):
    """Locus 0 = chr:1000-1050 (window 990 .. 1060, minlen 5) with one read of every kind the record tells apart; locus 1 has no pairs;
    every read of locus 2 is fetched and filtered (mapq 5)."""
    bb = B.BatchBuilder(minlen=5, support=3, unphased=unphased)
    enc = B.encode_cigar
    reads = [
        # (pos, cigar, mapq, phase, is_2d)                                          unphased          phased
        (100, [("M", 50)], 60, 1, False),                      # ends at 150: not fetched
        (900, [("M", 300)], 10, 1, False),                     # mapq 10                   fetched only      fetched only
        (900, [("M", 130)], 60, 2, False),                     # ends inside the window    fetched only      kept, HP 2, Span 0
        (900, [("M", 300)], 60, None, False),                  # no HP                     kept, Span 0      fetched only
        (900, [("M", 300)], 60, 0, False),                     # HP 0                      kept, Span 0      kept, no group
        (900, [("M", 120), ("I", 12), ("M", 180)], 60, 1, False),  # HP 1                  kept, Span 12     HP 1, Span 12
        (900, [("M", 120), ("D", 20), ("M", 180)], 60, 2, False),  # a negative Call        kept, Span -20    HP 2, Span -20
        (900, [("M", 110), ("I", 7), ("M", 190)], 60, 1, False),   #                        kept, Span 7      HP 1, Span 7
        (900, [("M", 300)], 11, 2, False),                     # mapq 11 passes            kept, Span 0      HP 2, Span 0
        (990, [("S", 10), ("M", 200)], 60, 2, False),          # a soft clip in the window kept, Clip 10     HP 2, Clip 10
        (990, [("S", 10), ("M", 200)], 60, 1, True),           # ... of a 2D read: ignored kept, Span 0      HP 1, Span 0
    ]
    idx = [bb.add_read(pos, enc(cig), mapq=mq, phase=ph, is_2d=twod) for pos, cig, mq, ph, twod in reads]
    bb.add_locus(1000, 1050, idx)
    bb.add_locus(2000, 2050, [])
    idx = [bb.add_read(2900, enc([("M", 300)]), mapq=5, phase=1 + k % 2) for k in range(3)]
    bb.add_locus(3000, 3050, idx)
    want = np.zeros(3, dtype=EV)
    #          fetched kept h1 h2 clip - min max
    want[0] = (10, 8, 4, 4, 1, 0, -20, 12) if unphased else (10, 8, 3, 4, 1, 0, -20, 12)
    want[2] = (3, 0, 0, 0, 0, 0, 0, 0)
    return bb.build(), want


@pytest.mark.parametrize("unphased", [False, True])
def test_hand_built_locus(ctx, orc, unphased):
    batch, by_hand = _hand_built(unphased)
    want, exp = _oracle(orc, ("hand", unphased), batch)
    _assert_records(exp, by_hand, "the oracle-derived records against the hand-written ones")
    _check_both_entries(ctx, batch, want, by_hand, f"hand-built unphased={unphased}")
    rc, got, _flags, ev = ctx.call_batch_evidence(batch)
    # h1 of the phased form has exactly `support` Calls, locus 2 none: a number and a NaN
    assert not np.isnan(got.phase1[0]) and np.isnan(got.phase1[1]) and np.isnan(got.phase1[2])


# ---- random batches ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unphased", [False, True])
@pytest.mark.parametrize("n_loci", [1, 3, 4, 5, 40])
def test_random_batches(ctx, orc, n_loci, unphased):
    """n_loci 1, 3, 5: the last workgroup of the first launch has idle waves; 4: none."""
    for seed in (11, 12, 13):
        batch, _ = gen.random_case(990_000 + seed, n_loci=n_loci, unphased=unphased)
        want, exp = _oracle(orc, ("random", seed, n_loci, unphased), batch)
        _check_both_entries(ctx, batch, want, exp, f"random seed={seed} n_loci={n_loci} unphased={unphased}")


# ---- every depth class ------------------------------------------------------------------------------------------------------------
LADDER_SEED = 31


def _ladder(orc, unphased):
    batch, depths = gen.depth_ladder_case(LADDER_SEED, unphased, 3)
    return (batch, depths) + _oracle(orc, ("ladder", unphased), batch)


@pytest.mark.parametrize("unphased", [False, True])
def test_depth_classes(ctx, orc, unphased):
    """One locus at each of 0, 1, 64, 65, 256, 257, 2 048, 2 049, 16 384, 16 385, ..., 65 537, 70 001 pairs: one wave, one slice, and
    two to five slices merged with the last arriver writing the totals."""
    batch, depths, want, exp = _ladder(orc, unphased)
    for d in (0, 1, 256, 257, 16_384, 16_385, 65_537, 70_001):
        assert d in depths
    # the case reaches every field on the deep side too
    deep = np.array(depths) > 16_384
    assert exp["n_clip"][deep].all() and (exp["n_fetched"][deep] > exp["n_kept"][deep]).all() and (exp["call_min"][deep] < 0).all()
    if not unphased:
        assert (exp["n_kept"][deep] > exp["n_group1"][deep] + exp["n_group2"][deep]).all()
    _check_both_entries(ctx, batch, want, exp, f"ladder unphased={unphased}")


@pytest.mark.parametrize("unphased", [False, True])
def test_depth_hint_skips_the_second_launch(ctx, orc, unphased):
    """max_reads_hint = 256 on a batch that honours it (loci of 250 .. 253 pairs), through the device entry, where the option holds"""
    batch = gen.all_listed_case(9, 250, unphased=unphased)
    assert int(np.diff(batch.locus_pair_off.astype(np.int64)).max()) <= 256
    want, exp = _oracle(orc, ("listed", unphased), batch)
    ctx.set_option("max_reads_hint", 256)
    try:
        code, rc, got, _flags, ev = _device_call(ctx, batch)
    finally:
        ctx.set_option("max_reads_hint", 0)
    assert code == 0 and rc == 0
    _assert_records(ev, exp, "hint 256")
    _assert_properties(batch, got, exp)
    assert exp["n_kept"].any()


def test_device_entry_needs_the_per_pair_outputs(ctx, orc):
    batch, _depths, _want, exp = _ladder(orc, False)
    code, rc, _res, _flags, ev = _device_call(ctx, batch, evidence=True, pair_outputs=False, check=False)
    assert code == B.INQ_ERR_ARG and rc == 0
    assert (ev.view(np.uint8) == 0xFF).all()  # nothing was enqueued
    # without evidence they stay optional
    code, rc, res, _flags, _ev = _device_call(ctx, batch, evidence=False, pair_outputs=False)
    assert code == 0 and rc == 0
    assert np.array_equal(np.isnan(res.phase1), exp["n_group1"] < batch.support)


def test_one_context_several_calls(orc):
    """With evidence, without, then with evidence on a larger batch (the scratch grows): each call is right."""
    small, _ = gen.random_case(990_021, n_loci=5, unphased=True)
    want_s, exp_s = _oracle(orc, ("random", 21, 5, True), small)
    big, _depths, want_b, exp_b = _ladder(orc, True)
    with hipcall.Context(0) as c:
        rc, got, _fl, ev = c.call_batch_evidence(small)
        assert rc == 0
        _assert_records(ev, exp_s, "first call")
        rc, plain, flags = c.call_batch_flags(small)
        assert rc == 0 and gen.same_f64(plain.phase1, got.phase1) and gen.same_f64(plain.phase2, got.phase2)
        rc, got_b, _fl, ev = c.call_batch_evidence(big)
        assert rc == 0
        _assert_records(ev, exp_b, "third call, larger batch")
        _assert_properties(big, got_b, exp_b)
        rc, got, _fl, ev = c.call_batch_evidence(small)
        assert rc == 0
        _assert_records(ev, exp_s, "fourth call, small again")


# ---- the deferred batch -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,unphased", [(41, False), (42, True)])
def test_flush_with_evidence(ctx, orc, tmp_path, seed, unphased):
    from tests.test_host_frontend import _make_case

    minlen, support = 5, 3
    bam, bed, _loci, _recs = _make_case(tmp_path, seed, n_loci=40)
    sp = call.Spans(bam, region_file=bed, minlen=minlen, support=support, threads=2, unphased=unphased, max_comp_bytes=8_000)
    spans = [{k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in s.items()} for s in sp.spans()][:2]
    sp.close()
    assert len(spans) == 2
    ctx.call_discard()
    sizes = {"n_cigar_words": 0, "n_reads": 0, "n_pairs": 0}
    for s in spans:
        rc, stats = ctx.call_span_deferred(s["comp"], s["blocks"], s["anchors"], s["anchor_stop"], s["locus_tid"], s["locus_start"], s["locus_end"],
                                           minlen, support, unphased)
        assert rc == 0
        for k in sizes:
            sizes[k] += int(getattr(stats, k))
    n = ctx.deferred_loci
    assert n == sum(len(s["locus_start"]) for s in spans)
    rc, p1, p2, ties, _ms, flags, ev = ctx.call_flush_evidence()
    assert rc == 0 and len(ev) == n

    class St:
        n_cigar_words, n_reads, n_pairs = sizes["n_cigar_words"], sizes["n_reads"], sizes["n_pairs"]

    cigar, reads, pair_read, off = ctx.span_fetch_batch(St, n)
    batch = B.Batch(cigar=cigar, reads=reads, pair_read=pair_read, locus_pair_off=off,
                    locus_start=np.concatenate([s["locus_start"] for s in spans]).astype(np.uint32),
                    locus_end=np.concatenate([s["locus_end"] for s in spans]).astype(np.uint32), minlen=minlen, support=support, unphased=unphased)
    oc, want = orc.call_batch(batch, debug=True)
    assert oc == 0
    exp = expected_evidence(batch, want)
    _assert_records(ev, exp, "flush")
    assert gen.same_f64(p1, want.phase1) and gen.same_f64(p2, want.phase2) and ties == want.n_tie_loci == int(flags.sum())
    _assert_properties(batch, want, exp)
    assert exp["n_kept"].any() and batch.n_pairs > 0


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def file_evidence(loci, recs, unphased, minlen):
    """The evidence of every BED line, restated on the records the BAM was written from: (fetched, kept, h1, h2, clipped, min, max)"""
    out = []
    for _chrom, s, e, t in loci:
        se, ee = s - 10, e + 10
        fetched = py._fetch(recs[t], t, se, ee)
        groups, kept = {1: [], 2: []}, 0
        for r in fetched:
            if unphased:
                if se < (r.pos & py.U32) or (py.reference_end(r) & py.U32) < ee or r.mapq <= 10:
                    continue
                groups[1].append(py.call_from_cigar(r, minlen, se, ee))  # (which half a Call falls into is not part of the record)
            else:
                phase = py.get_phase(r)
                if phase is None or (se < (r.pos & py.U32) and (py.reference_end(r) & py.U32) < ee) or r.mapq <= 10:
                    continue
                c = py.call_from_cigar(r, minlen, se, ee)
                if phase in groups:
                    groups[phase].append(c)
            kept += 1
        grouped = groups[1] + groups[2]
        h1, h2 = (kept // 2, kept - kept // 2) if unphased else (len(groups[1]), len(groups[2]))
        vals = [v for _k, v in grouped]
        out.append((len(fetched), kept, h1, h2, sum(1 for k, _v in grouped if k == "Clip"), min(vals) if vals else None, max(vals) if vals else None))
    return out


def evidence_text(loci, rows, threads):
    dot = lambda v: "." if v is None else str(v)
    return HEADER + "\n" + "".join(
        f"{loci[i][0]}\t{loci[i][1]}\t{loci[i][2]}\t" + "\t".join(str(v) for v in rows[i][:5]) + f"\t{dot(rows[i][5])}\t{dot(rows[i][6])}\n"
        for i in row_order(loci, threads))


def _cli(args, env):
    e = dict(os.environ)
    e.pop("INQ_SERVER", None)
    e.update(env)
    return subprocess.run([call.CLI_PATH] + args, capture_output=True, text=True, env=e, timeout=300)


@pytest.mark.parametrize("frontend", ["host", "device"])
@pytest.mark.parametrize("unphased", [False, True])
def test_end_to_end(tmp_path, frontend, unphased):
    from tests.test_host_frontend import _make_case

    bam, bed, loci, recs = _make_case(tmp_path, 51, n_loci=40)
    rows = file_evidence(loci, recs, unphased, 5)
    # what the case must hold for the file to say anything
    assert any(r[3 if unphased else 2] < 3 for r in rows), "a NaN row"
    assert any(r[4] > 0 for r in rows) and any(r[0] > r[1] for r in rows) and any(r[5] is not None and r[5] < 0 for r in rows)
    assert row_order(loci, 4) != row_order(loci, 1)
    u = ["-u"] if unphased else []
    for threads in (1, 4):
        want = evidence_text(loci, rows, threads)
        plain, with_e, ev = tmp_path / f"plain{threads}.inq", tmp_path / f"e{threads}.inq", tmp_path / f"e{threads}.tsv"
        with open(plain, "w") as f:
            call.genotype_repeats(bam, None, bed, 5, 3, threads, unphased, None, None, out=f, frontend=frontend)
        with open(with_e, "w") as f:
            call.genotype_repeats(bam, None, bed, 5, 3, threads, unphased, None, None, out=f, frontend=frontend, evidence=str(ev))
        assert with_e.read_bytes() == plain.read_bytes()
        assert ev.read_text() == want, f"library, -t {threads}"
        assert len(ev.read_text().splitlines()) == len(plain.read_text().splitlines()) == len(loci) + 1
        # the NaN rows are the rows whose group is short of `support`
        for line, eline in zip(plain.read_text().splitlines()[1:], ev.read_text().splitlines()[1:]):
            a, e_ = line.split("\t"), eline.split("\t")
            assert a[:3] == e_[:3] and (a[3] == "NaN") == (int(e_[5]) < 3) and (a[4] == "NaN") == (int(e_[6]) < 3)
        env = {"INQ_FRONTEND": frontend}
        p = _cli(["call", bam, "-R", bed, "-t", str(threads)] + u, env)
        assert p.returncode == 0, p.stderr
        cli_ev = tmp_path / f"cli{threads}.tsv"
        r = _cli(["call", bam, "-R", bed, "-t", str(threads), "--evidence", str(cli_ev)] + u, env)
        assert r.returncode == 0, r.stderr
        assert r.stdout == p.stdout and r.stderr == p.stderr and r.stdout == plain.read_text()
        assert cli_ev.read_text() == want, f"CLI, -t {threads}"
    dev_ev = tmp_path / "devices.tsv"
    r = _cli(["call", bam, "-R", bed, "-t", "4", "--devices", "0,0", f"--evidence={dev_ev}"] + u, {"INQ_FRONTEND": frontend})
    assert r.returncode == 0, r.stderr
    assert r.stdout == (tmp_path / "plain4.inq").read_text()
    assert dev_ev.read_text() == evidence_text(loci, rows, 4), "--devices 0,0"
