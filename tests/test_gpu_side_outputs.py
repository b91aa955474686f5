"""The per-locus side outputs together (tie flags, evidence, per-read Calls): every subset of the three through the widest entry of
each family - host buffers, device pointers, the flush of a deferred batch - against the call that asks for all three (which
test_gpu_tie_flags / test_gpu_evidence / test_gpu_read_calls tie to the oracle), and the three files of `call` at once, on one device and
on several, against the runs that ask for one file each."""
import ctypes as C
import itertools

import numpy as np
import pytest

from inquistr_amd import batch as B
from inquistr_amd import call, hipcall
from tests import gen
from tests.test_gpu_read_calls import _cli, _hand_built
from tests.test_tie_report import make_tie_case

pytestmark = pytest.mark.gpu

RC = hipcall.READ_CALL_DTYPE
EV = hipcall.EVIDENCE_DTYPE
SUBSETS = list(itertools.product([False, True], repeat=3))  # (flags, evidence, lists)
ALL = (True, True, True)


@pytest.fixture(scope="module")
def ctx():
    c = hipcall.Context(0)
    assert c.backend.startswith("hip:gfx950")
    yield c
    c.close()


def _batch(which, unphased):
    if which == "hand-built":  # one locus with pairs, one empty, one all filtered: every output differs from locus to locus
        return _hand_built(unphased)[0]
    return gen.random_case(990_011, n_loci=5, unphased=unphased)[0]  # five loci: more than the four of a workgroup


def _host_arrays(n, flags, evidence, lists):
    """the caller's arrays for n loci, every byte 0xFF; None where not asked for"""
    fl = np.full(n, 0xFF, dtype=np.uint8) if flags else None
    ev = np.full(n * EV.itemsize, 0xFF, dtype=np.uint8) if evidence else None
    off = np.full((n + 1) * 8, 0xFF, dtype=np.uint8) if lists else None
    return fl, ev, off


def _ptr(a):
    return None if a is None else a.ctypes.data


def _fetch_checks(ctx, lists, off, want_rec):
    """inq_read_calls_fetch behind a call: the records of a call with the lists, none of a call without"""
    if not lists:
        assert ctx.read_calls_fetch(1, check=False)[0] == B.INQ_ERR_ARG
        return
    total = int(off.view(np.uint64)[-1])
    assert total == len(want_rec)
    assert ctx.read_calls_fetch(total).tobytes() == want_rec.tobytes()
    assert ctx.read_calls_fetch(total + 1, check=False)[0] == B.INQ_ERR_ARG


def _same_as_all(got, want, subset, what):
    """every output asked for is byte for byte that of the call that asked for all three"""
    for name, asked, g, w in zip(("flags", "evidence", "kept_off"), subset, got, want):
        assert (g is not None) == asked
        if asked:
            assert g.tobytes() == w.tobytes(), f"{what}: {name}"


# ---- 1. host buffers --------------------------------------------------------------------------------------------------------------
def _host_call(ctx, batch, subset):
    res = B.Result.alloc(batch)
    bc, rc_ = batch.as_c(), res.as_c()
    out = _host_arrays(batch.n_loci, *subset)
    rc = ctx._L.inq_call_batch_reads(ctx._h, C.byref(bc), C.byref(rc_), *[_ptr(a) for a in out])
    assert rc == 0
    return res, int(rc_.n_tie_loci), out


@pytest.mark.parametrize("unphased", [False, True])
@pytest.mark.parametrize("which", ["hand-built", "random"])
def test_every_subset_through_the_host_entry(ctx, which, unphased):
    batch = _batch(which, unphased)
    want_res, want_ties, want = _host_call(ctx, batch, ALL)
    want_rec = ctx.read_calls_fetch(int(want[2].view(np.uint64)[-1]))
    assert len(want_rec) > 0 and not (want[0] == 0xFF).any()
    for subset in SUBSETS:
        what = f"{which} unphased={unphased} (flags, evidence, lists)={subset}"
        res, ties, got = _host_call(ctx, batch, subset)
        _same_as_all(got, want, subset, what)
        assert gen.same_f64(res.phase1, want_res.phase1) and gen.same_f64(res.phase2, want_res.phase2) and ties == want_ties, what
        _fetch_checks(ctx, subset[2], got[2], want_rec)


# ---- 2. device pointers -----------------------------------------------------------------------------------------------------------
def _device_call(ctx, batch, flags, evidence, lists):
    """The batch through inq_call_batch_device_reads with torch tensors, on torch's stream; all four output arrays exist and start as
    0xFF bytes, the call is handed those asked for.  Returns (Result, flags, evidence, kept_off, all n_pairs record slots) as bytes."""
    import torch

    dev = torch.device("cuda:0")

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)

    def ff(n_bytes):
        return torch.full((n_bytes,), 0xFF, dtype=torch.uint8, device=dev)

    t = {k: up(getattr(batch, k)) for k in ("cigar", "reads", "pair_read", "locus_pair_off", "locus_start", "locus_end")}
    n = batch.n_loci
    p1 = torch.full((n,), 7.0, dtype=torch.float64, device=dev)
    p2 = torch.full((n,), 7.0, dtype=torch.float64, device=dev)
    pc = torch.zeros(batch.n_pairs, dtype=torch.int64, device=dev)
    pb = torch.zeros(batch.n_pairs, dtype=torch.uint8, device=dev)
    fl, ev, ko, kr = ff(n), ff(n * EV.itemsize), ff((n + 1) * 8), ff(batch.n_pairs * RC.itemsize)
    b = B.InqBatchC()
    b.n_reads, b.n_cigar_words, b.n_pairs, b.n_loci = batch.n_reads, int(batch.cigar.shape[0]), batch.n_pairs, batch.n_loci
    for k, v in t.items():
        setattr(b, k, v.data_ptr())
    b.minlen, b.support, b.unphased, b.reserved = int(batch.minlen), int(batch.support), int(batch.unphased), 0
    r = B.InqResultC(p1.data_ptr(), p2.data_ptr(), pc.data_ptr(), pb.data_ptr(), 0)
    torch.cuda.synchronize()  # the uploads and fills are there: the enqueue below does not wait for torch's own work
    ctx.call_batch_device_reads(b, r, fl.data_ptr() if flags else None, ev.data_ptr() if evidence else None, ko.data_ptr() if lists else None,
                                kr.data_ptr() if lists else None, torch.cuda.current_stream().cuda_stream)
    rc, ties = ctx.status()  # (waits for the device)
    assert rc == 0
    res = B.Result(phase1=p1.cpu().numpy(), phase2=p2.cpu().numpy(), pair_call=pc.cpu().numpy(), pair_bits=pb.cpu().numpy(), n_tie_loci=ties)
    return (res,) + tuple(x.cpu().numpy() for x in (fl, ev, ko, kr))


def test_every_subset_through_the_device_entry(ctx):
    batch = _batch("random", False)
    want_res, *want = _device_call(ctx, batch, *ALL)
    total = int(want[2].view(np.uint64)[-1])
    assert 0 < total <= batch.n_pairs and not (want[0] == 0xFF).any()
    for subset in SUBSETS:
        what = f"(flags, evidence, lists)={subset}"
        res, *got = _device_call(ctx, batch, *subset)
        for name, asked, g, w in zip(("flags", "evidence", "kept_off", "records"), subset + (subset[2],), got, want):
            if asked:
                assert g.tobytes() == w.tobytes(), f"{what}: {name}"
            else:
                assert (g == 0xFF).all(), f"{what}: {name} was not asked for and is written"
        assert gen.same_f64(res.phase1, want_res.phase1) and gen.same_f64(res.phase2, want_res.phase2), what
        assert res.n_tie_loci == want_res.n_tie_loci, what
        assert np.array_equal(res.pair_call, want_res.pair_call) and np.array_equal(res.pair_bits, want_res.pair_bits), what


# ---- 3. the flush of a deferred batch ------------------------------------------------------------------------------------------------
def test_every_subset_through_the_flush(ctx, tmp_path):
    from tests.test_host_frontend import _make_case

    minlen, support, unphased = 5, 3, False
    bam, bed, _loci, _recs = _make_case(tmp_path, 41, n_loci=40)
    sp = call.Spans(bam, region_file=bed, minlen=minlen, support=support, threads=2, unphased=unphased, max_comp_bytes=8_000)
    spans = [{k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in s.items()} for s in sp.spans()][:2]
    sp.close()
    assert len(spans) == 2
    n = sum(len(s["locus_start"]) for s in spans)

    def flush(subset):
        ctx.call_discard()
        for s in spans:
            rc, _stats = ctx.call_span_deferred(s["comp"], s["blocks"], s["anchors"], s["anchor_stop"], s["locus_tid"], s["locus_start"],
                                                s["locus_end"], minlen, support, unphased)
            assert rc == 0
        assert ctx.deferred_loci == n
        p1, p2 = np.full(n, np.nan), np.full(n, np.nan)
        res = B.InqResultC(p1.ctypes.data, p2.ctypes.data, None, None, 0)
        ms = C.c_double(0.0)
        out = _host_arrays(n, *subset)
        rc = ctx._L.inq_call_flush_reads(ctx._h, C.byref(res), n, C.byref(ms), *[_ptr(a) for a in out])
        assert rc == 0 and ctx.deferred_loci == 0
        return p1, p2, int(res.n_tie_loci), out

    want_p1, want_p2, want_ties, want = flush(ALL)
    want_rec = ctx.read_calls_fetch(int(want[2].view(np.uint64)[-1]))
    assert len(want_rec) > 0 and not (want[0] == 0xFF).any()
    for subset in SUBSETS:
        what = f"flush (flags, evidence, lists)={subset}"
        p1, p2, ties, got = flush(subset)
        _same_as_all(got, want, subset, what)
        assert gen.same_f64(p1, want_p1) and gen.same_f64(p2, want_p2) and ties == want_ties, what
        _fetch_checks(ctx, subset[2], got[2], want_rec)


# ---- 4. the three files at once ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("frontend", ["host", "device"])
def test_all_three_files_at_once(tmp_path, frontend, threads):
    """--ties, --evidence and --read-calls together, on one device and with --devices 0,0, through the library and the CLI: each file is
    the one of a run that asked for it alone, the .inq the plain run's."""
    bam, bed, _loci, _recs, ties = make_tie_case(tmp_path)
    assert any(ties)
    names = ("ties", "evidence", "read_calls")

    def run(tag, devices=None, **files):
        out = tmp_path / f"{tag}.inq"
        with open(out, "w") as f:
            call.genotype_repeats(bam, None, bed, 5, 3, threads, True, None, None, out=f, frontend=frontend, devices=devices, **files)
        return out.read_bytes()

    plain = run("plain")
    alone = {}
    for name in names:
        path = tmp_path / f"alone.{name}"
        assert run(f"alone_{name}", **{name: str(path)}) == plain
        alone[name] = path.read_bytes()
    assert alone["ties"], "the tie report of the case is not empty"
    assert alone["evidence"].count(b"\n") == alone["read_calls"].count(b"\n") == len(ties) + 1

    def check(tag, paths):
        for name in names:
            assert paths[name].read_bytes() == alone[name], f"{tag}: {name}"

    for tag, devices in (("library", None), ("library --devices", [0, 0])):
        paths = {name: tmp_path / f"{tag.replace(' ', '')}.{name}" for name in names}
        assert run(tag.replace(" ", ""), devices=devices, **{k: str(v) for k, v in paths.items()}) == plain, tag
        check(tag, paths)
    for tag, extra in (("CLI", []), ("CLI --devices", ["--devices", "0,0"])):
        paths = {name: tmp_path / f"{tag.replace(' ', '')}.{name}" for name in names}
        r = _cli(["call", bam, "-R", bed, "-t", str(threads), "-u", "--ties", str(paths["ties"]), "--evidence", str(paths["evidence"]),
                  "--read-calls", str(paths["read_calls"])] + extra, {"INQ_FRONTEND": frontend})
        assert r.returncode == 0, r.stderr
        assert r.stdout.encode() == plain, tag
        check(tag, paths)
