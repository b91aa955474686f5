"""Per-locus tie flags on the GPU (INQ_LOCUS_TIE): the *_flags entry points against the oracle locus by locus over every reduce
tier, and the tie report (`--ties`) end to end through both front ends, several devices, a server, a cohort and call_dist."""
import os
import random
import socket
import subprocess
import tempfile
import time

import numpy as np
import pytest
import torch.multiprocessing as mp

from inquistr_amd import batch as B
from inquistr_amd import call
from tests import gen
from tests.test_tie_report import TIE_LOCUS, expected_report, make_tie_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from inquistr_amd import hipcall

    c = hipcall.Context(0)
    assert c.backend.startswith("hip:gfx950")
    yield c
    c.close()


def _clip_heavy(seed, unphased, n_loci=200, depths=(4, 7, 12, 33, 64, 90, 300, 2100)):
    """The shape of test_gpu_parity.test_clip_heavy_ties: many equal values of mixed Span / Clip."""
    rng = random.Random(seed)
    bb = B.BatchBuilder(minlen=5, support=3, unphased=unphased)
    for j in range(n_loci):
        start = 5000 + 1000 * j
        idx = []
        for _ in range(depths[j % len(depths)] if n_loci <= len(depths) * 2 else rng.choice(depths)):
            v = rng.choice([8, 8, 8, 20, 20, 31])
            if rng.random() < 0.5:
                cig, pos = [("M", 20), ("S", v), ("M", 200)], start - 10
            else:
                cig, pos = [("M", 100), ("I", v), ("M", 200)], start - 10 - 80
            idx.append(bb.add_read(pos, B.encode_cigar(cig), phase=rng.choice([1, 2])))
        bb.add_locus(start, start + 40, idx)
    return bb.build()


def _oracle_flags(orc, batch):
    flags = np.zeros(batch.n_loci, dtype=np.uint8)
    for j in range(batch.n_loci):
        code, r = orc.call_batch(batch.slice_loci(j, j + 1))
        assert code == 0
        flags[j] = 1 if r.n_tie_loci else 0
    return flags


def _batches():
    yield "clip_heavy_unphased", lambda: _clip_heavy(7, True)
    yield "clip_heavy_phased", lambda: _clip_heavy(7, False)
    # every reduce tier with ties in it: one wave (<= 256 reads), the workgroup's LDS sort (<= 2 048 / 16 384), the global-store
    # select, and the grid-wide select beyond 65 536 reads
    deep = (40, 200, 1500, 5000, 20_000, 70_000)
    yield "clip_heavy_deep_unphased", lambda: _clip_heavy(8, True, n_loci=len(deep) * 2, depths=deep)
    yield "clip_heavy_deep_phased", lambda: _clip_heavy(8, False, n_loci=len(deep) * 2, depths=deep)
    for k in range(4):
        yield f"mixed_depth_{k}", (lambda k=k: gen.mixed_depth_case(880_100 + k, k)[0])
    # case 0 holds the locus beyond 65 536 reads (the grid-wide select); called unphased here
    yield "mixed_depth_0_unphased", lambda: _as_unphased(gen.mixed_depth_case(880_100, 0)[0])


def _as_unphased(batch):
    batch.unphased = True
    return batch


_CASES = list(_batches())


@pytest.mark.parametrize("name", [n for n, _ in _CASES])
def test_batch_flags_match_oracle(ctx, orc, name):
    batch = dict(_CASES)[name]()
    rc, got, flags = ctx.call_batch_flags(batch)
    assert rc == 0
    want = _oracle_flags(orc, batch)
    assert np.array_equal(flags, want), f"{name}: flags differ at {np.nonzero(flags != want)[0][:8]}"
    assert int(flags.sum()) == got.n_tie_loci
    if not batch.unphased:
        assert not flags.any()
    elif name.startswith("clip_heavy"):
        assert got.n_tie_loci > 0, "the case should hold tie loci"
    rc2, plain = ctx.call_batch(batch)
    assert rc2 == 0
    assert gen.same_f64(got.phase1, plain.phase1) and gen.same_f64(got.phase2, plain.phase2)
    assert got.n_tie_loci == plain.n_tie_loci
    # the same built batch and the same oracle flags under the promised variants (the window-bounded row walk)
    assert not batch.reads["promise"].any() and gen.checked_share(batch) == 1.0
    for what in gen.promise_variants(batch, gen.DEEP_PROMISE_VARIANTS[1:]):
        rc3, got3, flags3 = ctx.call_batch_flags(batch)
        assert rc3 == 0, what
        assert np.array_equal(flags3, want), f"{name} {what}: flags differ at {np.nonzero(flags3 != want)[0][:8]}"
        assert int(flags3.sum()) == got3.n_tie_loci == got.n_tie_loci, what
        assert gen.same_f64(got3.phase1, got.phase1) and gen.same_f64(got3.phase2, got.phase2), what


def test_device_entry_flags(ctx, orc):
    import ctypes as C

    import torch

    batch = _clip_heavy(11, True)
    want = _oracle_flags(orc, batch)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).to(dev)  # (bytes: the library reads them as its own types)
    cig, rd, pr = t(batch.cigar), t(batch.reads), t(batch.pair_read)
    off, ls, le = t(batch.locus_pair_off), t(batch.locus_start), t(batch.locus_end)
    p1 = torch.empty(batch.n_loci, dtype=torch.float64, device=dev)
    p2 = torch.empty_like(p1)
    fl = torch.full((batch.n_loci,), 0xFF, dtype=torch.uint8, device=dev)
    bc = batch.as_c()
    bc.cigar, bc.reads, bc.pair_read = cig.data_ptr(), rd.data_ptr(), pr.data_ptr()
    bc.locus_pair_off, bc.locus_start, bc.locus_end = off.data_ptr(), ls.data_ptr(), le.data_ptr()
    from inquistr_amd.batch import InqResultC

    res = InqResultC(p1.data_ptr(), p2.data_ptr(), None, None, 0)
    torch.cuda.synchronize(dev)
    assert ctx._L.inq_call_batch_device_flags(ctx._h, C.byref(bc), C.byref(res), C.c_void_p(fl.data_ptr()), C.c_void_p(0)) == 0
    rc, ties = ctx.status()
    assert rc == 0
    got = fl.cpu().numpy()
    assert np.array_equal(got, want)
    assert int(got.sum()) == ties


def _flush_case(tmp_path):
    bam, bed, loci, _recs, ties = make_tie_case(tmp_path)
    return bam, bed, loci, ties


@pytest.mark.parametrize("frontend", ["host", "device"])
@pytest.mark.parametrize("threads", [1, 4])
def test_library_ties_both_front_ends(tmp_path, frontend, threads):
    bam, bed, loci, ties = _flush_case(tmp_path)
    plain, with_t, rep = tmp_path / "plain.inq", tmp_path / "t.inq", tmp_path / "t.bed"
    with open(plain, "w") as f:
        call.genotype_repeats(bam, None, bed, 5, 3, threads, True, None, None, out=f, frontend=frontend)
    with open(with_t, "w") as f:
        call.genotype_repeats(bam, None, bed, 5, 3, threads, True, None, None, out=f, frontend=frontend, ties=str(rep))
    assert with_t.read_bytes() == plain.read_bytes()
    assert rep.read_text() == expected_report(loci, ties, threads)
    assert f"{TIE_LOCUS[0]}\t{TIE_LOCUS[1]}\t{TIE_LOCUS[2]}\n" in rep.read_text()
    # phased: an empty report
    with open(tmp_path / "ph.inq", "w") as f:
        call.genotype_repeats(bam, None, bed, 5, 3, threads, False, None, None, out=f, frontend=frontend, ties=str(tmp_path / "ph.bed"))
    assert (tmp_path / "ph.bed").read_text() == ""
    # the report as -R: those loci's rows again
    again = tmp_path / "again.inq"
    with open(again, "w") as f:
        call.genotype_repeats(bam, None, str(rep), 5, 3, threads, True, None, None, out=f, frontend=frontend)
    rows = {tuple(l.split("\t")[:3]): l for l in plain.read_text().splitlines()[1:]}
    got = again.read_text().splitlines()[1:]
    assert got and all(rows[tuple(l.split("\t")[:3])] == l for l in got)


def _cli(args, env=None, **kw):
    e = dict(os.environ)
    e.pop("INQ_SERVER", None)
    e.update(env or {})
    return subprocess.run([call.CLI_PATH] + args, capture_output=True, text=True, env=e, timeout=300, **kw)


@pytest.mark.parametrize("frontend", ["host", "device"])
def test_cli_ties_and_devices(tmp_path, frontend):
    bam, bed, loci, ties = _flush_case(tmp_path)
    env = {"INQ_FRONTEND": frontend}
    plain = _cli(["call", bam, "-R", bed, "-u", "-t", "4"], env)
    assert plain.returncode == 0, plain.stderr
    rep = tmp_path / "cli.bed"
    r = _cli(["call", bam, "-R", bed, "-u", "-t", "4", "--ties", str(rep)], env)
    assert r.returncode == 0, r.stderr
    assert r.stdout == plain.stdout and r.stderr == plain.stderr
    assert rep.read_text() == expected_report(loci, ties, 4)
    rep2 = tmp_path / "dev.bed"
    r = _cli(["call", bam, "-R", bed, "-u", "-t", "1", "--devices", "0,0", "--ties", str(rep2)], env)
    assert r.returncode == 0, r.stderr
    assert rep2.read_text() == expected_report(loci, ties, 1)


def test_cohort_and_server_ties(tmp_path):
    bam, bed, loci, ties = _flush_case(tmp_path)
    out_dir = tmp_path / "calls"
    out_dir.mkdir()
    r = _cli(["cohort", "-R", bed, "-u", "-t", "2", "--ties", "--out-dir", str(out_dir), bam])
    assert r.returncode == 0, r.stderr
    assert (out_dir / "ties.sorted.ties.bed").read_text() == expected_report(loci, ties, 2)
    # served: the client sends the absolute path, the server writes it
    sock = os.path.join(tempfile.mkdtemp(prefix="inq"), "s.sock")  # (a socket's path has a length limit: not under a deep temp dir)
    srv = subprocess.Popen([call.CLI_PATH, "serve", "--socket", sock, "--idle-exit", "60"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    try:
        t0 = time.time()
        while not os.path.exists(sock) and time.time() - t0 < 60:
            time.sleep(0.1)
        direct = _cli(["call", bam, "-R", bed, "-u"])
        served = _cli(["call", os.path.basename(bam), "-R", bed, "-u", "--ties", "served.bed"], {"INQ_SERVER": sock}, cwd=str(tmp_path))
        assert served.returncode == 0, served.stderr
        assert served.stdout == direct.stdout
        assert (tmp_path / "served.bed").read_text() == expected_report(loci, ties, 1)
    finally:
        subprocess.run([call.CLI_PATH, "serve", "--socket", sock, "--quit"], timeout=60)
        try:
            srv.wait(timeout=60)
        except subprocess.TimeoutExpired:
            srv.kill()
            srv.wait()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _nccl_worker(rank, port, bam, bed, out_path, ties_path):
    import torch
    import torch.distributed as dist

    from inquistr_amd import call_dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        with open(out_path, "w") as f:
            call_dist.genotype_repeats_distributed(bam, None, bed, 5, 3, 4, True, None, out=f, rank=0, world=1, rows="device",
                                                   frontend="device", ties=ties_path)
    finally:
        dist.destroy_process_group()


def test_call_dist_world1_nccl_ties(tmp_path):
    bam, bed, loci, ties = _flush_case(tmp_path)
    out, rep = str(tmp_path / "d.inq"), str(tmp_path / "d.bed")
    mp.spawn(_nccl_worker, args=(_free_port(), bam, bed, out, rep), nprocs=1, join=True)
    assert open(rep).read() == expected_report(loci, ties, 4)
    plain = _cli(["call", bam, "-R", bed, "-u", "-t", "4"])
    assert plain.returncode == 0 and open(out).read() == plain.stdout
