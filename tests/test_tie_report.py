"""The tie report (`inquistr call --ties FILE`, inq_call_args_t.ties_path) without a GPU: the output stage of a prepared run
(inq_run_write_ties), the file as a -R input again, the one-process-per-GPU gather of the flags (call_dist on gloo, the oracle as
the per-rank compute) and the CLI's handling of a path it cannot write."""
import functools
import os
import random
import socket
import subprocess

import numpy as np
import pytest
import torch.multiprocessing as mp

from inquistr_amd import call
from oracle import pyoracle as py
from tests import gen
from tools import bamio

REFS = [("chr2", 300_000), ("chr7", 200_000), ("chr10", 250_000)]
TIE_LOCUS = ("chr7", 1000, 1050)


def tie_locus_reads():
    """Six unphased reads around chr7:1000-1050 (start_ext 990, end_ext 1060) whose sorted Calls are [0, 0, 10, 10, 20, 20]: the
    split (ks = 3) falls between the two 10s, one a Span (an insertion) and one a Clip (a soft clip inside the window)."""
    R = py.Record
    return [
        R(pos=960, cigar=[("M", 200)]),
        R(pos=960, cigar=[("M", 200)]),
        R(pos=960, cigar=[("M", 50), ("I", 10), ("M", 150)]),
        R(pos=990, cigar=[("S", 10), ("M", 200)]),
        R(pos=960, cigar=[("M", 50), ("I", 20), ("M", 150)]),
        R(pos=960, cigar=[("M", 50), ("I", 20), ("M", 150)]),
    ]


def make_tie_case(tmp_path, seed=5, n_random=8):
    """A coordinate-sorted BAM + BED: the hand-made tie locus, loci with random reads on chr2 and chr10 (BED order interleaves the
    contigs, so -t 1 and -t >= 2 order the rows differently).  Returns (bam, bed, loci, recs_by_tid, ties) with ties[i] the
    reference-shaped oracle's verdict for BED line i (unphased, minlen 5, support 3)."""
    rng = random.Random(seed)
    recs = {t: [] for t in range(len(REFS))}
    loci = []
    for k in range(n_random):
        t = 0 if k % 2 == 0 else 2
        start = 20_000 + 15_000 * k + rng.randint(0, 2000)
        end = start + rng.randint(5, 200)
        loci.append((REFS[t][0], start, end, t))
        recs[t] += gen.random_locus_reads(rng, start, end, rng.choice([3, 6, 9, 14]))
    for r in tie_locus_reads():
        recs[1].append(r)
    loci.insert(3, (TIE_LOCUS[0], TIE_LOCUS[1], TIE_LOCUS[2], 1))
    # a locus with no reads at all
    loci.append(("chr2", 5_000, 5_030, 0))
    bam = str(tmp_path / "ties.sorted.bam")
    w = bamio.BamWriter(bam, REFS)
    n = 0
    for t in range(len(REFS)):
        recs[t].sort(key=lambda r: r.pos)
        for r in recs[t]:
            r.tid = t
            tags = [("HP", r.hp[0], r.hp[1])] if r.hp else []
            w.add(f"r{n}", r.flag, t, r.pos, r.mapq, r.cigar, tags)
            n += 1
    w.close()
    bed = str(tmp_path / "ties.bed")
    with open(bed, "w") as f:
        for c, s, e, _ in loci:
            f.write(f"{c}\t{s}\t{e}\n")
    ties = [bool(py.genotype_repeat_unphased(recs[t], t, s, e, 5, 3)[2]) for _, s, e, t in loci]
    return bam, bed, loci, recs, ties


def row_order(loci, threads):
    """The .inq's row order (src/call.rs:141): BED order for -t 1, (human_compare(chrom), start) for -t >= 2, equal keys in BED order."""
    idx = list(range(len(loci)))
    if threads > 1:
        idx.sort(key=functools.cmp_to_key(lambda a, b: py.human_compare(loci[a][0], loci[b][0]) or (loci[a][1] > loci[b][1]) - (loci[a][1] < loci[b][1])))
    return idx


def expected_report(loci, flags, threads):
    return "".join(f"{loci[i][0]}\t{loci[i][1]}\t{loci[i][2]}\n" for i in row_order(loci, threads) if flags[i])


def test_hand_made_locus_is_a_tie(tmp_path):
    _bam, _bed, loci, _recs, ties = make_tie_case(tmp_path)
    k = [i for i, l in enumerate(loci) if l[:3] == TIE_LOCUS]
    assert len(k) == 1 and ties[k[0]]
    assert sum(ties) >= 1


@pytest.mark.parametrize("threads", [1, 4])
def test_write_ties_order_and_reuse_as_region_file(tmp_path, threads):
    bam, bed, loci, _recs, _ties = make_tie_case(tmp_path)
    flags = np.array([1 if i % 3 != 1 else 0 for i in range(len(loci))], dtype=np.uint8)
    run = call.Run(bam, None, bed, threads=threads)
    try:
        assert run.n_targets == len(loci)
        out = tmp_path / f"t{threads}.bed"
        with open(out, "w") as f:
            run.write_ties(flags, f)
        text = out.read_text()
        assert text == expected_report(loci, flags, threads)
        assert row_order(loci, 4) != row_order(loci, 1)  # the case tells the two orders apart
        # a flag count that does not match the target list is refused
        with open(tmp_path / "bad.bed", "w") as f, pytest.raises(call.CallError):
            run.write_ties(flags[:-1], f)
        # no rows call has collected flags on this run
        with pytest.raises(call.CallError):
            run.tie_flags(len(loci))
    finally:
        run.close()
    # the report is itself a valid -R input: it names exactly the flagged targets
    fe = call.FrontEnd(bam, region_file=str(out))
    try:
        got = [tuple(t) for t in fe.targets()]
    finally:
        fe.close()
    want = [tuple(loci[i][:3]) for i in row_order(loci, threads) if flags[i]]
    assert got == want


def test_all_zero_flags_write_an_empty_report(tmp_path):
    bam, bed, loci, _recs, _ties = make_tie_case(tmp_path)
    run = call.Run(bam, None, bed, threads=2)
    try:
        out = tmp_path / "none.bed"
        with open(out, "w") as f:
            run.write_ties(np.zeros(len(loci), dtype=np.uint8), f)
        assert out.read_text() == ""
    finally:
        run.close()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dist_worker(rank, world, port, bam, bed, threads, out_path, ties_path):
    import torch.distributed as dist

    from inquistr_amd import call_dist
    from oracle import orc

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)

    def compute(batch):
        code, res = orc.call_batch(batch)
        assert code == 0
        flags = np.zeros(batch.n_loci, dtype=np.uint8)
        for j in range(batch.n_loci):
            c1, r1 = orc.call_batch(batch.slice_loci(j, j + 1))
            assert c1 == 0
            flags[j] = 1 if r1.n_tie_loci else 0
        assert int(flags.sum()) == res.n_tie_loci
        return res.phase1, res.phase2, flags

    with open(out_path if rank == 0 else os.devnull, "w") as f:
        call_dist.genotype_repeats_distributed(bam, None, bed, 5, 3, threads, True, "S", out=f, rank=rank, world=world,
                                               compute=compute, ties=ties_path)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("threads", [1, 4])
def test_call_dist_gathers_tie_flags(tmp_path, orc, threads):
    bam, bed, loci, _recs, ties = make_tie_case(tmp_path)
    out, ties_path = str(tmp_path / "dist.inq"), str(tmp_path / "dist.ties.bed")
    mp.spawn(_dist_worker, args=(2, _free_port(), bam, bed, threads, out, ties_path), nprocs=2, join=True)
    assert open(ties_path).read() == expected_report(loci, ties, threads)
    assert TIE_LOCUS[0] + f"\t{TIE_LOCUS[1]}\t{TIE_LOCUS[2]}\n" in open(ties_path).read()


def test_cli_unwritable_ties_path(tmp_path):
    bam, bed, _loci, _recs, _ties = make_tie_case(tmp_path)
    bad = "/nonexistent/dir/x"
    env = dict(os.environ)
    env.pop("INQ_SERVER", None)
    r = subprocess.run([call.CLI_PATH, "call", bam, "-R", bed, "-u", "--ties", bad], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 1, r.stderr
    assert r.stdout == ""
    assert bad in r.stderr
    assert "tie report" in r.stderr


def test_library_unwritable_ties_path(tmp_path):
    bam, bed, _loci, _recs, _ties = make_tie_case(tmp_path)
    bad = str(tmp_path / "missing" / "t.bed")
    out = tmp_path / "o.inq"
    with open(out, "w") as f, pytest.raises(call.CallError) as e:
        call.genotype_repeats(bam, None, bed, 5, 3, 1, True, None, None, out=f, ties=bad)
    assert e.value.status == 1 and bad in e.value.message
    assert out.read_text() == ""
