#!/usr/bin/env python3
"""What the launches behind the locus kernels cost a caller who asks for more than rows: the launch sequence of
inq_call_batch_device_reads on a device-resident batch with rows only, with per-pair outputs, with evidence, and with evidence and
the per-read Calls (read_calls.hip).  One process, the variants alternate, HIP events around the whole sequence
(inq_ctx_timing_read which = 0); profiles/r15_read_calls/summary.md.

    python3 tools/read_calls_timing.py [workload] [rounds] [reps]        # the table, one JSON line
    python3 tools/read_calls_timing.py [workload] once                   # one sequence of each variant (under rocprofv3 --kernel-trace)
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = ("rows", "pairs", "evidence", "evidence_lists")


def main():
    import torch

    from inquistr_amd import hipcall, synth
    from inquistr_amd.batch import InqResultC

    name = sys.argv[1] if len(sys.argv) > 1 else "unphased100k"
    once = len(sys.argv) > 2 and sys.argv[2] == "once"
    rounds = 1 if once else int(sys.argv[2]) if len(sys.argv) > 2 else 6
    reps = 1 if once else int(sys.argv[3]) if len(sys.argv) > 3 else 20
    wl = synth.WORKLOADS[name]
    dev = torch.device("cuda:0")
    ctx = hipcall.Context(0)
    shard = synth.DeviceBatch(wl, dev, 0, wl.n_loci, debug=True)
    stream = torch.cuda.Stream(device=dev)
    ev = torch.zeros(shard.n_loci * hipcall.EVIDENCE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    off = torch.zeros(shard.n_loci + 1, dtype=torch.int64, device=dev)
    kept = torch.zeros(shard.n_pairs * hipcall.READ_CALL_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    rows_only = InqResultC(shard.phase1.data_ptr(), shard.phase2.data_ptr(), None, None, 0)
    ctx.set_option("max_reads_hint", wl.reads_per_locus)

    def enqueue(variant):
        res = rows_only if variant == "rows" else shard.c_result
        ctx.call_batch_device_reads(shard.c_batch, res, None, ev.data_ptr() if variant.startswith("evidence") else None,
                                    off.data_ptr() if variant == "evidence_lists" else None,
                                    kept.data_ptr() if variant == "evidence_lists" else None, stream.cuda_stream)

    for v in VARIANTS:  # warm: scratch grown, code objects loaded
        for _ in range(1 if once else 5):
            enqueue(v)
    torch.cuda.synchronize()
    us = {v: [] for v in VARIANTS}
    for _ in range(rounds):
        for v in VARIANTS:
            ctx.timing_enable(True)
            ctx.timing_reset()
            for _ in range(reps):
                enqueue(v)
            torch.cuda.synchronize()
            ms, n = ctx.timing_read(0)
            ctx.timing_enable(False)
            us[v].append(ms / n * 1e3)
    rc, _ties = ctx.status()
    assert rc == 0, rc
    n_kept = int(off[-1].item())
    out = {"workload": name, "loci": shard.n_loci, "pairs": shard.n_pairs, "kept": n_kept, "rounds": rounds, "reps": reps,
           "tile": int(ctx._L.inq_read_call_tile()), "algorithmic_bytes": shard.algorithmic_bytes(),
           # what the three launches move: bits twice, Calls and pair_read of the kept pairs (and a descriptor word when phased) in,
           # a 16-byte record per kept pair and the offsets out
           "read_calls_bytes": 2 * shard.n_pairs + n_kept * (8 + 4 + (0 if wl.unphased else 4) + 16) + 16 * (shard.n_loci + 1),
           "us_per_sequence": {v: {"median": statistics.median(x), "min": min(x), "max": max(x)} for v, x in us.items()}}
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
