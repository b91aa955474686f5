#!/usr/bin/env python3
"""What `--read-seqs` costs the device front end on a SEQ-bearing synthetic BAM (the shape of bench.py's l2_seq block, tools/make_synth_bam.py):

  cli    `inquistr call` with INQ_FRONTEND=device and INQ_TIMING=2, alternately plain, with --read-table and with --read-seqs: the span
         loop's seconds and the flushes' wall milliseconds as the library prints them, median (min - max) over the rounds
  api    the spans appended to one deferred batch and flushed, with names only and with sequences, alternated: wall time of the
         appends and of flush + fetches, the records, and the device bytes the batch's slices hold (seq_off[n_pairs], every pair's)
  once   one append + flush with sequences (under rocprofv3 --kernel-trace --stats)

    python3 tools/read_seqs_timing.py [cli|api|once] [workload] [n_loci] [rounds]        # one JSON line

profiles/r18_read_seqs/summary.md."""
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stat(xs):
    return [round(statistics.median(xs), 4), round(min(xs), 4), round(max(xs), 4)]


def main():
    import numpy as np

    from inquistr_amd import call, hipcall, synth
    from tools import make_synth_bam

    mode = sys.argv[1] if len(sys.argv) > 1 else "cli"
    name = sys.argv[2] if len(sys.argv) > 2 else "phased10k"
    n_loci = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
    rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    wl = synth.WORKLOADS[name]
    line = dict(mode=mode, workload=name, n_loci=n_loci, rounds=rounds)
    with tempfile.TemporaryDirectory() as tmp:
        prefix = os.path.join(tmp, "w")
        t0 = time.perf_counter()
        if os.path.exists(os.path.join(ROOT, "tools", "libsynthbam.so")):
            make_synth_bam.write_native(name, n_loci, prefix, seq=True)
        else:
            make_synth_bam.write(name, n_loci, prefix, seq=True)
        line["bam_bytes"] = os.path.getsize(prefix + ".bam")
        line["write_s"] = round(time.perf_counter() - t0, 2)
        if mode == "cli":
            env = dict(os.environ, INQ_FRONTEND="device", INQ_TIMING="2")
            env.pop("INQ_SERVER", None)
            base = [call.CLI_PATH, "call", prefix + ".bam", "-R", prefix + ".bed", "-t", "8", "-m", str(wl.minlen), "-s", str(wl.support)]
            base += ["-u"] if wl.unphased else []
            variants = {"plain": [], "table": ["--read-table", os.path.join(tmp, "t.tsv")], "seqs": ["--read-seqs", os.path.join(tmp, "s.tsv")]}
            got = {k: dict(loop_s=[], flush_ms=[], wall_s=[]) for k in variants}
            for r in range(rounds + 1):  # (the first round warms the page cache and is dropped)
                for k, extra in variants.items():
                    t = time.perf_counter()
                    p = subprocess.run(base + extra, capture_output=True, text=True, env=env, timeout=600)
                    wall = time.perf_counter() - t
                    if p.returncode != 0:
                        raise SystemExit(p.stderr[-2000:])
                    if r == 0:
                        continue
                    loop = re.search(r"span loop: .*? ([0-9.]+) s from the first", p.stderr)
                    flushes = [float(x) for x in re.findall(r"locus kernels [0-9.]+ ms \| wall ([0-9.]+) ms", p.stderr)]
                    got[k]["loop_s"].append(float(loop.group(1)) if loop else float("nan"))
                    got[k]["flush_ms"].append(sum(flushes))
                    got[k]["wall_s"].append(wall)
            for k in variants:
                for f, xs in got[k].items():
                    line[f"{k}_{f}"] = _stat(xs)
            line["seqs_file_bytes"] = os.path.getsize(os.path.join(tmp, "s.tsv"))
            line["seqs_file_lines"] = sum(1 for _ in open(os.path.join(tmp, "s.tsv")))
            print(json.dumps(line), flush=True)
            return
        sp = call.Spans(prefix + ".bam", region_file=prefix + ".bed", minlen=wl.minlen, support=wl.support, threads=8, unphased=wl.unphased)
        spans = [{k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in s.items()} for s in sp.spans()]
        sp.close()
    ctx = hipcall.Context(0)

    def run(seqs):
        t0 = time.perf_counter()
        ctx.call_discard()
        n_pairs = 0
        for s in spans:
            _rc, st = ctx.call_span_deferred(s["comp"], s["blocks"], s["anchors"], s["anchor_stop"], s["locus_tid"], s["locus_start"], s["locus_end"],
                                             wl.minlen, wl.support, wl.unphased, names=True, seqs=seqs)
            n_pairs += int(st.n_pairs)
        t1 = time.perf_counter()
        out = ctx.call_flush_seqs() if seqs else ctx.call_flush_origins()
        t2 = time.perf_counter()
        held = 0
        if seqs:  # the offsets alone: seq_off[n_pairs] is what the batch's slices hold on the device
            off = np.zeros(n_pairs + 1, dtype=np.uint64)
            rc = ctx._L.inq_span_fetch_seqs(ctx._h, None, None, off.ctypes.data, None, C.c_uint64(1 << 62))
            held = int(off[-1]) if rc == 0 else -1
        return dict(ms_call=out[4], append_ms=(t1 - t0) * 1e3, flush_ms=(t2 - t1) * 1e3, records=int(out[7][-1]), pairs=n_pairs,
                    seq_bytes_kept=out[14] if seqs else 0, seq_bytes_held=held)

    if mode == "once":
        print(json.dumps(dict(line, **run(True), spans=len(spans))), flush=True)
        return
    for v in (False, True):  # warm: buffers grown, code objects loaded
        run(v)
    got = {False: [], True: []}
    for _ in range(rounds):
        for v in (False, True):
            got[v].append(run(v))
    line["spans"] = len(spans)
    for v, key in ((False, "names"), (True, "names_seqs")):
        for f in ("ms_call", "append_ms", "flush_ms"):
            line[f"{key}_{f}"] = _stat([r[f] for r in got[v]])
        for f in ("records", "pairs", "seq_bytes_kept", "seq_bytes_held"):
            line[f"{key}_{f}"] = got[v][0][f]
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
