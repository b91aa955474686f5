#!/usr/bin/env python3
"""What `--read-motifs` costs the device front end on a SEQ-bearing synthetic BAM (the shape tools/read_seqs_timing.py uses), every
target under the motif CAG:

  cli    `inquistr call` with INQ_FRONTEND=device and INQ_TIMING=2, alternately with --read-seqs and with --read-motifs: the span loop's
         seconds and the flushes' wall milliseconds as the library prints them, median (min - max) over the rounds
  api    the spans appended to one deferred batch and flushed, with names + sequences and with names + sequences + motifs, alternated:
         the flush's launch sequence by HIP events, wall time of flush + fetches
  once   one append + flush with motifs (under rocprofv3 --kernel-trace --stats)
  clip   the kernel alone (inq_motif_runs) over n_loci x 30 records whose slices are a 20 kb soft clip + 164 bases of a noisy CAG
         repeat, twice (under rocprofv3 --kernel-trace --stats: read_motif_kernel's time is the second launch's)

    python3 tools/read_motifs_timing.py [cli|api|once|clip] [workload] [n_loci] [rounds]        # one JSON line

profiles/r19_read_motifs/summary.md."""
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
    cag = hipcall.encode_motif("CAG")
    line = dict(mode=mode, workload=name, n_loci=n_loci, rounds=rounds)
    if mode == "clip":
        n, length = n_loci * 30, 20_000 + 164
        rng = np.random.default_rng(19)
        codes = np.broadcast_to(np.array([2, 1, 4], dtype=np.uint8)[np.arange(length) % 3], (256, length)).copy()
        codes[rng.random(codes.shape) < 0.02] = 15  # an interruption every ~50 bases; 256 different slices, dealt round
        rows = (codes[:, 0::2] << 4) | codes[:, 1::2]  # (length is even: every slice fills its bytes)
        packed = rows[np.arange(n) % 256].reshape(-1)
        sq = np.zeros(n, dtype=hipcall.SEQ_DTYPE)
        sq["n_bases"] = length
        kept_off = np.arange(0, n + 1, 30, dtype=np.uint64)
        words = np.full(n_loci, cag, dtype=np.uint64)
        ctx = hipcall.Context(0)
        walls = []
        for _ in range(2):
            t0 = time.perf_counter()
            got = ctx.motif_runs(sq, packed, kept_off, words)
            walls.append(round((time.perf_counter() - t0) * 1e3, 2))
        print(json.dumps(dict(line, records=n, bases_per_record=length, packed_bytes=int(packed.size), wall_ms=walls,
                              mean_motif_bases=float(got["motif_bases"].mean()), mean_runs=float(got["n_runs"].mean()))), flush=True)
        return
    with tempfile.TemporaryDirectory() as tmp:
        prefix = os.path.join(tmp, "w")
        if os.path.exists(os.path.join(ROOT, "tools", "libsynthbam.so")):
            make_synth_bam.write_native(name, n_loci, prefix, seq=True)
        else:
            make_synth_bam.write(name, n_loci, prefix, seq=True)
        line["bam_bytes"] = os.path.getsize(prefix + ".bam")
        if mode == "cli":
            env = dict(os.environ, INQ_FRONTEND="device", INQ_TIMING="2")
            env.pop("INQ_SERVER", None)
            base = [call.CLI_PATH, "call", prefix + ".bam", "-R", prefix + ".bed", "-t", "8", "-m", str(wl.minlen), "-s", str(wl.support)]
            base += ["-u"] if wl.unphased else []
            variants = {"seqs": ["--read-seqs", os.path.join(tmp, "s.tsv")],
                        "motifs": ["--read-motifs", os.path.join(tmp, "m.tsv"), "--motif", "CAG"]}
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
            line["motifs_file_bytes"] = os.path.getsize(os.path.join(tmp, "m.tsv"))
            line["motifs_file_lines"] = sum(1 for _ in open(os.path.join(tmp, "m.tsv")))
            print(json.dumps(line), flush=True)
            return
        sp = call.Spans(prefix + ".bam", region_file=prefix + ".bed", minlen=wl.minlen, support=wl.support, threads=8, unphased=wl.unphased)
        spans = [{k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in s.items()} for s in sp.spans()]
        sp.close()
    ctx = hipcall.Context(0)

    def run(motifs):
        ctx.call_discard()
        for s in spans:
            ctx.call_span_deferred(s["comp"], s["blocks"], s["anchors"], s["anchor_stop"], s["locus_tid"], s["locus_start"], s["locus_end"],
                                   wl.minlen, wl.support, wl.unphased, names=True, seqs=True)
        words = np.full(ctx.deferred_loci, cag, dtype=np.uint64)
        t1 = time.perf_counter()
        out = ctx.call_flush_motifs(words) if motifs else ctx.call_flush_seqs()
        t2 = time.perf_counter()
        got = dict(ms_call=out[4], flush_ms=(t2 - t1) * 1e3, records=int(out[7][-1]), mean_bases=float(out[12]["n_bases"].mean()))
        if motifs:
            got.update(mean_motif_bases=float(out[15]["motif_bases"].mean()), mean_runs=float(out[15]["n_runs"].mean()))
        return got

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
    for v, key in ((False, "seqs"), (True, "seqs_motifs")):
        for f in ("ms_call", "flush_ms"):
            line[f"{key}_{f}"] = _stat([r[f] for r in got[v]])
        line[f"{key}_records"] = got[v][0]["records"]
    line["mean_bases"], line["mean_motif_bases"], line["mean_runs"] = got[True][0]["mean_bases"], got[True][0]["mean_motif_bases"], got[True][0]["mean_runs"]
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
