#!/usr/bin/env python3
"""What the read table costs the device front end: a synthetic workload written as a BAM (tools/make_synth_bam.py), its spans appended
to one deferred batch and flushed - with the per-read Calls only, and with origins and names too.  One process, one context, the
variants alternate; per variant the HIP-event time of the flush's launch sequence (ms_call: the origin pass and its scan are inside,
the names' copy launch is not) and the wall time of append + flush + fetches.  profiles/r17_read_table/summary.md.

    python3 tools/read_table_timing.py [workload] [n_loci] [rounds] [seq]        # one JSON line
    python3 tools/read_table_timing.py [workload] [n_loci] once [seq]            # one round (under rocprofv3 --kernel-trace --stats)
"""
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np

    from inquistr_amd import call, hipcall, synth
    from tools import make_synth_bam

    name = sys.argv[1] if len(sys.argv) > 1 else "unphased100k"
    n_loci = int(sys.argv[2]) if len(sys.argv) > 2 else synth.WORKLOADS[name].n_loci
    once = len(sys.argv) > 3 and sys.argv[3] == "once"
    rounds = 1 if once else int(sys.argv[3]) if len(sys.argv) > 3 else 6
    seq = len(sys.argv) > 4 and sys.argv[4] == "seq"
    wl = synth.WORKLOADS[name]
    with tempfile.TemporaryDirectory() as tmp:
        prefix = os.path.join(tmp, "w")
        make_synth_bam.write(name, n_loci, prefix, seq=seq)
        sp = call.Spans(prefix + ".bam", region_file=prefix + ".bed", minlen=wl.minlen, support=wl.support, threads=8, unphased=wl.unphased)
        spans = [{k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in s.items()} for s in sp.spans()]
        sp.close()
    ctx = hipcall.Context(0)

    def run(names):
        t0 = time.perf_counter()
        ctx.call_discard()
        scan_ms = 0.0
        for s in spans:
            _rc, st = ctx.call_span_deferred(s["comp"], s["blocks"], s["anchors"], s["anchor_stop"], s["locus_tid"], s["locus_start"], s["locus_end"],
                                             wl.minlen, wl.support, wl.unphased, names=names)
            scan_ms += st.ms_scan
        t1 = time.perf_counter()
        out = ctx.call_flush_origins() if names else ctx.call_flush_reads()
        t2 = time.perf_counter()
        return dict(ms_call=out[4], append_ms=(t1 - t0) * 1e3, flush_ms=(t2 - t1) * 1e3, scan_ms=scan_ms, records=int(out[7][-1]),
                    name_bytes=out[11] if names else 0)

    for v in (False, True):  # warm: buffers grown, code objects loaded
        run(v)
    got = {False: [], True: []}
    for _ in range(rounds):
        for v in (False, True):
            got[v].append(run(v))
    line = dict(workload=name, n_loci=n_loci, seq=seq, spans=len(spans), rounds=rounds)
    for v, key in ((False, "lists"), (True, "lists_origins")):
        for f in ("ms_call", "append_ms", "flush_ms", "scan_ms"):
            xs = [r[f] for r in got[v]]
            line[f"{key}_{f}"] = [round(statistics.median(xs), 4), round(min(xs), 4), round(max(xs), 4)]
        line[f"{key}_records"] = got[v][0]["records"]
        line[f"{key}_name_bytes"] = got[v][0]["name_bytes"]
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
