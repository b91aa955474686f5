#!/usr/bin/env python3
"""locus_motif_kernel beside its yardstick read_motif_kernel, both alone over the same host buffers (inq_locus_motifs_find,
inq_motif_runs), each launched twice (under rocprofv3 --kernel-trace --stats a kernel's time is the second launch's):

  short  n_loci x 30 records of 163 bases of a CAG repeat with an interruption every ~50 bases (the shape of a 150-base window)
  clip   n_loci x 30 records of a 20 kb soft clip + 164 bases (tools/read_motifs_timing.py's `clip`)
  deep   ONE locus of n_loci x 100 records of 163 bases (n_loci = 1000: 100 000 records; a locus is the unit of work of the kernel)

    python3 tools/locus_motifs_timing.py [short|clip|deep] [n_loci]        # one JSON line

profiles/r20_locus_motifs/summary.md."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np

    from inquistr_amd import hipcall

    mode = sys.argv[1] if len(sys.argv) > 1 else "short"
    n_loci = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    per_locus = 100 if mode == "deep" else 30
    n, length = n_loci * per_locus, 20_000 + 164 if mode == "clip" else 163
    rng = np.random.default_rng(20)
    width = length + (length & 1)
    codes = np.broadcast_to(np.array([2, 1, 4], dtype=np.uint8)[np.arange(width) % 3], (256, width)).copy()
    codes[rng.random(codes.shape) < 0.02] = 15  # 256 different slices, dealt round
    codes[:, length:] = 0  # (an odd length leaves its last nibble empty)
    rows = (codes[:, 0::2] << 4) | codes[:, 1::2]
    packed = rows[np.arange(n) % 256].reshape(-1)
    sq = np.zeros(n, dtype=hipcall.SEQ_DTYPE)
    sq["n_bases"] = length
    kept_off = np.array([0, n], dtype=np.uint64) if mode == "deep" else np.arange(0, n + 1, per_locus, dtype=np.uint64)
    words = np.full(len(kept_off) - 1, hipcall.encode_motif("CAG"), dtype=np.uint64)
    ctx = hipcall.Context(0)
    walls = dict(read_motif=[], locus_motif=[])
    for _ in range(2):
        t0 = time.perf_counter()
        runs = ctx.motif_runs(sq, packed, kept_off, words)
        t1 = time.perf_counter()
        found, use = ctx.locus_motifs_find(sq, packed, kept_off)
        t2 = time.perf_counter()
        walls["read_motif"].append(round((t1 - t0) * 1e3, 2))
        walls["locus_motif"].append(round((t2 - t1) * 1e3, 2))
    print(json.dumps(dict(mode=mode, loci=len(words), records=n, bases_per_record=length, packed_bytes=int(packed.size), wall_ms=walls,
                          found_agc=int((use == hipcall.encode_motif("AGC")).sum()), mean_copies=float(found["copies"].mean()),
                          mean_motif_bases=float(runs["motif_bases"].mean()))), flush=True)


if __name__ == "__main__":
    main()
