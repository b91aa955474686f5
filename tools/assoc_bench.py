"""Kernel time of inq_assoc_rows (HIP events, inq_ctx_timing_read), the whole call, and the numpy restatement on a sample of the same
rows.  usage: python tools/assoc_bench.py [n_rows] [n_samples] [binary|continuous] [k]
The reference's README reports for its R loop (scripts/STR_regression.R, one glm() per locus): "about 20 % of variants were tested in
a day" for 268 samples x 654 K loci, and 3 min for one chromosome with four cores busy.  That is what a user has today, not a target."""
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synth(n_rows, ns, outcome, k, seed=1):
    rng = np.random.default_rng(seed)
    y = (rng.random(ns) < 0.45).astype(np.float64) if outcome == "binary" else rng.normal(50.0, 10.0, ns)
    cov = rng.normal(size=(k, ns))
    lean = np.repeat(np.round((y - y.mean()) / y.std()), 2).astype(np.float32)
    vals = np.empty((n_rows, 2 * ns), dtype=np.float32)
    for r0 in range(0, n_rows, 50_000):  # in pieces: the generator's f64 / i64 temporaries are eight times the matrix
        v = vals[r0:r0 + 50_000]
        n = len(v)
        v[:] = rng.choice([8, 15, 31, 120, 400], (n, 1)).astype(np.float32) + rng.integers(-3, 4, (n, 2 * ns), dtype=np.int8)
        v += lean[None, :] * rng.integers(0, 3, (n, 1)).astype(np.float32)
        v[rng.random((n, 2 * ns), dtype=np.float32) < 0.03] = np.nan
    return vals, y, cov


def _restate(args):
    from tests import assoc_restatement as ar

    vals, y, cov, outcome = args
    return ar.assoc_rows(vals, y, cov, outcome, "max", 0.8, "chol")[0]


def main():
    n_rows = int(sys.argv[1]) if len(sys.argv) > 1 else 654_000
    ns = int(sys.argv[2]) if len(sys.argv) > 2 else 268
    outcome = sys.argv[3] if len(sys.argv) > 3 else "binary"
    k = int(sys.argv[4]) if len(sys.argv) > 4 else 0
    from inquistr_amd import hipcall  # noqa: E402

    vals, y, cov = synth(n_rows, ns, outcome, k)
    ctx = hipcall.Context(0)
    ctx.timing_enable(True)
    rows = None
    for it in range(4):  # the first call grows the buffers and loads the code object: warm-up
        ctx.timing_reset()
        t = time.perf_counter()
        rows = ctx.assoc_rows(vals, y, cov, outcome, "max", 0.8)
        wall = time.perf_counter() - t
        ms, launches = ctx.timing_read(0)
        print(f"{'warm-up' if it == 0 else 'run %d' % it}: {outcome} p = {2 + k}: {n_rows} loci x {ns} samples: kernel {ms:.3f} ms in {launches} launch(es) = "
              f"{n_rows / ms / 1e3:.2f} M loci/s, {vals.nbytes / ms / 1e6:.1f} GB/s of matrix read once; whole call incl. upload {wall * 1e3:.0f} ms = "
              f"{vals.nbytes / wall / 1e9:.2f} GB/s of host matrix", flush=True)
    st = np.bincount(rows["status"], minlength=7)
    print("rows per status:", dict(zip(hipcall.ASSOC_STATUS, st.tolist())), "mean n_iter", float(rows["n_iter"][rows["status"] == 0].mean()), flush=True)
    threads = min(16, len(os.sched_getaffinity(0)))
    sample = min(n_rows, 16 * 250)
    parts = [(vals[i::threads][: sample // threads], y, cov, outcome) for i in range(threads)]
    t = time.perf_counter()
    with ProcessPoolExecutor(threads) as ex:
        got = list(ex.map(_restate, parts))
    dt = time.perf_counter() - t
    done = sum(len(g) for g in got)
    same = all((g["status"] == rows[i::threads][: len(g)]["status"]).all() for i, g in enumerate(got))
    print(f"cpu restatement ({threads} processes, {done} loci, numpy f64, tests/assoc_restatement.py - not R): {dt * 1e3:.0f} ms = {done / dt / 1e3:.2f} K loci/s "
          f"(incl. starting the processes) -> {n_rows / (done / dt):.0f} s for all {n_rows}; same statuses as the GPU: {same}", flush=True)


if __name__ == "__main__":
    main()
