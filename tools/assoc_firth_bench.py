"""Kernel time (HIP events, inq_ctx_timing_read) and call time of inq_assoc_rows_firth beside inq_assoc_rows on the same input in the
same run: `always`, and `fallback` on a cohort with about 1 % separated loci and on one with none.  The cohort is
tools/assoc_bench.py's.  usage: python tools/assoc_firth_bench.py [n_rows] [n_samples] [k]
Every figure is printed as a time and as a ratio to the ordinary call on that input; there is no pass mark."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from assoc_bench import synth  # noqa: E402


def timed(ctx, what, fn, runs=5):
    """median kernel ms and call ms of `runs` calls behind one warm-up"""
    k, w, out = [], [], None
    for it in range(runs + 1):
        ctx.timing_reset()
        t = time.perf_counter()
        out = fn()
        wall = (time.perf_counter() - t) * 1e3
        ms, launches = ctx.timing_read(0)
        if it:
            k.append(ms), w.append(wall)
    k, w = float(np.median(k)), float(np.median(w))
    print(f"  {what:34s} kernel {k:9.3f} ms ({launches} launches)   call {w:8.1f} ms", flush=True)
    return k, w, out


def main():
    n_rows = int(sys.argv[1]) if len(sys.argv) > 1 else 654_000
    ns = int(sys.argv[2]) if len(sys.argv) > 2 else 268
    k = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    from inquistr_amd import hipcall

    vals, y, cov = synth(n_rows, ns, "binary", k)
    ctx = hipcall.Context(0)
    ctx.timing_enable(True)
    print(f"binary p = {2 + k}: {n_rows} loci x {ns} samples", flush=True)
    for label in ("no separated locus", "about 1 % separated loci"):
        if label != "no separated locus":
            rng = np.random.default_rng(9)
            idx = rng.choice(n_rows, max(1, n_rows // 100), replace=False)
            vals[idx] = 10.0 + rng.integers(0, 4, (len(idx), 2 * ns)).astype(np.float32) + 8.0 * np.repeat(y, 2).astype(np.float32)[None, :]
        print(label + ":", flush=True)
        k0, w0, rows = timed(ctx, "inq_assoc_rows", lambda: ctx.assoc_rows(vals, y, cov, "binary", "max", 0.8))
        for when in ("fallback", "always"):
            k1, w1, (r1, firth) = timed(ctx, f"inq_assoc_rows_firth {when}", lambda: ctx.assoc_rows_firth(vals, y, cov, "max", 0.8, when))
            fitted = firth["status"] != 1
            ok = firth["status"] == 0
            print(f"    -> kernel x {k1 / k0:.2f}, call x {w1 / w0:.2f} of the ordinary call; rows identical: {r1.tobytes() == rows.tobytes()}; fitted "
                  f"{int(fitted.sum())} ({100.0 * fitted.mean():.2f} %), OK {int(ok.sum())}, mean steps full {float(firth['n_iter_full'][ok].mean()) if ok.any() else 0:.1f} "
                  f"null {float(firth['n_iter_null'][ok].mean()) if ok.any() else 0:.1f}, most {int(firth['n_iter_full'].max())}", flush=True)
        if label == "no separated locus":
            # the entry's own cost: with the bound at 0 no row of this cohort is selected, every wave of the second kernel reads its
            # row's status and returns
            ctx.set_option("assoc_firth_mu_ppb", 0)
            k1, w1, (r1, firth) = timed(ctx, "inq_assoc_rows_firth fallback, bound 0", lambda: ctx.assoc_rows_firth(vals, y, cov, "max", 0.8, "fallback"))
            ctx.set_option("assoc_firth_mu_ppb", 1000)
            print(f"    -> kernel x {k1 / k0:.2f}, call x {w1 / w0:.2f} of the ordinary call; rows identical: {r1.tobytes() == rows.tobytes()}; fitted "
                  f"{int((firth['status'] != 1).sum())}", flush=True)
        st = np.bincount(rows["status"], minlength=7)
        print("  ordinary rows per status:", dict(zip(hipcall.ASSOC_STATUS, st.tolist())), flush=True)


if __name__ == "__main__":
    main()
