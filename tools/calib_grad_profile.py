#!/usr/bin/env python3
"""The calibration gradient launch against the gradient sweeps it follows, on one GPU: N = 8192, d = 8, power-exponential,
order 1, r = 8 components on one design, nt = 16 outputs, M = 131 072 device-resident points.

    timeout -k 10 900 python tools/calib_grad_profile.py [--out profiles/calib_grad.txt] [--M 131072]

Measured:
  * gpemu_calib_grad_dev alone, HIP events through the library's profile class GPEMU_PROF_CALIB (median of REPS calls after
    WARM), both outputs and the log density's alone, and its achieved bytes/s against the 16 nr d + 16 d (8 d for one output)
    bytes per point it must move (the 16 nr bytes of means and variances are left out of that count)
  * the r components' gpemu_predict_var_grad_dev and gpemu_predict_mean_grad_dev in front of it (wall clock with a
    synchronise, one call per component after one warm-up call each: the long part)
  * for comparison the existing entries: ONE evaluation of all points, r x gpemu_predict_batch_dev + gpemu_calib_eval_dev
    (wall clock); central differences take 2 d + 1 of them, which is that time multiplied, not run
No ratio is asserted."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madaiemulator_amd import abi, synth  # noqa: E402

KIND, ORDER, N, D, R, NT, SEED = 1, 1, 8192, 8, 8, 16, 20261003 + 2
WARM, REPS = 3, 15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="append the lines to this file as well")
    ap.add_argument("--M", type=int, default=131072)
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    M = a.M
    rng = np.random.default_rng(11)
    X, y = synth.design(N, D, SEED)
    ctxs = [abi.Context(0) for _ in range(R)]
    th = synth.default_thetas(KIND, D)
    for k, c in enumerate(ctxs):
        c.set_model(KIND, ORDER, X, y * (1.0 + 0.1 * k) + 0.05 * rng.standard_normal(N))
    _, _, status, rc = abi.predict_setup_batch(ctxs, np.tile(th, (R, 1)))
    assert rc == abi.OK, status
    c0 = ctxs[0]
    Q, _ = np.linalg.qr(rng.standard_normal((NT, R)))
    A = np.ascontiguousarray(Q * (2.0 * 10.0 ** (-1.5 * np.arange(R) / R)))
    ybar, sd = rng.uniform(0.5, 3.0, NT), rng.uniform(0.05, 0.3, NT)
    c0.calib_setup(ybar, A, ybar + A @ rng.standard_normal(R) + sd * rng.standard_normal(NT), sd=sd)
    md = M * D
    xq, mv, g, o, st, wi = (c0.dev_alloc(8 * n) for n in (md, 2 * R * M, 2 * R * md, 2 * md, 5 * M, M))
    at = lambda base, k, n: base.__class__(base.value + 8 * k * n)
    try:
        c0.upload(xq, synth.queries(M, D, 5))
        w = min(M, 16384)
        c0.predict_var_grad_dev(w, xq, at(mv, 0, M), at(mv, R, M), at(g, R, md))       # warm-up of the sweeps' kernels
        c0.predict_mean_grad_dev(w, xq, None, at(g, 0, md))
        c0.predict_dev(w, xq, at(mv, 0, M), at(mv, R, M))
        c0.sync()

        def wall(enqueue):
            t0 = time.perf_counter()
            for k, c in enumerate(ctxs):
                enqueue(k, c)
            for c in ctxs:
                c.sync()
            return (time.perf_counter() - t0) * 1e3

        vg_ms = wall(lambda k, c: c.predict_var_grad_dev(M, xq, at(mv, k, M), at(mv, R + k, M), at(g, R + k, md)))
        mg_ms = wall(lambda k, c: c.predict_mean_grad_dev(M, xq, None, at(g, k, md)))
        pb_ms = wall(lambda k, c: c.predict_dev(M, xq, at(mv, k, M), at(mv, R + k, M)))
        t0 = time.perf_counter()
        c0.calib_eval_dev(M, at(mv, 0, M), at(mv, R, M), M, st, wi)
        c0.sync()
        ev_ms = (time.perf_counter() - t0) * 1e3
        c0.predict_var_grad_dev(M, xq, at(mv, 0, M), at(mv, R, M), at(g, R, md))       # (component 0's rows again: the sweep's own m, v)
        c0.sync()
        say(f"# N={N} d={D} pow-exp order {ORDER}, r={R} components, nt={NT}, M={M} device-resident points; events: medians of {REPS} after {WARM}")
        say(f"variance-gradient sweeps, {R} x gpemu_predict_var_grad_dev, wall clock, one call   {vg_ms:12.1f} ms")
        say(f"mean-gradient sweeps,     {R} x gpemu_predict_mean_grad_dev, wall clock, one call  {mg_ms:12.1f} ms")
        for both in (True, False):
            call = lambda: c0.calib_grad_dev(M, D, at(mv, 0, M), at(mv, R, M), M, at(g, 0, md), at(g, R, md), md,
                                             at(o, 0, md) if both else None, at(o, 1, md))
            for _ in range(WARM):
                call()
            ms = []
            for _ in range(REPS):
                c0.prof_begin(abi.PROF_CALIB)
                call()
                ms.append(c0.prof_end()["ms"])
            t = statistics.median(ms)
            must = M * (16.0 * R * D + (16.0 if both else 8.0) * D)
            say(f"gpemu_calib_grad_dev, {'both outputs' if both else 'glogpdf alone'}  {t:9.3f} ms  (min {min(ms):.3f}, max {max(ms):.3f})  "
                f"{must / t / 1e9:7.3f} TB/s of the {must / 1e6:.0f} MB it must move   = {t / (vg_ms + mg_ms) * 100:.4f} % of the sweeps before it")
        one = pb_ms + ev_ms
        say(f"one evaluation by the existing entries, {R} x gpemu_predict_batch_dev + gpemu_calib_eval_dev, wall clock   {one:12.1f} ms")
        say(f"central differences, 2 d + 1 = {2 * D + 1} such evaluations (multiplied, not run)   {one * (2 * D + 1):12.1f} ms   "
            f"against {vg_ms + mg_ms:.1f} ms of sweeps + the launch")
        gl = c0.download(at(o, 1, md), (M, D))
        say(f"(glogpdf: {np.isfinite(gl).mean() * 100:.2f} % finite, median |g| {np.nanmedian(np.abs(gl)):.3e})")
    finally:
        for p_ in (xq, mv, g, o, st, wi):
            c0.dev_free(p_)
        for c in ctxs:
            c.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
