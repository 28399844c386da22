#!/usr/bin/env python3
"""Calibration epilogue against the prediction sweep it follows, on one GPU: N = 8192, d = 8, power-exponential, order 1,
r = 8 components on one design, M = 10^6 device-resident candidate points, nt = 16 and 128 outputs.

    timeout -k 10 900 python tools/calib_profile.py [--out profiles/calib.txt] [--M 1000000]

Measured, HIP events through the library's profile classes (medians of REPS calls after WARM), wall clock where said:
  * gpemu_calib_eval_dev (GPEMU_PROF_CALIB) per nt, and gpemu_calib_select_dev at a cut that keeps about 1 %
  * the r components' gpemu_predict_batch_dev on the same points (wall clock with a synchronise, one call per component after
    one warm-up call: it is the long part)
  * what a user had before: the r x M means and variances to the host (one download) and the per-output statistics with the
    diagonal variance rule in numpy -- back-projection to M x nt, I_t, the largest three -- on this machine's CPU (wall clock).
    The host layer's own back-projection in C is not reachable from this tool and is not measured.
No ratio is asserted."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madaiemulator_amd import abi, synth  # noqa: E402

KIND, ORDER, N, D, R, SEED = 1, 1, 8192, 8, 8, 20261003 + 2
WARM, REPS = 3, 15


def observation_set(nt, rng):
    Q, _ = np.linalg.qr(rng.standard_normal((nt, R)))
    A = np.ascontiguousarray(Q * (2.0 * 10.0 ** (-1.5 * np.arange(R) / R)))
    ybar = rng.uniform(0.5, 3.0, nt)
    sd = rng.uniform(0.05, 0.3, nt)
    z = ybar + A @ rng.standard_normal(R) + sd * rng.standard_normal(nt)
    return ybar, A, z, sd, rng.uniform(0.0, 0.1, nt)


def numpy_before(mean, var, ybar, A, z, sd, rel, block=65536):
    """the diagonal rule on the host: stat rows 2-4 and worst, block by block"""
    M = mean.shape[1]
    top = np.empty((3, M))
    worst = np.empty(M, dtype=np.int32)
    A2 = A * A
    for q0 in range(0, M, block):
        m, v = mean[:, q0:q0 + block].T, np.maximum(var[:, q0:q0 + block].T, 0.0)
        y = ybar + m @ A.T
        I = np.abs(z - y) / np.sqrt(v @ A2.T + sd * sd + (rel * y) ** 2)
        worst[q0:q0 + block] = np.argmax(I, axis=1)
        top[:, q0:q0 + block] = -np.partition(-I, 2, axis=1)[:, :3].T
    return top, worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="append the lines to this file as well")
    ap.add_argument("--M", type=int, default=1000000)
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
    xq, mv, st = c0.dev_alloc(M * D * 8), c0.dev_alloc(2 * R * M * 8), c0.dev_alloc(5 * M * 8)
    wi = c0.dev_alloc(2 * M * 4)
    mean_at = lambda k: xq.__class__(mv.value + k * M * 8)
    var_at = lambda k: xq.__class__(mv.value + (R + k) * M * 8)
    try:
        c0.upload(xq, synth.queries(M, D, 5))
        ctxs[0].predict_dev(min(M, 16384), xq, mean_at(0), var_at(0))          # warm-up of the sweep's kernels
        ctxs[0].sync()
        t0 = time.perf_counter()
        for k, c in enumerate(ctxs):
            c.predict_dev(M, xq, mean_at(k), var_at(k))
        for c in ctxs:
            c.sync()
        sweep_ms = (time.perf_counter() - t0) * 1e3
        say(f"# N={N} d={D} pow-exp order {ORDER}, r={R} components, M={M} device-resident points; events: medians of {REPS} after {WARM}")
        say(f"prediction sweep, {R} x gpemu_predict_batch_dev, wall clock, one call   {sweep_ms:12.1f} ms")
        t0 = time.perf_counter()
        host_mv = c0.download(mv, (2 * R, M))
        down_ms = (time.perf_counter() - t0) * 1e3
        say(f"download of the {R} x M means and variances ({16 * R * M / 1e6:.0f} MB)                 {down_ms:12.1f} ms")
        for nt in (16, 128):
            ybar, A, z, sd, rel = observation_set(nt, rng)
            c0.calib_setup(ybar, A, z, sd=sd, rel=rel)
            call = lambda: c0.calib_eval_dev(M, mean_at(0), var_at(0), M, st, wi)
            for _ in range(WARM):
                call()
            ms = []
            for _ in range(REPS):
                c0.prof_begin(abi.PROF_CALIB)
                call()
                p = c0.prof_end()
                ms.append(p["ms"])
            ev = statistics.median(ms)
            stat = c0.download(st, (5, M))
            cut = float(np.nanquantile(stat[2], 0.01))
            sel = lambda: c0.calib_select_dev(M, st, np.inf, 1, cut, wi.__class__(wi.value + 4 * M))
            for _ in range(WARM):
                kept = sel()
            ms = []
            for _ in range(REPS):
                c0.prof_begin(abi.PROF_CALIB)
                sel()
                ms.append(c0.prof_end()["ms"])
            se = statistics.median(ms)
            t0 = time.perf_counter()
            top, worst = numpy_before(host_mv[:R], host_mv[R:], ybar, A, z, sd, rel)
            np_ms = (time.perf_counter() - t0) * 1e3
            agree = np.nanmax(np.abs(top[0] - stat[2]) / np.maximum(1.0, np.abs(stat[2])))
            say(f"nt={nt:4d}  gpemu_calib_eval_dev  {ev:9.3f} ms  ({p['flops'] / ev / 1e9:8.1f} TFLOP/s by the header's rule, "
                f"{p['bytes'] / ev / 1e6:8.1f} GB/s)   = {ev / sweep_ms * 100:.4f} % of the sweep")
            say(f"nt={nt:4d}  gpemu_calib_select_dev {se:8.3f} ms  (three launches and the count; kept {kept} of {M})")
            say(f"nt={nt:4d}  numpy on the host, diagonal rule only (no chi2, no logpdf)  {np_ms:9.1f} ms   "
                f"(largest I_t agrees with the device to {agree:.1e})")
    finally:
        for p_ in (xq, mv, st, wi):
            c0.dev_free(p_)
        for c in ctxs:
            c.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
