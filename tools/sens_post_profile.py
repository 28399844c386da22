#!/usr/bin/env python3
"""Emulator uncertainty of the closed-form sensitivity analysis (gpemu_sens_post_dev, gpemu_sens_main_var) on one GPU: where
its time goes, what it costs beside gpemu_sens_cov_dev on the same context, and what the route a user had before costs -- the
box average of gpemu_predict_batch_dev's variance over resident uniform points.

    timeout -k 10 900 python tools/sens_post_profile.py [--out FILE] [--cases 4096x8,8192x8,4096x16]

Model: synth.design(N, d), power-exponential, order 1, the supplied thetas (lengths 0.6); box: the design's own range.

gpemu_sens_post_dev: HIP events on the context's stream around its four launches (GPEMU_PROF_SENS_POST), median of 7 calls after
3 warm-up calls, the launches one by one from one call's GPEMU_PROF_DUMP lines.  The corner C^-1 = U U^T is built by the first
call after a set-up and kept: its time is the GPEMU_PROF_GEMM time of that first call, measured once per case.  Beside it
gpemu_sens_cov_dev on the same context (GPEMU_PROF_SENS, the same medians) and its sweep, which the weighted sweep is compared
with.  gpemu_sens_main_var: host time of the call (it returns the curves, so it waits), ngrid = 32, median of 7 after 3.

Monte Carlo: n = 100 000 uniform points in the box, device-resident queries and results (generation and upload NOT timed), host
time of gpemu_predict_batch_dev + synchronisation, median of 5 after 2; the line gives the average variance minus the nugget
against s_all and the sample's own standard error.  No time is a pass criterion."""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madaiemulator_amd import abi, synth  # noqa: E402
from sens_profile import dumped, wall  # noqa: E402

KIND, ORDER, SEED = 1, 1, 20261003 + 2
NBASE, NGRID = 100000, 32


def events(c, cls, call, warm=3, reps=7):
    for _ in range(warm):
        call()
    c.sync()
    ms = []
    for _ in range(reps):
        c.prof_begin(cls)
        call()
        ms.append(c.prof_end()["ms"])
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="append the lines to this file as well")
    ap.add_argument("--cases", default="4096x8,8192x8,4096x16")
    a = ap.parse_args()
    lines = [f"# power-exponential, order {ORDER}, lengths 0.6, box = the design's range; HIP events around the launches, median of 7 after 3; "
             f"band: ngrid = {NGRID}, host time; Monte Carlo: n = {NBASE} points through gpemu_predict_batch_dev, host time + synchronisation, median of 5 after 2"]
    c = abi.Context(0)
    try:
        for case in a.cases.split(","):
            N, d = (int(v) for v in case.split("x"))
            X, y = synth.design(N, d, SEED)
            th = synth.default_thetas(KIND, d)
            c.set_model(KIND, ORDER, X, y)
            _, rc = c.predict_setup(th)
            assert rc == abi.OK
            lo, hi = X.min(axis=0), X.max(axis=0)
            out = c.dev_alloc(8 * (3 + 2 * d))
            try:
                def post():
                    c.sens_post_dev(lo, hi, out)

                def cov():
                    c.sens_cov_dev(lo, hi, out)

                c.prof_begin(abi.PROF_GEMM)                  # the first call of a set-up builds the corner
                post()
                corner = c.prof_end()["ms"]
                ms = events(c, abi.PROF_SENS_POST, post)
                parts = dumped(c, abi.PROF_SENS_POST, post)
                s = c.download(out, (2 + 2 * d,))
                cov_ms = events(c, abi.PROF_SENS, cov)
                cov_parts = dumped(c, abi.PROF_SENS, cov)
            finally:
                c.dev_free(out)
            sw, usw = dict(parts).get("sens_sweep_weighted", float("nan")), dict(cov_parts).get("sens_sweep", float("nan"))
            lines.append(f"N={N} d={d}: gpemu_sens_post_dev {ms:9.3f} ms (4 launches; " + ", ".join(f"{t} {v:.3f}" for t, v in parts) +
                         f") + corner once per set-up {corner:9.3f} ms; gpemu_sens_cov_dev {cov_ms:9.3f} ms -> post / cov {ms / cov_ms:5.2f}; "
                         f"weighted sweep / unweighted sweep {sw / usw:5.2f} ({usw:.3f} ms); s_none {s[0]:.6g} s_all {s[1]:.6g}")
            print(lines[-1], flush=True)
            grid = np.stack([np.linspace(lo[l], hi[l], NGRID) for l in range(d)])
            band_ms = wall(c.sync, lambda: c.sens_main_var(lo, hi, grid), 3, 7)
            lines.append(f"          gpemu_sens_main_var, {d} x {NGRID} + 1 rows: {band_ms:9.3f} ms (host call, results copied out)")
            print(lines[-1], flush=True)
            rng = np.random.default_rng(7)
            Q = np.ascontiguousarray(lo + (hi - lo) * rng.random((NBASE, d)))
            buf = c.dev_alloc(8 * (NBASE * d + 2 * NBASE))
            try:
                c.upload(buf, Q)
                mean_dev = abi.C.c_void_p(buf.value + 8 * NBASE * d)
                var_dev = abi.C.c_void_p(mean_dev.value + 8 * NBASE)
                mc_ms = wall(c.sync, lambda: c.predict_dev(NBASE, buf, mean_dev, var_dev), 2, 5)
                v = c.download(var_dev, (NBASE,))
            finally:
                c.dev_free(buf)
            est, se = v.mean() - float(np.exp(th[1])), v.std(ddof=1) / np.sqrt(NBASE)
            lines.append(f"          Monte Carlo, n = {NBASE} variances: {mc_ms:9.3f} ms -> Monte Carlo / closed form {mc_ms / ms:6.2f}; average variance - nugget "
                         f"{est:.6g} against s_all {s[1]:.6g}: off by {abs(est - s[1]) / s[1]:.2e} (its own standard error {se / s[1]:.2e})")
            print(lines[-1], flush=True)
    finally:
        c.close()
    if a.out:
        with open(a.out, "a") as fo:
            fo.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
