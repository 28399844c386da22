#!/usr/bin/env python3
"""Mean-only sweep against the mean+variance sweep on one GPU at BASELINE configs[2] (N=8192, d=8, Matern 5/2, order 1).

    python tools/predict_mean_profile.py dev  [--out FILE]     M = 10^6 device-resident queries, both sweeps, HIP events
    python tools/predict_mean_profile.py host [--out FILE]     M = 1 and M = 64 through the host-buffer entries, wall clock

Each mode is one process; run them one after the other, each under its own time limit, e.g.

    timeout -k 10 300 python tools/predict_mean_profile.py dev --out profiles/predict_mean_only.txt && \\
    timeout -k 10 120 python tools/predict_mean_profile.py host --out profiles/predict_mean_only.txt

Medians of 25 timed calls after 5 warm-up calls.  The yardstick for the fused kernel is the k-vector kernel of the
mean+variance sweep (GPEMU_PROF_FILL around gpemu_predict_batch_dev) per 16 384-query block: same element work, plus one
multiply-add per element and a row reduction, minus the 8 Np bytes per query it stores."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madaiemulator_amd import abi, synth  # noqa: E402

KIND, ORDER, N, D, SEED = 3, 1, 8192, 8, 20261003 + 2
WARM, REPS, BLOCK = 5, 25, 16384


def context():
    X, y = synth.design(N, D, SEED)
    c = abi.Context(0)
    c.set_model(KIND, ORDER, X, y)
    _, rc = c.predict_setup(synth.default_thetas(KIND, D))
    assert rc == abi.OK
    return c


def prof(c, cls, call):
    """median over REPS of (summed event time of the launches of class cls in one call, launches)"""
    for _ in range(WARM):
        call()
    ms, n = [], 0
    for _ in range(REPS):
        c.prof_begin(cls)
        call()
        p = c.prof_end()
        ms.append(p["ms"])
        n = p["n"]
    return statistics.median(ms), n


def wall(c, call):
    for _ in range(WARM):
        call()
    t = []
    for _ in range(REPS):
        c.sync()
        t0 = time.perf_counter()
        call()
        c.sync()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def run_dev(say):
    M = 1000000
    c = context()
    nblocks = (M + BLOCK - 1) // BLOCK
    buf = c.dev_alloc(M * (D + 2) * 8)
    try:
        c.upload(buf, synth.queries(M, D, 5))
        mean, var = buf.value + M * D * 8, buf.value + M * (D + 1) * 8
        ms_mean, n_mean = prof(c, abi.PROF_MEAN, lambda: c.predict_mean_dev(M, buf, mean))
        w_mean = wall(c, lambda: c.predict_mean_dev(M, buf, mean))
        ms_fill, n_fill = prof(c, abi.PROF_FILL, lambda: c.predict_dev(M, buf, mean, var))
        w_full = wall(c, lambda: c.predict_dev(M, buf, mean, var))
    finally:
        c.dev_free(buf)
        c.close()
    say(f"# dev: N={N} d={D} Matern 5/2 order {ORDER}, M={M} device-resident queries, {nblocks} blocks of {BLOCK}; medians of {REPS} after {WARM}")
    say(f"mean-only sweep, both launches (GPEMU_PROF_MEAN)   {ms_mean:10.3f} ms / call  {n_mean} launches  {ms_mean / nblocks * 1e3:9.1f} us / block")
    say(f"k-vector kernel of the full sweep (GPEMU_PROF_FILL) {ms_fill:10.3f} ms / call  {n_fill} launches  {ms_fill / nblocks * 1e3:9.1f} us / block")
    say(f"ratio mean-only / k-vector kernel                   {ms_mean / ms_fill:10.3f}   (criterion: <= 1.25)")
    say(f"mean-only sweep, wall clock                         {w_mean:10.3f} ms / call  {M / w_mean / 1e3:9.2f} M predictions/s")
    say(f"mean+variance sweep, wall clock                     {w_full:10.3f} ms / call  {M / w_full / 1e3:9.2f} M predictions/s")
    say(f"speed-up of the mean-only sweep                     {w_full / w_mean:10.1f} x")


def run_host(say):
    c = context()
    try:
        say(f"# host: N={N} d={D} Matern 5/2 order {ORDER}, host-buffer entries, wall clock per call; medians of {REPS} after {WARM}")
        for M in (1, 64):
            Xq = synth.queries(M, D, 6)
            a = wall(c, lambda: c.predict_mean(Xq))
            b = wall(c, lambda: c.predict(Xq))
            say(f"M={M:3d}  gpemu_predict_mean {a * 1e3:9.1f} us   gpemu_predict_batch {b * 1e3:9.1f} us")
    finally:
        c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["dev", "host"])
    ap.add_argument("--out", help="append the lines to this file as well")
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")

    (run_dev if a.mode == "dev" else run_host)(say)
    if out:
        out.close()


if __name__ == "__main__":
    main()
