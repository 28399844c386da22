#!/usr/bin/env python3
"""The mean-gradient sweep against the mean-only sweep on one GPU at BASELINE configs[2] (N=8192, d=8, Matern 5/2, order 1).

    timeout -k 10 400 python tools/predict_mean_grad_profile.py [--out FILE] [--queries M]

M = 10^6 device-resident queries through gpemu_predict_mean_grad_dev (GPEMU_PROF_MEAN_GRAD: both launches) and through
gpemu_predict_mean_dev (GPEMU_PROF_MEAN, the unchanged mean-only kernels: the yardstick), in one process; medians of 25 timed
calls after 5 warm-up calls.  The third row is what a caller paid for a central-difference gradient before: 2 d + 1
mean-only sweeps."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madaiemulator_amd import abi, synth  # noqa: E402

KIND, ORDER, N, D, SEED = 3, 1, 8192, 8, 20261003 + 2
WARM, REPS, BLOCK = 5, 25, 16384


def prof(c, cls, call):
    """median over REPS of the summed event time of the launches of class cls in one call, and their number"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="append the lines to this file as well")
    ap.add_argument("--queries", type=int, default=1000000)
    a = ap.parse_args()
    M = a.queries
    X, y = synth.design(N, D, SEED)
    c = abi.Context(0)
    c.set_model(KIND, ORDER, X, y)
    _, rc = c.predict_setup(synth.default_thetas(KIND, D))
    assert rc == abi.OK
    nblocks = (M + BLOCK - 1) // BLOCK
    buf = c.dev_alloc(M * (2 * D + 1) * 8)
    try:
        c.upload(buf, synth.queries(M, D, 5))
        mean, grad = buf.value + M * D * 8, buf.value + M * (D + 1) * 8
        ms_mean, n_mean = prof(c, abi.PROF_MEAN, lambda: c.predict_mean_dev(M, buf, mean))
        ms_grad, n_grad = prof(c, abi.PROF_MEAN_GRAD, lambda: c.predict_mean_grad_dev(M, buf, mean, grad))
        ms_mean2, _ = prof(c, abi.PROF_MEAN, lambda: c.predict_mean_dev(M, buf, mean))
    finally:
        c.dev_free(buf)
        c.close()
    lines = [
        f"# N={N} d={D} Matern 5/2 order {ORDER}, M={M} device-resident queries, {nblocks} blocks of {BLOCK}; medians of {REPS} after {WARM}",
        f"mean-only sweep (GPEMU_PROF_MEAN), before           {ms_mean:10.3f} ms / call  {n_mean} launches  {ms_mean / nblocks * 1e3:9.1f} us / block",
        f"mean + gradient sweep (GPEMU_PROF_MEAN_GRAD)        {ms_grad:10.3f} ms / call  {n_grad} launches  {ms_grad / nblocks * 1e3:9.1f} us / block",
        f"mean-only sweep (GPEMU_PROF_MEAN), after            {ms_mean2:10.3f} ms / call",
        f"ratio gradient sweep / mean-only sweep              {ms_grad / ms_mean:10.3f}   (expected about 2, no gate)",
        f"central differences: {2 * D + 1} mean-only sweeps             {(2 * D + 1) * ms_mean:10.3f} ms           {(2 * D + 1) * ms_mean / ms_grad:9.1f} x the gradient sweep",
    ]
    out = open(a.out, "a") if a.out else None
    for line in lines:
        print(line, flush=True)
        if out:
            out.write(line + "\n")
    if out:
        out.close()


if __name__ == "__main__":
    main()
