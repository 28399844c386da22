#!/usr/bin/env python3
"""The joint-covariance entry against the prediction sweep on one GPU at BASELINE configs[2] (N=8192, d=8, Matern 5/2, order 1).

    timeout -k 10 900 python tools/predict_cov_profile.py [--out FILE] [--sizes 64,1024,4096,16384]

For each M, M device-resident queries through gpemu_predict_cov_dev and through gpemu_predict_batch_dev (the unchanged
prediction sweep on the same queries: the yardstick) in one process: medians of 25 timed calls after 5 warm-up calls, each
call timed on the host from its first enqueue to the end of a stream synchronisation, the sweep timed before and after the
entry.  Expected from the structure: the sweep's M N^2 flops plus M^2 N for the symmetric product, (1 + M / N) sweeps; accepted
up to 1.5 x that at M >= 4096.  Then the entry's launches by profiling class (GPEMU_PROF_GEMM: the sweep's product and the
symmetric one; GPEMU_PROF_FILL: the k-vectors; GPEMU_PROF_COV: the prior tiles and the mirror).  M = 64 is the one-tile
case, for which there is no fast path."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madaiemulator_amd import abi, synth  # noqa: E402

KIND, ORDER, N, D, SEED = 3, 1, 8192, 8, 20261003 + 2
WARM, REPS = 5, 25


def wall(c, call):
    """median over REPS of the host time of one call and the synchronisation behind it, ms"""
    for _ in range(WARM):
        call()
    c.sync()
    ms = []
    for _ in range(REPS):
        t = time.perf_counter()
        call()
        c.sync()
        ms.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ms)


def prof(c, cls, call, reps=5):
    """median over reps of the summed event time of the launches of class cls in one call, their number and flops"""
    ms, n, fl = [], 0, 0.0
    for _ in range(reps):
        c.prof_begin(cls)
        call()
        p = c.prof_end()
        ms.append(p["ms"])
        n, fl = p["n"], p["flops"]
    return statistics.median(ms), n, fl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="append the lines to this file as well")
    ap.add_argument("--sizes", default="64,1024,4096,16384")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    X, y = synth.design(N, D, SEED)
    c = abi.Context(0)
    c.set_model(KIND, ORDER, X, y)
    _, rc = c.predict_setup(synth.default_thetas(KIND, D))
    assert rc == abi.OK
    mmax = max(sizes)
    lines = [f"# N={N} d={D} Matern 5/2 order {ORDER}, M device-resident queries in one block; medians of {REPS} after {WARM}, host time of call + synchronisation"]
    buf = c.dev_alloc((mmax * (D + 2) + mmax * mmax) * 8)
    try:
        c.upload(buf, synth.queries(mmax, D, 5))
        mean, var, cov = buf.value + mmax * D * 8, buf.value + mmax * (D + 1) * 8, buf.value + mmax * (D + 2) * 8
        for M in sizes:
            def batch():
                c.predict_dev(M, buf, mean, var)

            def pcov():
                c.predict_cov_dev(M, buf, mean, cov)

            ms_batch = wall(c, batch)
            ms_cov = wall(c, pcov)
            ms_batch2 = wall(c, batch)
            base = min(ms_batch, ms_batch2)
            expect = 1.0 + M / N
            lines.append(f"M={M:6d}  prediction sweep before / after {ms_batch:9.3f} / {ms_batch2:9.3f} ms   gpemu_predict_cov_dev {ms_cov:9.3f} ms   "
                         f"ratio {ms_cov / base:6.3f}   expected (1 + M/N) {expect:5.3f}   ratio / expected {ms_cov / base / expect:5.3f}"
                         + ("   (accepted up to 1.5)" if M >= 4096 else "   (no acceptance below M = 4096)"))
            for name, k in (("GPEMU_PROF_GEMM", abi.PROF_GEMM), ("GPEMU_PROF_FILL", abi.PROF_FILL), ("GPEMU_PROF_COV", abi.PROF_COV)):
                ms, n, fl = prof(c, k, pcov)
                rate = f"  {fl / ms * 1e-9:7.2f} TFLOP/s" if k == abi.PROF_GEMM and ms > 0 else ""
                lines.append(f"          of the entry, {name:16s} {ms:9.3f} ms / call  {n} launches{rate}")
            ms, n, fl = prof(c, abi.PROF_GEMM, batch)
            lines.append(f"          of the prediction sweep, GPEMU_PROF_GEMM {ms:9.3f} ms / call  {n} launches  {fl / ms * 1e-9:7.2f} TFLOP/s")
    finally:
        c.dev_free(buf)
        c.close()
    out = open(a.out, "a") if a.out else None
    for line in lines:
        print(line, flush=True)
        if out:
            out.write(line + "\n")
    if out:
        out.close()


if __name__ == "__main__":
    main()
