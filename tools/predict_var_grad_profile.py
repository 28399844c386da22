#!/usr/bin/env python3
"""The variance-gradient entry against the prediction sweep on one GPU at BASELINE configs[2] (N=8192, d=8, Matern 5/2, order 1).

    timeout -k 10 600 python tools/predict_var_grad_profile.py [--out FILE] [--queries M]

M = 131 072 device-resident queries through gpemu_predict_var_grad_dev and through gpemu_predict_batch_dev (the unchanged
prediction sweep: the yardstick) in one process: medians of 25 timed calls after 5 warm-up calls, each call timed on the host
from its first enqueue to the end of a stream synchronisation.  Then the entry's launches by profiling class (GPEMU_PROF_GEMM:
its two products; GPEMU_PROF_VAR_GRAD: the fused sweep and its finish; GPEMU_PROF_FILL: the k-vectors), what central
differences cost before (2 d + 1 prediction sweeps), and ONE query through both entries."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madaiemulator_amd import abi, synth  # noqa: E402

KIND, ORDER, N, D, SEED = 3, 1, 8192, 8, 20261003 + 2
WARM, REPS, BLOCK = 5, 25, 16384


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
    """median over reps of the summed event time of the launches of class cls in one call, and their number"""
    ms, n = [], 0
    for _ in range(reps):
        c.prof_begin(cls)
        call()
        p = c.prof_end()
        ms.append(p["ms"])
        n = p["n"]
    return statistics.median(ms), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="append the lines to this file as well")
    ap.add_argument("--queries", type=int, default=131072)
    a = ap.parse_args()
    M = a.queries
    X, y = synth.design(N, D, SEED)
    c = abi.Context(0)
    c.set_model(KIND, ORDER, X, y)
    _, rc = c.predict_setup(synth.default_thetas(KIND, D))
    assert rc == abi.OK
    nblocks = (M + BLOCK - 1) // BLOCK
    buf = c.dev_alloc(M * (2 * D + 2) * 8)
    try:
        c.upload(buf, synth.queries(M, D, 5))
        mean, var, grad = buf.value + M * D * 8, buf.value + M * (D + 1) * 8, buf.value + M * (D + 2) * 8

        def batch(m=M):
            c.predict_dev(m, buf, mean, var)

        def vgrad(m=M):
            c.predict_var_grad_dev(m, buf, mean, var, grad)

        ms_batch = wall(c, batch)
        ms_grad = wall(c, vgrad)
        ms_batch2 = wall(c, batch)
        cls = [(name, prof(c, k, vgrad)) for name, k in (("GPEMU_PROF_GEMM", abi.PROF_GEMM), ("GPEMU_PROF_VAR_GRAD", abi.PROF_VAR_GRAD),
                                                         ("GPEMU_PROF_FILL", abi.PROF_FILL))]
        gemm_batch = prof(c, abi.PROF_GEMM, batch)
        one_batch = wall(c, lambda: batch(1))
        one_grad = wall(c, lambda: vgrad(1))
    finally:
        c.dev_free(buf)
        c.close()
    base = min(ms_batch, ms_batch2)
    lines = [
        f"# N={N} d={D} Matern 5/2 order {ORDER}, M={M} device-resident queries, {nblocks} blocks of {BLOCK}; medians of {REPS} after {WARM}, host time of call + synchronisation",
        f"prediction sweep (gpemu_predict_batch_dev), before     {ms_batch:10.3f} ms / call  {ms_batch / nblocks:9.3f} ms / block",
        f"variance-gradient entry (gpemu_predict_var_grad_dev)   {ms_grad:10.3f} ms / call  {ms_grad / nblocks:9.3f} ms / block",
        f"prediction sweep, after                                {ms_batch2:10.3f} ms / call",
        f"ratio entry / one prediction sweep                     {ms_grad / base:10.3f}   (expected 2 - 2.5, accepted up to 3)",
        f"central differences: {2 * D + 1} prediction sweeps              {(2 * D + 1) * base:10.3f} ms           {(2 * D + 1) * base / ms_grad:9.1f} x the entry",
    ]
    for name, (ms, n) in cls:
        lines.append(f"  of the entry, {name:22s}             {ms:10.3f} ms / call  {n} launches")
    lines.append(f"  of the prediction sweep, GPEMU_PROF_GEMM               {gemm_batch[0]:10.3f} ms / call  {gemm_batch[1]} launches")
    lines.append(f"ONE query: prediction sweep {one_batch * 1e3:9.1f} us, variance-gradient entry {one_grad * 1e3:9.1f} us (one 64-row tile through the block kernels)")
    out = open(a.out, "a") if a.out else None
    for line in lines:
        print(line, flush=True)
        if out:
            out.write(line + "\n")
    if out:
        out.close()


if __name__ == "__main__":
    main()
