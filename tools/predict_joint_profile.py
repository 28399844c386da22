#!/usr/bin/env python3
"""Hold-out validation and joint draws against the joint-covariance entry on one GPU at BASELINE configs[2] (N=8192, d=8,
Matern 5/2, order 1).

    timeout -k 10 900 python tools/predict_joint_profile.py [--out FILE] [--sizes 4096,16384] [--draws 1,64,1024]

For each M, M device-resident queries through gpemu_predict_joint_factor_dev (three observation rows, noise on the diagonal)
and through gpemu_predict_cov_dev on the same queries (the entry it extends: the yardstick) in one process, alternating, each
timed before and after the other: medians of 15 timed calls after 3 warm-up calls, each call timed on the host from its
first enqueue to the end of a stream synchronisation.  Then gpemu_predict_joint_draw_dev at every ndraw, the same way.  Then
the factor entry's launches by profiling class, HIP events on the context's stream around every launch of the class (the
whole factorisation under GPEMU_PROF_POTRF): medians of 5 calls.

Flop model: M N^2 for the sweep, M^2 N for the symmetric product, M^3 / 3 for the factorisation (ONE matrix: expect the
one-evaluation rate of DESIGN.md section 7, not the batch rate), ndraw M^2 for a block of draws.  No time is a pass criterion:
the lines give the measured times, the rates they imply and, for the factor entry, its time over the covariance entry's
against the model's (M N^2 + M^2 N + M^3 / 3) / (M N^2 + M^2 N)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madaiemulator_amd import abi, synth  # noqa: E402

KIND, ORDER, N, D, SEED = 3, 1, 8192, 8, 20261003 + 2
WARM, REPS, NOBS = 3, 15, 3


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
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--draws", default="1,64,1024")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    draws = [int(s) for s in a.draws.split(",")]
    X, y = synth.design(N, D, SEED)
    th = synth.default_thetas(KIND, D)
    c = abi.Context(0)
    c.set_model(KIND, ORDER, X, y)
    _, rc = c.predict_setup(th)
    assert rc == abi.OK
    mmax, dmax = max(sizes), max(draws)
    lines = [f"# N={N} d={D} Matern 5/2 order {ORDER}, M device-resident queries, {NOBS} observation rows, noise on the diagonal; medians of "
             f"{REPS} after {WARM}, host time of call + synchronisation; classes: HIP events around the launches, medians of 5"]
    rng = np.random.default_rng(7)
    sizes_el = dict(xq=mmax * D, noise=mmax, yobs=NOBS * mmax, mean=mmax, var=mmax, werr=NOBS * mmax, stat=1 + NOBS + 1, info=2,
                    z=dmax * mmax, out=dmax * mmax, cov=mmax * mmax)
    buf = c.dev_alloc(8 * sum(sizes_el.values()))
    try:
        p, off = {}, 0
        for k, n in sizes_el.items():
            p[k] = buf.value + 8 * off
            off += n
        c.upload(p["xq"], synth.queries(mmax, D, 5))
        c.upload(p["noise"], 0.05 * (th[0] + th[1]) * (1.0 + rng.random(mmax)))
        c.upload(p["z"], rng.standard_normal(dmax * mmax))
        for M in sizes:
            def pcov():
                c.predict_cov_dev(M, p["xq"], p["mean"], p["cov"])

            def factor():
                c.predict_joint_factor_dev(M, p["xq"], p["noise"], NOBS, p["yobs"], p["mean"], p["var"], p["werr"], p["stat"], p["info"])

            pcov()
            c.sync()
            mean = c.download(p["mean"], (M,))
            c.upload(p["yobs"], (mean + rng.standard_normal((NOBS, M))).ravel())     # rows of M, as the call reads them
            ms_cov = wall(c, pcov)
            ms_fac = wall(c, factor)
            ms_cov2 = wall(c, pcov)
            ms_fac2 = wall(c, factor)
            info = int(c.download(p["info"], (1,), dtype=np.int32)[0])
            stat = c.download(p["stat"], (1 + NOBS,))
            assert info >= 0x7f7f7f7f and np.all(np.isfinite(stat)), ("the factorisation failed", info, stat)
            base, fac = min(ms_cov, ms_cov2), min(ms_fac, ms_fac2)
            f_cov = float(M) * N * N + float(M) * M * N
            f_pot = float(M) ** 3 / 3.0
            lines.append(f"M={M:6d}  gpemu_predict_cov_dev before / after {ms_cov:9.3f} / {ms_cov2:9.3f} ms   gpemu_predict_joint_factor_dev "
                         f"{ms_fac:9.3f} / {ms_fac2:9.3f} ms   ratio {fac / base:6.3f}   flop model {(f_cov + f_pot) / f_cov:5.3f}   "
                         f"ratio / model {fac / base / ((f_cov + f_pot) / f_cov):5.3f}   whole entry {(f_cov + f_pot) / fac * 1e-9:6.2f} TFLOP/s   "
                         f"logdet {stat[0]:.6g} maha/M {stat[1] / M:.4f}")
            for name, k in (("GPEMU_PROF_POTRF", abi.PROF_POTRF), ("GPEMU_PROF_GEMM", abi.PROF_GEMM), ("GPEMU_PROF_LEAF", abi.PROF_LEAF),
                            ("GPEMU_PROF_FILL", abi.PROF_FILL), ("GPEMU_PROF_COV", abi.PROF_COV), ("GPEMU_PROF_JOINT", abi.PROF_JOINT)):
                ms, n, fl = prof(c, k, factor)
                rate = f"  {fl / ms * 1e-9:7.2f} TFLOP/s" if k in (abi.PROF_GEMM, abi.PROF_POTRF) and ms > 0 else ""
                lines.append(f"          of the factor entry, {name:16s} {ms:9.3f} ms / call  {n} launches{rate}")
            factor()
            for nd in draws:
                def draw():
                    c.predict_joint_draw_dev(nd, p["z"], p["out"])

                ms = wall(c, draw)
                msj, nj, _ = prof(c, abi.PROF_JOINT, draw)
                msg, ng, fl = prof(c, abi.PROF_GEMM, draw)
                lines.append(f"          gpemu_predict_joint_draw_dev ndraw={nd:5d} {ms:9.3f} ms / call   staging {msj:8.3f} ms ({nj} launches)   "
                             f"product {msg:8.3f} ms ({ng} launches, {fl / msg * 1e-9:6.2f} TFLOP/s of ndraw M^2 flops)")
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
