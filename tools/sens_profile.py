#!/usr/bin/env python3
"""Closed-form sensitivity analysis (gpemu_sens_cov_dev) against pick-freeze Monte Carlo through gpemu_predict_mean_dev, the path
a user had before, and against the vector-fp64 bound of its sweep, on one GPU.

    timeout -k 10 900 python tools/sens_profile.py [--out FILE] [--cases 4096x8,8192x8,4096x16]

Model: synth.design(N, d), power-exponential, order 1, the supplied thetas (lengths 0.6); box: the design's own range.

gpemu_sens_cov_dev: HIP events on the context's stream around its three launches (GPEMU_PROF_SENS), median of 7 calls after 3
warm-up calls, the launches one by one from one call's GPEMU_PROF_DUMP lines; beside it the host time of call + stream
synchronisation, median of 15 after 3.

Pick-freeze: n = 100 000 base points A, a second sample B, and per coordinate j the hybrid that takes x_j from B and the rest
from A: (d + 2) n evaluations of the mean, device-resident queries and results (their generation and upload are NOT timed),
host time of the d + 2 calls + synchronisation, median of 5 after 2.  From them first-order indices by Saltelli's estimator,
E[f_B (f_ABj - f_A)] / V, and total indices by Jansen's, E[(f_A - f_ABj)^2] / 2 V; the line gives their largest deviation from
the closed form -- the sampling error a user of that route lives with.

Bound: the sweep evaluates 2 N^2 d erf or erfc; the device's erf compiles to ERF_F64 = 57 fp64 vector instructions (erfc: 71), a
CU issues 4 x 16 fp64 lanes per clock, 256 CUs at 2.4 GHz: 3.93e13 lane-instructions per second.  bound = 2 N^2 d ERF_F64 /
3.93e13.  The exp, the products and the sums of a pair are not in it.  No time is a pass criterion."""
import argparse
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madaiemulator_amd import abi, synth  # noqa: E402

KIND, ORDER, SEED = 1, 1, 20261003 + 2
NBASE = 100000
ERF_F64 = 57
LANE_RATE = 256 * 4 * 16 * 2.4e9


def wall(sync, call, warm, reps):
    for _ in range(warm):
        call()
    sync()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        sync()
        ms.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ms)


def dumped(c, cls, call):
    """the [gpemu prof] lines of one call under class cls -> list of (tag, ms)"""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.environ["GPEMU_PROF_DUMP"] = "1"
        os.dup2(tmp.fileno(), 2)
        try:
            c.prof_begin(cls)
            call()
            c.prof_end()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
            del os.environ["GPEMU_PROF_DUMP"]
        tmp.seek(0)
        text = tmp.read().decode()
    return [(m.group(1), float(m.group(2))) for m in re.finditer(r"\[gpemu prof\] (\S+).* ms=([0-9.]+)", text)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="append the lines to this file as well")
    ap.add_argument("--cases", default="4096x8,8192x8,4096x16")
    a = ap.parse_args()
    lines = [f"# power-exponential, order {ORDER}, lengths 0.6, box = the design's range; closed form: HIP events around the three launches, "
             f"median of 7 after 3; pick-freeze: n = {NBASE} base points through gpemu_predict_mean_dev, host time + synchronisation, median of 5 after 2"]
    c = abi.Context(0)
    try:
        for case in a.cases.split(","):
            N, d = (int(v) for v in case.split("x"))
            X, y = synth.design(N, d, SEED)
            c.set_model(KIND, ORDER, X, y)
            _, rc = c.predict_setup(synth.default_thetas(KIND, d))
            assert rc == abi.OK
            lo, hi = X.min(axis=0), X.max(axis=0)
            out = c.dev_alloc(8 * (3 + 2 * d))
            try:
                def sens():
                    c.sens_cov_dev(lo, hi, out)

                for _ in range(3):
                    sens()
                c.sync()
                ev = []
                for _ in range(7):
                    c.prof_begin(abi.PROF_SENS)
                    sens()
                    p = c.prof_end()
                    ev.append(p["ms"])
                ms = statistics.median(ev)
                parts = dumped(c, abi.PROF_SENS, sens)
                host = wall(c.sync, sens, 3, 15)
                o = c.download(out, (3 + 2 * d,))
            finally:
                c.dev_free(out)
            V, first, total = o[2], o[3:3 + d] / o[2], (o[2] - o[3 + d:]) / o[2]
            bound = 2.0 * N * N * d * ERF_F64 / LANE_RATE * 1e3
            lines.append(f"N={N} d={d}: gpemu_sens_cov_dev {ms:9.3f} ms (3 launches; " + ", ".join(f"{t} {v:.3f}" for t, v in parts) +
                         f"); host call + sync {host:9.3f} ms; vector-fp64 bound of 2 N^2 d erf {bound:7.3f} ms -> sweep / bound "
                         f"{dict(parts).get('sens_sweep', ms) / bound:5.1f}; V {V:.6g} first {np.array2string(first, precision=4, max_line_width=10000)} "
                         f"total {np.array2string(total, precision=4, max_line_width=10000)}")
            print(lines[-1], flush=True)
            # pick-freeze through the mean-only sweep
            rng = np.random.default_rng(7)
            A, B = (lo + (hi - lo) * rng.random((NBASE, d)) for _ in range(2))
            Q = [A, B]
            for j in range(d):
                h = A.copy()
                h[:, j] = B[:, j]
                Q.append(h)
            Q = np.ascontiguousarray(np.concatenate(Q))
            M = Q.shape[0]
            buf = c.dev_alloc(8 * (M * d + M))
            try:
                c.upload(buf, Q)
                mean_dev = abi.C.c_void_p(buf.value + 8 * M * d)

                def mc():
                    for b in range(d + 2):
                        c.predict_mean_dev(NBASE, abi.C.c_void_p(buf.value + 8 * b * NBASE * d), abi.C.c_void_p(mean_dev.value + 8 * b * NBASE))

                mc_ms = wall(c.sync, mc, 2, 5)
                f = c.download(mean_dev, (d + 2, NBASE))
            finally:
                c.dev_free(buf)
            fA, fB = f[0], f[1]
            Vmc = fA.var()
            S = np.array([np.mean(fB * (f[2 + j] - fA)) for j in range(d)]) / Vmc
            T = np.array([0.5 * np.mean((fA - f[2 + j]) ** 2) for j in range(d)]) / Vmc
            lines.append(f"          pick-freeze, (d + 2) n = {M} means: {mc_ms:9.3f} ms -> pick-freeze / closed form {mc_ms / ms:6.2f}; largest index error: "
                         f"first {np.max(np.abs(S - first)):.2e} total {np.max(np.abs(T - total)):.2e} (smallest first-order index {first.min():.2e}), "
                         f"V off by {abs(Vmc - V) / V:.2e}")
            print(lines[-1], flush=True)
    finally:
        c.close()
    if a.out:
        with open(a.out, "a") as fo:
            fo.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
