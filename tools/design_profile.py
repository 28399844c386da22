#!/usr/bin/env python3
"""Expected IMSE reduction of candidate runs (gpemu_design_gain_dev) on one GPU: where its time goes, what it costs beside
gpemu_predict_batch_dev on the same queries, and what the routes a user had before cost.

    timeout -k 10 900 python tools/design_profile.py [--out FILE] [--cases 4096x8,8192x8,4096x16]

Model: synth.design(N, d), power-exponential, order 1, the supplied thetas (lengths 0.6); box: the design's own range;
M = 16 384 device-resident candidates, uniform in the box (generation and upload NOT timed).

gpemu_design_gain_dev: the whole call as host time of the enqueue plus the synchronisation, median of 7 after 3 (K resident); its
own launches by HIP events (GPEMU_PROF_DESIGN) and its three products (GPEMU_PROF_GEMM), each the median of 7 calls after 3, the
launches one by one from one call's GPEMU_PROF_DUMP lines.  The K rebuild is the design_kmat launch of the first call after a
set-up, measured once per case.  Beside it gpemu_predict_batch_dev on the same queries (host time + synchronisation, the same
medians); the flop model is three M N^2 products plus 2 M N d pair factors against the sweep's one.

Refit route: gpemu_predict_setup on the design with one candidate appended + gpemu_sens_post_dev, host time of 4 candidates, their
mean MULTIPLIED to M -- not run for all of them.  Monte-Carlo route: gpemu_predict_cov_dev on 64 candidates and n = 16 320 uniform
points x (its limit is 16 384 points a call), gain = mean_x cov(x, x*)^2 / cov(x*, x*) (its diagonal holds the nugget), host time + synchronisation,
median of 3 after 1; the line gives its largest error against the closed form relative to the largest gain.  No time is a pass
criterion."""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madaiemulator_amd import abi, synth  # noqa: E402
from sens_profile import dumped, wall  # noqa: E402
from sens_post_profile import events  # noqa: E402

KIND, ORDER, SEED = 1, 1, 20261020
M, NCAND_MC, NREFIT = 16384, 64, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="append the lines to this file as well")
    ap.add_argument("--cases", default="4096x8,8192x8,4096x16")
    a = ap.parse_args()
    lines = [f"# power-exponential, order {ORDER}, lengths 0.6, box = the design's range, M = {M} resident candidates; whole call: host time + "
             f"synchronisation, median of 7 after 3; launch classes: HIP events, median of 7 after 3"]
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
            rng = np.random.default_rng(11)
            Q = np.ascontiguousarray(lo + (hi - lo) * rng.random((M, d)))
            buf = c.dev_alloc(8 * (M * d + 3 * M))
            try:
                c.upload(buf, Q)
                g_dev = abi.C.c_void_p(buf.value + 8 * M * d)
                n_dev = abi.C.c_void_p(g_dev.value + 8 * M)
                v_dev = abi.C.c_void_p(n_dev.value + 8 * M)

                def gain():
                    c.design_gain_dev(lo, hi, M, buf, g_dev, n_dev, v_dev)

                first = dict(dumped(c, abi.PROF_DESIGN, gain))           # the first call of a set-up builds K
                whole = wall(c.sync, gain, 3, 7)
                own = events(c, abi.PROF_DESIGN, gain)
                gemm = events(c, abi.PROF_GEMM, gain)
                parts = dumped(c, abi.PROF_DESIGN, gain)
                gparts = dumped(c, abi.PROF_GEMM, gain)
                g = c.download(g_dev, (M,))
                pred = wall(c.sync, lambda: c.predict_dev(M, buf, n_dev, v_dev), 3, 7)
            finally:
                c.dev_free(buf)
            lines.append(f"N={N} d={d}: gpemu_design_gain_dev {whole:9.3f} ms whole call; its own launches {own:9.3f} ms (" +
                         ", ".join(f"{t} {v:.3f}" for t, v in parts) + f"); its three products {gemm:9.3f} ms (the first in two launches: " +
                         ", ".join(f"{v:.3f}" for _, v in gparts) + f"); K rebuild once per set-up and box {first.get('design_kmat', float('nan')):9.3f} ms")
            print(lines[-1], flush=True)
            model = (3.0 * M * N * N + 2.0 * M * N * d) / (1.0 * M * N * N)
            lines.append(f"          gpemu_predict_batch_dev on the same queries {pred:9.3f} ms -> gain / prediction {whole / pred:5.2f} "
                         f"(products alone {gemm / pred:5.2f}; flop model, pair factors at one flop each: {model:4.2f})")
            print(lines[-1], flush=True)
            # the refit route on a few candidates
            out = c.dev_alloc(8 * (3 + 2 * d))
            try:
                ms = []
                for q in range(NREFIT + 1):
                    X2, y2 = np.vstack([X, Q[q][None, :]]), np.append(y, 0.0)

                    def refit():
                        c.set_model(KIND, ORDER, X2, y2)
                        c.predict_setup(th)
                        c.sens_post_dev(lo, hi, out)
                    t = wall(c.sync, refit, 0, 1)
                    if q:                                                  # (the first one pays for the new shape's allocations)
                        ms.append(t)
            finally:
                c.dev_free(out)
            lines.append(f"          refit route (set_model + gpemu_predict_setup + gpemu_sens_post_dev), {NREFIT} candidates timed: {statistics.mean(ms):9.3f} ms each "
                         f"-> MULTIPLIED to M = {M}: {statistics.mean(ms) * M / 1e3:9.1f} s (not run) against {whole / 1e3:7.3f} s")
            print(lines[-1], flush=True)
            # Monte Carlo through the joint covariance
            c.set_model(KIND, ORDER, X, y)
            c.predict_setup(th)
            nx = 16384 - NCAND_MC
            P = np.ascontiguousarray(np.vstack([Q[:NCAND_MC], lo + (hi - lo) * rng.random((nx, d))]))
            buf = c.dev_alloc(8 * (16384 * d + 16384 * 16384))
            try:
                c.upload(buf, P)
                cov_dev = abi.C.c_void_p(buf.value + 8 * 16384 * d)
                mc_ms = wall(c.sync, lambda: c.predict_cov_dev(16384, buf, None, cov_dev), 1, 3)
                rows = c.download(cov_dev, (NCAND_MC, 16384))
            finally:
                c.dev_free(buf)
            mc = (rows[:, NCAND_MC:] ** 2).mean(axis=1) / rows[np.arange(NCAND_MC), np.arange(NCAND_MC)]     # (Sigma_pp holds the nugget)
            se = (rows[:, NCAND_MC:] ** 2).std(axis=1, ddof=1) / np.sqrt(nx) / rows[np.arange(NCAND_MC), np.arange(NCAND_MC)]
            lines.append(f"          Monte Carlo through gpemu_predict_cov_dev, {NCAND_MC} candidates x {nx} points: {mc_ms:9.3f} ms ({mc_ms / NCAND_MC:7.3f} ms a candidate "
                         f"against {whole / M * 1e3:7.3f} us) -> largest error in gain {np.max(np.abs(mc - g[:NCAND_MC])) / g[:NCAND_MC].max():.2e} of the largest gain "
                         f"(its own standard error up to {se.max() / g[:NCAND_MC].max():.2e}; median error over gain {np.median(np.abs(mc - g[:NCAND_MC]) / g[:NCAND_MC]):.2e})")
            print(lines[-1], flush=True)
    finally:
        c.close()
    if a.out:
        with open(a.out, "a") as fo:
            fo.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
