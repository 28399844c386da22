#!/usr/bin/env python3
"""Second-order closed forms (gpemu_sens_pairs_dev, gpemu_sens_pairs_post_dev) on one GPU: their time beside gpemu_sens_cov_dev and
gpemu_sens_post_dev on the same context, and what the route a user had before costs -- pick-freeze through
gpemu_predict_mean_dev, once per pair of parameters.

    timeout -k 10 1100 python tools/sens_pairs_profile.py [--out FILE] [--cases 8192x8,4096x8,4096x16]

Model: synth.design(N, d), power-exponential, order 1, the supplied thetas (lengths 0.6); box: the design's own range.

The four entries: HIP events on the context's stream around their launches (GPEMU_PROF_SENS, GPEMU_PROF_SENS_POST), median of 7
calls after 3 warm-up calls, the launches one by one from one call's GPEMU_PROF_DUMP lines (the two launches of a pair sweep at
d > 8 are one line).  The corner C^-1 = U U^T is built by the first post call of a set-up, which is a warm-up call here.

Pick-freeze: n = 100 000 base points A, a second sample B, and per pair (j, k) the hybrid that takes x_j and x_k from A and the
rest from B: (npairs + 2) n evaluations of the mean, device-resident queries and results (generation and upload NOT timed),
host time of the npairs + 2 calls + synchronisation, median of 3 after 1.  From them V_jk / V by E[f_A f_AB] - E0^2; the line
gives the largest deviation from the closed form.  No time is a pass criterion."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madaiemulator_amd import abi, synth  # noqa: E402
from sens_post_profile import events  # noqa: E402
from sens_profile import dumped, wall  # noqa: E402

KIND, ORDER, SEED = 1, 1, 20261003 + 2
NBASE = 100000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="append the lines to this file as well")
    ap.add_argument("--cases", default="8192x8,4096x8,4096x16")
    a = ap.parse_args()
    lines = [f"# power-exponential, order {ORDER}, lengths 0.6, box = the design's range; HIP events around the launches, median of 7 after 3; "
             f"pick-freeze: n = {NBASE} base points through gpemu_predict_mean_dev, host time + synchronisation, median of 3 after 1"]
    c = abi.Context(0)
    try:
        for case in a.cases.split(","):
            N, d = (int(v) for v in case.split("x"))
            npairs = d * (d - 1) // 2
            X, y = synth.design(N, d, SEED)
            c.set_model(KIND, ORDER, X, y)
            _, rc = c.predict_setup(synth.default_thetas(KIND, d))
            assert rc == abi.OK
            lo, hi = X.min(axis=0), X.max(axis=0)
            out = c.dev_alloc(8 * max(npairs, 3 + 2 * d))
            try:
                calls = dict(pairs=(abi.PROF_SENS, lambda: c.sens_pairs_dev(lo, hi, out)), cov=(abi.PROF_SENS, lambda: c.sens_cov_dev(lo, hi, out)),
                             pairs_post=(abi.PROF_SENS_POST, lambda: c.sens_pairs_post_dev(lo, hi, out)),
                             post=(abi.PROF_SENS_POST, lambda: c.sens_post_dev(lo, hi, out)))
                ms = {k: events(c, cls, call) for k, (cls, call) in calls.items()}
                parts = {k: dumped(c, cls, call) for k, (cls, call) in calls.items()}
                c.sens_cov_dev(lo, hi, out)
                V = c.download(out, (3,))[2]
                c.sens_pairs_dev(lo, hi, out)
                pair = c.download(out, (npairs,))
            finally:
                c.dev_free(out)
            for k, other in (("pairs", "cov"), ("pairs_post", "post")):
                lines.append(f"N={N} d={d}: gpemu_sens_{k}_dev {ms[k]:9.3f} ms (" + ", ".join(f"{t} {v:.3f}" for t, v in parts[k]) +
                             f"); gpemu_sens_{other}_dev {ms[other]:9.3f} ms (" + ", ".join(f"{t} {v:.3f}" for t, v in parts[other]) +
                             f") -> {k} / {other} {ms[k] / ms[other]:5.2f}")
                print(lines[-1], flush=True)
            # pick-freeze through the mean-only sweep, one index set per pair
            rng = np.random.default_rng(7)
            A, B = (lo + (hi - lo) * rng.random((NBASE, d)) for _ in range(2))
            Q = [A, B]
            for j in range(d):
                for k in range(j + 1, d):
                    h = B.copy()
                    h[:, [j, k]] = A[:, [j, k]]
                    Q.append(h)
            Q = np.ascontiguousarray(np.concatenate(Q))
            M = Q.shape[0]
            buf = c.dev_alloc(8 * (M * d + M))
            try:
                c.upload(buf, Q)
                mean_dev = abi.C.c_void_p(buf.value + 8 * M * d)

                def mc():
                    for b in range(npairs + 2):
                        c.predict_mean_dev(NBASE, abi.C.c_void_p(buf.value + 8 * b * NBASE * d), abi.C.c_void_p(mean_dev.value + 8 * b * NBASE))

                mc_ms = wall(c.sync, mc, 1, 3)
                f = c.download(mean_dev, (npairs + 2, NBASE))
            finally:
                c.dev_free(buf)
            fA = f[0]
            e0, Vmc = fA.mean(), fA.var()
            S = np.array([np.mean(fA * f[2 + p]) - e0 * f[2 + p].mean() for p in range(npairs)]) / Vmc
            lines.append(f"          pick-freeze, (npairs + 2) n = {M} means: {mc_ms:9.3f} ms ({mc_ms / (npairs + 2):.2f} ms per index set) -> pick-freeze / "
                         f"closed form {mc_ms / ms['pairs']:6.2f}; largest error of V_jk / V: {np.max(np.abs(S - pair / V)):.2e} "
                         f"(V_jk / V from {np.min(pair / V):.3e} to {np.max(pair / V):.3e})")
            print(lines[-1], flush=True)
    finally:
        c.close()
    if a.out:
        with open(a.out, "a") as fo:
            fo.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
