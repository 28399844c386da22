#!/usr/bin/env python3
"""What the input measure costs in the closed-form sensitivity entries (gpemu_sens_set_measure) on one GPU:
gpemu_sens_cov_dev, gpemu_sens_post_dev, gpemu_sens_pairs_dev and gpemu_sens_pairs_post_dev under all-uniform, all-Gaussian and
half-and-half kinds (the first d / 2 coordinates uniform, the others Gaussian), on one context, every ratio within one run.

    timeout -k 10 900 python tools/sens_measure_profile.py [--out FILE] [--cases 4096x8,8192x8,4096x16]

Model: synth.design(N, d), power-exponential, order 1, the supplied thetas (lengths 0.6).  Uniform coordinates: the design's own
range; Gaussian coordinates: mean at the centre of that range, sd 0.3 of it.

Per entry and measure: HIP events on the context's stream around the launches (GPEMU_PROF_SENS, GPEMU_PROF_SENS_POST), median of
7 calls after 3 warm-up calls; the N x N sweep alone from one call's GPEMU_PROF_DUMP lines.  The corner C^-1 = U U^T is built by
the first post call of a set-up, which is a warm-up call here.

Expectation (instruction counts: erf 57, exp 19, about 20 others per pair and coordinate): an all-Gaussian sweep takes 0.25 to
0.4 of the all-uniform one, the mixed one lies in between.  Condition: all-Gaussian is not slower than all-uniform at any size.
No time is a pass criterion of a test."""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madaiemulator_amd import abi, synth  # noqa: E402
from sens_profile import dumped  # noqa: E402

KIND, ORDER, SEED = 1, 1, 20261003 + 2
MEASURES = ("uniform", "gauss", "half")


def kinds(name, d):
    if name == "uniform":
        return np.zeros(d, dtype=np.int32)
    if name == "gauss":
        return np.ones(d, dtype=np.int32)
    return (np.arange(d) >= d // 2).astype(np.int32)


def timed(c, cls, call):
    """-> (median ms of the entry's launches, {tag: ms} of one call)"""
    for _ in range(3):
        call()
    c.sync()
    ev = []
    for _ in range(7):
        c.prof_begin(cls)
        call()
        ev.append(c.prof_end()["ms"])
    return statistics.median(ev), dict(dumped(c, cls, call))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="append the lines to this file as well")
    ap.add_argument("--cases", default="4096x8,8192x8,4096x16")
    a = ap.parse_args()
    lines = [f"# power-exponential, order {ORDER}, lengths 0.6; uniform coordinates on the design's range, Gaussian ones N(centre, (0.3 range)^2); "
             "half: the first d / 2 coordinates uniform, the others Gaussian; HIP events around the launches, median of 7 after 3; "
             "sweep: the N x N launch(es) alone; ratios against the all-uniform figure of the same run"]
    c = abi.Context(0)
    try:
        for case in a.cases.split(","):
            N, d = (int(v) for v in case.split("x"))
            npairs = d * (d - 1) // 2
            X, y = synth.design(N, d, SEED)
            c.set_model(KIND, ORDER, X, y)
            _, rc = c.predict_setup(synth.default_thetas(KIND, d))
            assert rc == abi.OK
            blo, bhi = X.min(axis=0), X.max(axis=0)
            out = c.dev_alloc(8 * (3 + 2 * d + npairs))
            try:
                entries = (("gpemu_sens_cov_dev", abi.PROF_SENS, "sens_sweep", lambda lo, hi: c.sens_cov_dev(lo, hi, out)),
                           ("gpemu_sens_post_dev", abi.PROF_SENS_POST, "sens_sweep_weighted", lambda lo, hi: c.sens_post_dev(lo, hi, out)),
                           ("gpemu_sens_pairs_dev", abi.PROF_SENS, "sens_pair_sweep", lambda lo, hi: c.sens_pairs_dev(lo, hi, out)),
                           ("gpemu_sens_pairs_post_dev", abi.PROF_SENS_POST, "sens_pair_sweep_weighted", lambda lo, hi: c.sens_pairs_post_dev(lo, hi, out)))
                for name, cls, sweep_tag, call in entries:
                    res = {}
                    for mn in MEASURES:
                        k = kinds(mn, d)
                        c.sens_set_measure(k)
                        lo = np.where(k == 1, (blo + bhi) / 2, blo)
                        hi = np.where(k == 1, 0.3 * (bhi - blo), bhi)
                        res[mn] = timed(c, cls, lambda: call(lo, hi))
                    u_ms, u_parts = res["uniform"]
                    text = f"N={N} d={d}: {name:26s}"
                    for mn in MEASURES:
                        ms, parts = res[mn]
                        text += (f" | {mn} {ms:8.3f} ms (sweep {parts[sweep_tag]:8.3f})" +
                                 ("" if mn == "uniform" else f" -> entry / uniform {ms / u_ms:5.2f}, sweep / uniform {parts[sweep_tag] / u_parts[sweep_tag]:5.2f}"))
                    lines.append(text)
                    print(text, flush=True)
            finally:
                c.dev_free(out)
                c.sens_set_measure(None)
    finally:
        c.close()
    if a.out:
        with open(a.out, "a") as fo:
            fo.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
