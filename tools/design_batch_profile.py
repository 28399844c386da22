#!/usr/bin/env python3
"""Greedy batches of K runs (gpemu_design_batch_dev) on one GPU: the first pass, the time per pick split into its launches, the
column kernel's share of the memory bandwidth, and what the route a user had before costs.

    timeout -k 10 900 python tools/design_batch_profile.py [--out FILE] [--cases 4096x8,8192x8,4096x16] [--contexts 1,8]

Model: synth.design(N, d), power-exponential, order 1, the supplied thetas (lengths 0.6), every context the same model (the time
does not depend on the training values); box: the design's own range; M = 16 384 device-resident candidates, uniform in the
box (generation and upload NOT timed); nbatch = 64.

Whole call: host time of the enqueue plus the synchronisation, median of 5 after 2.  The launches of ctxs[0] by HIP events
(GPEMU_PROF_DESIGN) from one call's GPEMU_PROF_DUMP lines: the first pass is gpemu_design_gain_dev's own launches and the rows
of w (its three products are GPEMU_PROF_GEMM's, not in this split: `first pass, whole` is the wall time of a batch of one pick
minus that pick); per pick the mean over the 64 picks of the gather, the column kernel, the update and the arg-max.  The column
kernel's bandwidth is 24 M' Np bytes over its mean time, against 8 TB/s.  With events between the launches the streams of
several contexts do not overlap as they do unprofiled: the whole-call time is the one that counts for nctx > 1.

gpemu_design_gain_dev itself, on the same candidates: whole call, median of 7 after 3 with the smallest and the largest, to be
held against profiles/design.txt's figure for the commit before this entry existed (the launches are the same).

The route before: gpemu_design_gain for the first pick, then for every later pick a refit on N + j points per candidate
(set_model + gpemu_predict_setup + gpemu_sens_post_dev); 4 candidates timed at j = 1 (N + 2 points), their mean MULTIPLIED by M and by nbatch - 1
-- not run.  No time is a pass criterion."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madaiemulator_amd import abi, synth  # noqa: E402
from sens_profile import dumped, wall  # noqa: E402

KIND, ORDER, SEED = 1, 1, 20261020
M, NBATCH, NREFIT = 16384, 64, 4
PEAK = 8.0e12


def spread(sync, call, warm, reps):
    for _ in range(warm):
        call()
    sync()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        sync()
        ms.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="append the lines to this file as well")
    ap.add_argument("--cases", default="4096x8,8192x8,4096x16")
    ap.add_argument("--contexts", default="1,8")
    a = ap.parse_args()
    ncs = [int(v) for v in a.contexts.split(",")]
    lines = [f"# power-exponential, order {ORDER}, lengths 0.6, box = the design's range, M = {M} resident candidates, nbatch = {NBATCH}; whole call: "
             f"host time + synchronisation, median of 5 after 2; launches: HIP events of one call on ctxs[0]"]
    ctxs = [abi.Context(0) for _ in range(max(ncs))]
    c = ctxs[0]
    try:
        for case in a.cases.split(","):
            N, d = (int(v) for v in case.split("x"))
            X, y = synth.design(N, d, SEED)
            th = synth.default_thetas(KIND, d)
            lo, hi = X.min(axis=0), X.max(axis=0)
            Q = np.ascontiguousarray(lo + (hi - lo) * np.random.default_rng(11).random((M, d)))
            Np = (N + 63) // 64 * 64
            for nc in ncs:
                use = ctxs[:nc]
                for cc in use:
                    cc.set_model(KIND, ORDER, X, y)
                    _, rc = cc.predict_setup(th)
                    assert rc == abi.OK
                sizes = [8 * M * d, 4 * NBATCH + 4, 8 * NBATCH, 8 * NBATCH * nc, 8 * M, 8 * M, 8 * 3 * M]
                bufs = [c.dev_alloc(s) for s in sizes]
                try:
                    c.upload(bufs[0], Q)

                    def batch(nb=NBATCH):
                        abi.design_batch_dev(use, lo, hi, M, bufs[0], nb, bufs[1], bufs[2], bufs[3], bufs[4], bufs[5])

                    whole = wall(c.sync, batch, 2, 5)
                    one = wall(c.sync, lambda: batch(1), 2, 5)
                    parts = dumped(c, abi.PROF_DESIGN, batch)
                    per = {t: statistics.mean([v for tag, v in parts if tag == t] or [0.0])
                           for t in ("design_gather", "design_column", "design_update", "design_argmax")}
                    first = sum(v for tag, v in parts if tag not in per)
                    pick = (whole - one) / (NBATCH - 1)
                    frac = 24.0 * M * Np / (per["design_column"] * 1e-3) / PEAK
                    lines.append(f"N={N} d={d} nctx={nc}: gpemu_design_batch_dev {whole:9.3f} ms whole call ({NBATCH} picks); first pass, whole (a batch of one pick "
                                 f"less one pick) {one - pick:9.3f} ms, its own launches on ctxs[0] {first:7.3f} ms of which the rows of w "
                                 f"{sum(v for t, v in parts if t == 'design_wrows'):7.3f} ms; per pick {pick:7.3f} ms whole = gather {per['design_gather']:.3f} + column "
                                 f"{per['design_column']:.3f} + update {per['design_update']:.3f} + arg-max {per['design_argmax']:.3f} ms (events, ctxs[0]); column kernel "
                                 f"{24.0 * M * Np / 1e9:.2f} GB per pick and context -> {100 * frac:5.1f} % of 8 TB/s")
                    print(lines[-1], flush=True)
                    if nc == 1:
                        g_dev, n_dev, v_dev = (abi.C.c_void_p(bufs[6].value + 8 * M * k) for k in range(3))
                        med, lo_ms, hi_ms = spread(c.sync, lambda: c.design_gain_dev(lo, hi, M, bufs[0], g_dev, n_dev, v_dev), 3, 7)
                        lines.append(f"          gpemu_design_gain_dev on the same candidates {med:9.3f} ms whole call (median of 7 after 3; {lo_ms:.3f} .. {hi_ms:.3f})")
                        print(lines[-1], flush=True)
                finally:
                    for b in bufs:
                        c.dev_free(b)
                if nc == 1:
                    out = c.dev_alloc(8 * (3 + 2 * d))
                    try:
                        ms = []
                        for q in range(NREFIT + 1):
                            X2, y2 = np.vstack([X, Q[:1], Q[q + 1][None, :]]), np.append(y, [0.0, 0.0])

                            def refit():
                                c.set_model(KIND, ORDER, X2, y2)
                                c.predict_setup(th)
                                c.sens_post_dev(lo, hi, out)
                            t = wall(c.sync, refit, 0, 1)
                            if q:                                              # (the first one pays for the new shape's allocations)
                                ms.append(t)
                    finally:
                        c.dev_free(out)
                    each = statistics.mean(ms)
                    lines.append(f"          the route before: a refit on the design, the first pick and the candidate (N + 2 points) per candidate and pick, {NREFIT} candidates timed: {each:9.3f} ms each -> MULTIPLIED "
                                 f"by M = {M} and {NBATCH - 1} later picks: {each * M * (NBATCH - 1) / 1e3:11.1f} s (not run) against {whole / 1e3:7.3f} s")
                    print(lines[-1], flush=True)
    finally:
        for cc in ctxs:
            cc.close()
    if a.out:
        with open(a.out, "a") as fo:
            fo.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
