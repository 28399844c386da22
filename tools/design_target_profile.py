#!/usr/bin/env python3
"""Gain over a weighted set of target points (gpemu_design_target_gain_dev) on one GPU: where its time goes, what the target
set-up costs, and what the route a user had before costs.

    timeout -k 10 900 python tools/design_target_profile.py [--out FILE] [--cases 4096x8,8192x8,4096x16]

Model: synth.design(N, d), power-exponential, order 1, the supplied thetas (lengths 0.6); M = S = 16 384 device-resident candidates
and targets, uniform in the design's range, equal weights (generation and upload NOT timed); the panel width is the context's
(GPEMU_TARGET_PANEL, default 2048).

gpemu_design_target_gain_dev: the whole call as host time of the enqueue plus the synchronisation, median of 7 after 3 (the target
store resident); its own launches by HIP events (GPEMU_PROF_DESIGN_TARGET) and its products (GPEMU_PROF_GEMM), each the median of 7
calls after 3; the parts -- the candidate product (the launches of V = Kq [L^-1; gamma; W^T]^T), the panel products (those with
n = the panel width), the k fill, the sweep, the finish -- summed from one call's GPEMU_PROF_DUMP lines.  The sweep's bytes are the
panel read once and the partials written, 8 M (S + S / 64).  gpemu_design_target_set_dev: host time + synchronisation, the same
medians.  Flop model of the gain call: M N^2 for the candidate product (L^-1 is triangular) and 2 M S N for the panels.

The route before: gpemu_predict_cov_dev on 64 candidates and 16 320 targets in ONE call (its limit is 16 384 points), the square
and the sum over the targets on the host; host time + synchronisation of the device call alone, median of 3 after 1, MULTIPLIED
to M candidates -- not run for all of them.  It computes all 16 384^2 covariances to use 64 x 16 320 of them, clamps its
k-vectors and applies the nugget rule, so it is not the same number either where a target lies on a design point.
No time is a pass criterion."""
import argparse
import os
import re
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madaiemulator_amd import abi, synth  # noqa: E402
from sens_profile import wall  # noqa: E402
from sens_post_profile import events  # noqa: E402

KIND, ORDER, SEED = 1, 1, 20261021
M, S, NCAND_OLD = 16384, 16384, 64


def dumped_tags(c, cls, call):
    """the [gpemu prof] lines of one call under class cls -> list of (whole tag, ms)"""
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
    return [(m.group(1), float(m.group(2))) for m in re.finditer(r"\[gpemu prof\] (.*) ms=([0-9.]+)", text)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="append the lines to this file as well")
    ap.add_argument("--cases", default="4096x8,8192x8,4096x16")
    a = ap.parse_args()
    panel = int(os.environ.get("GPEMU_TARGET_PANEL", "2048"))
    lines = [f"# power-exponential, order {ORDER}, lengths 0.6, M = {M} resident candidates, S = {S} resident targets, equal weights, panel "
             f"{panel}; whole calls: host time + synchronisation, median of 7 after 3; launch classes: HIP events, median of 7 after 3"]
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
            rng = np.random.default_rng(13)
            Q = np.ascontiguousarray(lo + (hi - lo) * rng.random((M, d)))
            T = np.ascontiguousarray(lo + (hi - lo) * rng.random((S, d)))
            buf = c.dev_alloc(8 * (M * d + S * d + 3 * M))
            try:
                c.upload(buf, Q)
                t_dev = abi.C.c_void_p(buf.value + 8 * M * d)
                c.upload(t_dev, T)
                g_dev = abi.C.c_void_p(t_dev.value + 8 * S * d)
                n_dev = abi.C.c_void_p(g_dev.value + 8 * M)
                v_dev = abi.C.c_void_p(n_dev.value + 8 * M)

                def setup():
                    c.design_target_set_dev(S, t_dev)

                def gain():
                    c.design_target_gain_dev(M, buf, g_dev, n_dev, v_dev)

                set_ms = wall(c.sync, setup, 3, 7)
                whole = wall(c.sync, gain, 3, 7)
                own = events(c, abi.PROF_DESIGN_TARGET, gain)
                gemm = events(c, abi.PROF_GEMM, gain)
                parts, gparts = dumped_tags(c, abi.PROF_DESIGN_TARGET, gain), dumped_tags(c, abi.PROF_GEMM, gain)
                g = c.download(g_dev, (M,))
            finally:
                c.dev_free(buf)
            by = {t: sum(v for tag, v in parts if tag == t) for t in ("target_kvec", "target_sweep", "target_finish")}
            pan = [v for tag, v in gparts if f" n={min(panel, S)} " in tag + " "]
            cand = [v for tag, v in gparts if f" n={min(panel, S)} " not in tag + " "]
            model = (1.0 * M * N * N + 2.0 * M * S * N)
            sweep_bytes = 8.0 * M * (S + S / 64)
            lines.append(f"N={N} d={d}: gpemu_design_target_gain_dev {whole:9.3f} ms whole call ({model / whole / 1e9:6.2f} TFLOP/s on the flop model "
                         f"M N^2 + 2 M S N); candidate product {sum(cand):9.3f} ms in {len(cand)} launches, panel products {sum(pan):9.3f} ms in "
                         f"{len(pan)} ({2.0 * M * S * N / max(sum(pan), 1e-9) / 1e9:6.2f} TFLOP/s), k fill {by['target_kvec']:7.3f} ms, sweep "
                         f"{by['target_sweep']:8.3f} ms ({100 * by['target_sweep'] / whole:4.1f} % of the call; {sweep_bytes / max(by['target_sweep'], 1e-9) / 1e9:6.3f} TB/s), "
                         f"finish {by['target_finish']:7.3f} ms; classes: own {own:9.3f} ms, products {gemm:9.3f} ms")
            print(lines[-1], flush=True)
            lines.append(f"          gpemu_design_target_set_dev {set_ms:9.3f} ms (flop model S N^2: {1.0 * S * N * N / set_ms / 1e9:6.2f} TFLOP/s); "
                         f"gain: min {g.min():.3e}, max {g.max():.3e}")
            print(lines[-1], flush=True)
            # the route before: the joint covariance of 64 candidates and 16 320 targets, squared and summed on the host
            nx = 16384 - NCAND_OLD
            P = np.ascontiguousarray(np.vstack([Q[:NCAND_OLD], T[:nx]]))
            buf = c.dev_alloc(8 * (16384 * d + 16384 * 16384))
            try:
                c.upload(buf, P)
                cov_dev = abi.C.c_void_p(buf.value + 8 * 16384 * d)
                old_ms = wall(c.sync, lambda: c.predict_cov_dev(16384, buf, None, cov_dev), 1, 3)
                rows = c.download(cov_dev, (NCAND_OLD, 16384))
            finally:
                c.dev_free(buf)
            old = (rows[:, NCAND_OLD:] ** 2).sum(axis=1) / S / rows[np.arange(NCAND_OLD), np.arange(NCAND_OLD)]
            lines.append(f"          route before (gpemu_predict_cov_dev, {NCAND_OLD} candidates + {nx} targets a call, host sum): {old_ms:9.3f} ms a call "
                         f"-> MULTIPLIED to M = {M}: {old_ms * M / NCAND_OLD / 1e3:9.2f} s (not run) against {whole / 1e3:7.3f} s; its gain over "
                         f"{nx} of the {S} targets differs from the entry's by up to {np.max(np.abs(old - g[:NCAND_OLD])) / g[:NCAND_OLD].max():.2e} of the largest")
            print(lines[-1], flush=True)
    finally:
        c.close()
    if a.out:
        with open(a.out, "a") as fo:
            fo.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
