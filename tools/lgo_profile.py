#!/usr/bin/env python3
"""K-fold / leave-group-out validation from the resident factor (gpemu_lgo_dev) against the refit route on one GPU at
BASELINE configs[2] (N=8192, d=8, Matern 5/2, order 1).

    timeout -k 10 1100 python tools/lgo_profile.py [--out FILE] [--cases 5,10,64,g4]

Cases: K in {5, 10, 64} interleaved folds (point i in fold i mod K) and "g4" = 2048 groups of 4 consecutive points.

gpemu_lgo_dev: host-to-host medians of 25 calls after 5 warm-up calls, each call timed on the host from its first enqueue to
the end of a stream synchronisation; then its launches by profiling class, HIP events on the context's stream around every
launch of the class (the whole factorisations under GPEMU_PROF_POTRF): medians of 5 calls; then the gather launches alone
(GPEMU_PROF_DUMP lines of one call) with the bytes they move -- 8 nbc bp Np written plus the lower tiles of L^-1 read -- as
bytes/s, to be read beside loo_colsq_kernel's 5.6 TB/s.

The refit route is the only one the library offered before: per fold gpemu_set_model on the other points, gpemu_predict_setup
at the same thetas and gpemu_predict_joint_factor on the fold with its training values as the one observation row, on a second
context, timed the same way (host to host, synchronised).  One call of it costs K factorisations, so the number of timed calls
is cut to what a measurement run can afford and SAID on the line: 25 after 5 where a call is under a second, otherwise 3 after
1; for the 2048 groups of 4 the first 64 groups are refitted (2 calls after 1) and the time is scaled by 32 -- every refit there
has the same size, N - 4.

Flop model of the closed form: sum over the chunks of nbc (bp^2 Np + bp^3) -- the Gram product and the factorisation with its
inverse rows.  No time is a pass criterion: the lines give the measured times, the rates they imply and the ratio of the two
routes."""
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

KIND, ORDER, N, D, SEED = 3, 1, 8192, 8, 20261003 + 2
WARM, REPS = 5, 25
BUDGET = 2147483648.0


def wall(sync, call, warm, reps, spread=False):
    for _ in range(warm):
        call()
    sync()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        sync()
        ms.append((time.perf_counter() - t) * 1e3)
    return (statistics.median(ms), min(ms), max(ms)) if spread else statistics.median(ms)


def prof(c, cls, call, reps=5):
    ms, n, fl, by = [], 0, 0.0, 0.0
    for _ in range(reps):
        c.prof_begin(cls)
        call()
        p = c.prof_end()
        ms.append(p["ms"])
        n, fl, by = p["n"], p["flops"], p["bytes"]
    return statistics.median(ms), n, fl, by


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


def chunks(ngroups, bp, Np):
    per = 8.0 * bp * (Np + 2.0 * bp + 64)
    nbc = max(1, min(ngroups, 64, int(BUDGET / per)))
    return [min(nbc, ngroups - g0) for g0 in range(0, ngroups, nbc)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="append the lines to this file as well")
    ap.add_argument("--cases", default="5,10,64,g4")
    a = ap.parse_args()
    X, y = synth.design(N, D, SEED)
    th = synth.default_thetas(KIND, D)
    Np = (N + 63) // 64 * 64
    c = abi.Context(0)
    c.set_model(KIND, ORDER, X, y)
    _, rc = c.predict_setup(th)
    assert rc == abi.OK
    r = abi.Context(0)                       # the refit route's context
    lines = [f"# N={N} d={D} Matern 5/2 order {ORDER}; gpemu_lgo_dev: medians of {REPS} after {WARM}, host time of call + synchronisation; "
             f"classes: HIP events around the launches, medians of 5; refit route: see each line for its number of calls"]
    try:
        for case in a.cases.split(","):
            if case == "g4":
                group, what = (np.arange(N) // 4).astype(np.int32), "2048 groups of 4"
            else:
                group, what = (np.arange(N) % int(case)).astype(np.int32), f"{int(case)} interleaved folds"
            ng = int(group.max()) + 1
            sizes = np.bincount(group)
            bp = (int(sizes.max()) + 63) // 64 * 64
            ch = chunks(ng, bp, Np)
            flops = sum(nbc * (float(bp) ** 2 * Np + float(bp) ** 3) for nbc in ch)
            buf = c.dev_alloc(8 * (3 * N + 3 * ng) + 4 * ng)
            try:
                b0 = buf.value
                args = (group, ng, b0, b0 + 8 * N, b0 + 16 * N, b0 + 24 * N, b0 + 8 * (3 * N + 3 * ng))

                def lgo():
                    c.lgo_dev(*args)

                ms = wall(c.sync, lgo, WARM, REPS)
                info = c.download(abi.C.c_void_p(b0 + 8 * (3 * N + 3 * ng)), (ng,), dtype=np.int32)
                stat = c.download(abi.C.c_void_p(b0 + 24 * N), (3, ng))
                assert not info.any() and np.all(np.isfinite(stat))
                lines.append(f"{what}: bp {bp}, chunks {len(ch)} x <= {max(ch)} groups   gpemu_lgo_dev {ms:10.3f} ms / call   flop model "
                             f"{flops:.4g} -> {flops / ms * 1e-9:6.2f} TFLOP/s   sum maha / N {stat[0].sum() / N:.4f}  sum logpdf {stat[2].sum():.8g}")
                for name, k in (("GPEMU_PROF_LGO", abi.PROF_LGO), ("GPEMU_PROF_GEMM", abi.PROF_GEMM), ("GPEMU_PROF_POTRF", abi.PROF_POTRF),
                                ("GPEMU_PROF_LEAF", abi.PROF_LEAF)):
                    pm, n, fl, by = prof(c, k, lgo)
                    rate = f"  {fl / pm * 1e-9:7.2f} TFLOP/s" if fl > 0 and pm > 0 else ""
                    lines.append(f"          of it, {name:16s} {pm:10.3f} ms / call  {n} launches{rate}")
                g_ms = sum(t for tag, t in dumped(c, abi.PROF_LGO, lgo) if tag == "lgo_gather")
                g_bytes, g0 = 0.0, 0
                for nbc in ch:                 # per chunk: Z written; of L^-1 the tiles at or below the diagonal of the tile columns that hold a member
                    cts = np.unique(np.flatnonzero((group >= g0) & (group < g0 + nbc)) // 64)
                    g_bytes += 8.0 * nbc * bp * Np + 8.0 * 64 * 64 * float(np.sum((N + 63) // 64 - cts))
                    g0 += nbc
                lines.append(f"          lgo_gather alone {g_ms:10.3f} ms over {len(ch)} launches, {g_bytes:.4g} bytes (Z written + the lower tiles of "
                             f"L^-1 read) -> {g_bytes / g_ms * 1e-9:6.2f} TB/s   (loo_colsq_kernel: 5.6 TB/s)")
            finally:
                c.dev_free(buf)
            # the refit route on the same folds
            todo, scale = (list(range(64)), ng / 64.0) if case == "g4" else (list(range(ng)), 1.0)
            members = [np.flatnonzero(group == g) for g in todo]
            keeps = [np.setdiff1d(np.arange(N), B) for B in members]
            out = {}

            def refit():
                tot = 0.0
                for B, kp in zip(members, keeps):
                    r.set_model(KIND, ORDER, X[kp], y[kp])
                    _, rc2 = r.predict_setup(th)
                    assert rc2 == abi.OK
                    res = r.predict_joint_factor(X[B], None, y[B])
                    assert res["status"] == abi.OK
                    tot += float(res["logpdf"][0])
                out["logpdf"] = tot

            t = time.perf_counter()
            refit()
            first = (time.perf_counter() - t) * 1e3
            warm, reps = (WARM - 1, REPS) if first < 1000.0 and case != "g4" else ((0, 2) if case == "g4" else (0, 3))
            rms, rlo, rhi = (v * scale for v in wall(r.sync, refit, warm, reps, spread=True))
            same = "" if case == "g4" else f"  sum logpdf {out['logpdf']:.8g}"
            lines.append(f"          refit route (set_model + predict_setup + predict_joint_factor per fold) {rms:10.3f} ms / call"
                         f"{' (64 of the groups, scaled by 32)' if case == 'g4' else ''}, median of {reps} after {warm + 1} "
                         f"(fastest {rlo:.3f}, slowest {rhi:.3f})   refit / closed form {rms / ms:8.1f} (fastest refit call: {rlo / ms:.1f}){same}")
            print(lines[-1], flush=True)
    finally:
        c.close()
        r.close()
    out_f = open(a.out, "a") if a.out else None
    for line in lines:
        print(line, flush=True)
        if out_f:
            out_f.write(line + "\n")
    if out_f:
        out_f.write("\n")
        out_f.close()


if __name__ == "__main__":
    main()
