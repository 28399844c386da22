#!/usr/bin/env python3
"""The ensemble sampler's step against the sweeps it is made of, on one GPU: N = 8192, d = 8, power-exponential, order 1, r = 8
components on one design, nt = 16 outputs, W = 4096 and 16 384 walkers, 200 steps.

    timeout -k 10 900 python tools/sample_profile.py [--out profiles/sample.txt] [--steps 200] [--walkers 4096,16384]

Measured, all by a host clock around work that ends in a synchronise of every stream involved, after a warm-up of the same
shape (which also makes every allocation of the state):
  * gpemu_calib_sample, NULL traces: time per step = the call's wall time over its steps (the two start-up half-batches and the
    final copies are inside: 1 / steps of a step's work and three small copies)
  * the sum of its own sweeps issued directly, in the same run: per step 2 r gpemu_predict_batch_dev on W / 2 resident points,
    every component on its own stream, and 2 gpemu_calib_eval_dev, a synchronise at the end of all steps only
  * the new kernels alone: per step 2 gpemu_sample_propose_dev and 2 gpemu_sample_accept_dev on one stream
  * the same chain driven from the host, what a caller could do before the run existed: per half-step the proposal and the
    accept step in numpy (tests/sampleref.py), the r components' gpemu_predict_batch and gpemu_calib_eval through their
    host-buffer entries -- points up, 2 r + 5 numbers per point down: the route of emulate_points_multi_implausibility without
    that layer's C back-projection, which this tool cannot reach; HOST_STEPS steps, per step
A step's share beyond its sweeps and its kernels is what the event ordering and the enqueue cost.  No ratio is asserted."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from madaiemulator_amd import abi, synth  # noqa: E402
import sampleref  # noqa: E402

KIND, ORDER, N, D, R, NT, SEED = 1, 1, 8192, 8, 8, 16, 20261020
HOST_STEPS = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="append the lines to this file as well")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--walkers", default="4096,16384")
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    rng = np.random.default_rng(11)
    X, y = synth.design(N, D, SEED)
    comps = [abi.Context(0) for _ in range(R)]
    obs = abi.Context(0)
    th = synth.default_thetas(KIND, D)
    for k, c in enumerate(comps):
        c.set_model(KIND, ORDER, X, y * (1.0 + 0.1 * k) + 0.05 * rng.standard_normal(N))
    _, _, status, rc = abi.predict_setup_batch(comps, np.tile(th, (R, 1)))
    assert rc == abi.OK, status
    Q, _ = np.linalg.qr(rng.standard_normal((NT, R)))
    A = np.ascontiguousarray(Q * (2.0 * 10.0 ** (-1.5 * np.arange(R) / R)))
    ybar, sd = rng.uniform(0.5, 3.0, NT), rng.uniform(0.3, 0.6, NT)
    m0 = np.array([c.predict(np.full((1, D), 0.5))[0][0] for c in comps])
    z = ybar + A @ m0 + 0.3 * sd * rng.standard_normal(NT)
    obs.calib_setup(ybar, A, z, sd=sd)
    lo, hi, kind = np.zeros(D), np.ones(D), np.zeros(D, dtype=int)
    obs.sample_set_prior(lo, hi)
    say(f"# N={N} d={D} pow-exp order {ORDER}, r={R} components, nt={NT}; {a.steps} steps; host clock, synchronised, after a warm-up")

    def sync_all():
        for c in comps:
            c.sync()
        obs.sync()

    for W in [int(w) for w in a.walkers.split(",")]:
        h = W // 2
        x0 = sampleref.prior_draws(7, W, np.full(D, 0.3), np.full(D, 0.7), kind)
        abi.calib_sample(comps, obs, x0, 3, seed=1, trace=False)                       # warm-up: allocations, code load
        t0 = time.perf_counter()
        r = abi.calib_sample(comps, obs, x0, a.steps, seed=1, trace=False)
        step_ms = (time.perf_counter() - t0) * 1e3 / a.steps
        acc = r["naccept"].sum() / (a.steps * W)

        bufs = [obs.dev_alloc(8 * n) for n in (W * D, h * D, W, R * h, R * h, 5 * h, W)] + [obs.dev_alloc(4 * h), obs.dev_alloc(4 * W)]
        dx, dy, daux, dm, dv, ds, dlp, dw, dn = bufs
        off = lambda p, n: p.__class__(p.value + 8 * n)
        try:
            obs.upload(dx, r["x_end"]); obs.upload(dlp, r["lp_end"]); obs.upload(dn, np.zeros(W, dtype=np.int32))
            obs.sample_propose_dev(W, D, 0, 0, 1, 2.0, dx, dy, daux)
            obs.sync()

            def sweeps(steps):
                for _ in range(2 * steps):
                    for k, c in enumerate(comps):
                        c.predict_dev(h, dy, off(dm, k * h), off(dv, k * h))
                    obs.calib_eval_dev(h, dm, dv, h, ds, dw)
                sync_all()

            def kernels(steps):
                for g in range(steps):
                    for half in (0, 1):
                        obs.sample_propose_dev(W, D, half, g, 1, 2.0, dx, dy, daux)
                        obs.sample_accept_dev(W, D, half, g, 1, dy, daux, off(ds, h), dx, dlp, dn)
                obs.sync()

            sweeps(3)
            t0 = time.perf_counter(); sweeps(a.steps); sweeps_ms = (time.perf_counter() - t0) * 1e3 / a.steps
            kernels(3)
            t0 = time.perf_counter(); kernels(a.steps); kern_ms = (time.perf_counter() - t0) * 1e3 / a.steps
        finally:
            sync_all()
            for p in bufs:
                obs.dev_free(p)

        def host_loglik(pts):
            mv = [c.predict(pts) for c in comps]
            return obs.calib_eval(np.array([m for m, _ in mv]), np.array([v for _, v in mv]), M=pts.shape[0])[0][1]

        sampleref.run(host_loglik, x0, 1, lo, hi, kind, seed=1)                        # warm-up of the host-buffer entries
        t0 = time.perf_counter()
        sampleref.run(host_loglik, x0, HOST_STEPS, lo, hi, kind, seed=1)
        host_ms = (time.perf_counter() - t0) * 1e3 / (HOST_STEPS + 1)                  # (+ 1: the start-up evaluation is a step's work)

        rest = step_ms - sweeps_ms - kern_ms
        say(f"W={W:6d}  gpemu_calib_sample                       {step_ms:9.3f} ms per step   (accepted fraction {acc:.3f})")
        say(f"W={W:6d}  its sweeps issued directly                {sweeps_ms:9.3f} ms per step   = {sweeps_ms / step_ms * 100:5.1f} % of a step")
        say(f"W={W:6d}  propose + accept kernels alone            {kern_ms:9.3f} ms per step   = {kern_ms / step_ms * 100:5.1f} % of a step")
        say(f"W={W:6d}  the rest (event ordering, enqueue)        {rest:9.3f} ms per step   = {rest / step_ms * 100:5.1f} % of a step")
        say(f"W={W:6d}  the chain driven from the host, numpy     {host_ms:9.3f} ms per step   = {host_ms / step_ms:5.2f} x  ({HOST_STEPS} steps)")
    for c in comps:
        c.close()
    obs.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
