"""Gain over a weighted set of target points (gpemu_design_target_*, include/gpemu.h) through the public entries,
against tests/designtargetref.py (float64 LAPACK, checked against longdouble before it hands anything out; test_designtargetref.py
pins it against mpmath, the refit identity and the closed form of gpemu_design_gain).

The bars.  Every figure is measured on the CPU over exactly the cases of this file by `python tests/designtargetref.py --measure`.
  whole call   var, var_t at RTOL kappa, target_var at RTOL kappa sum w, num at 2 RTOL kappa^2 sum w, gain at that over var
               (RTOL = 1e-8, the project's parity bar: these depend on the fit itself; c* is compared on the scale kappa).
  sweep alone  u, r and Q r of targets and candidates are the device's own (gpemu_test_design_target_state); product, prior and
               reduction are redone in longdouble.  SWEEP_NP = 1.41e-16 is the largest float64-against-longdouble error of that
               same computation on its scale sum_s w_s T_qs^2, T = |c| + sum |u u| + sum |r Q r| (N = 1, d = 3, Matern 5/2);
               the device gets FACTOR = 8 times that, as in test_gpu_design.py and for the same reason: it sums in another order
               and its exp and sqrt may differ from libm's by an ulp or two per element              -> SWEEP_TOL = 1.13e-15
  refit        REFIT_NP = 1.88e-16 is the largest |gain - (target_var - target_var')| over kappa sum w with N + 1 points
               refitted in numpy (refit_cases(), every kind once)                                     -> REFIT_TOL = 1.5e-15
  quadrature   QUAD_NP = 1.95e-15: Gauss-Legendre targets (32 nodes for d = 1, 16 x 16 for d = 2) against designref.gain on the
               closed form's own scale (the float64 rounding of the two numpy routes; the rule's own error is below it from 12
               nodes per coordinate on, and 1.1e-12 to 2.7e-12 with 8); the two DEVICE entries are compared on that scale
               with the same factor                                                                    -> QUAD_TOL = 1.56e-14
(see DESIGN.md 4.23)."""
import ctypes as C
import os

import numpy as np
import pytest

import designref as D
import designtargetref as T
import sensref as R
from madaiemulator_amd import abi

SWEEP_NP = 1.41e-16
REFIT_NP = 1.88e-16
QUAD_NP = 1.95e-15
FACTOR = 8
SWEEP_TOL = FACTOR * SWEEP_NP
REFIT_TOL = FACTOR * REFIT_NP
QUAD_TOL = FACTOR * QUAD_NP
RTOL = T.RTOL
KEYS = ("gain", "num", "var")

pytestmark = pytest.mark.gpu

_refs = {}


def reference(c, rows=None):
    """the CPU reference of a case, computed once and shared"""
    if c["name"] not in _refs:
        _refs[c["name"]] = T.reference(c, rows)
    return _refs[c["name"]]


def fit(ctx, c, th=None):
    ctx.set_model(c["kind"], c["order"], c["X"], c["y"])
    _, rc = ctx.predict_setup(c["th"] if th is None else th)
    assert rc == abi.OK, rc


def run(ctx, c):
    """targets, then the gain, through the host entries -> dict(gain, num, var, var_t, target_var)"""
    got = ctx.design_target_set(c["Xt"], c["w"])
    got.update(ctx.design_target_gain(c["Xq"]))
    return got


def check_whole(c, got, ref):
    for k in ("gain", "num", "var", "var_t", "target_var"):
        assert np.all(np.isfinite(got[k])), (c["name"], k)
    e = T.errors(got, ref, ref["scale"])
    print(f"{c['name']}: whole call against the reference (in units of its bar RTOL = {RTOL:.0e}) " +
          ", ".join(f"{k} {v / RTOL:.2e}" for k, v in e.items()) + f"; reference's own {max(ref['ref_err'].values()):.1e}")
    assert max(e.values()) < RTOL, (c["name"], e)
    assert np.all(got["gain"] >= 0.0), c["name"]
    assert np.all(got["gain"] <= got["target_var"] + RTOL * (ref["scale"]["gain"] + ref["scale"]["target_var"])), c["name"]


def check_sweep(ctx, c, got, M=None):
    """num against the longdouble sum from the device's own rows; the state of the candidates is read directly behind the call"""
    M = len(c["Xq"]) if M is None else M
    Uq, Rq, _ = ctx.design_target_state(1, M)
    Ut, _, QRt = ctx.design_target_state(0, len(c["Xt"]))
    ref, scale = T.sweep(c["kind"], c["th"], c["Xq"][-M:], c["Xt"], c["w"], Uq, Ut, Rq, QRt)
    e = float(np.max(np.abs(got["num"][-M:] - np.asarray(ref, dtype=np.float64)) / scale))
    print(f"{c['name']}: sweep against longdouble on the device's rows {e:.2e} (bar {SWEEP_TOL:.2e})")
    assert e < SWEEP_TOL, (c["name"], e)


def same(a, b, keys=KEYS):
    return all(np.array_equal(a[k], b[k]) for k in keys)


@pytest.fixture(scope="module")
def second_ctx():
    ctx = abi.Context(0)
    yield ctx
    ctx.close()


def context_with_panel(width):
    old = os.environ.get("GPEMU_TARGET_PANEL")
    os.environ["GPEMU_TARGET_PANEL"] = str(width)
    try:
        return abi.Context(0)
    finally:
        if old is None:
            del os.environ["GPEMU_TARGET_PANEL"]
        else:
            os.environ["GPEMU_TARGET_PANEL"] = old


# ---------------------------------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize("N", T.NS)
def test_shapes(gpu_ctx, N):
    """one design tile, a ragged second one, three; one target or candidate, a ragged tile, four tiles; every kind; d past the
    register chunk of the fill; targets and candidates on design points and on each other, a weight of 0"""
    for c in T.all_cases():
        if c["N"] != N:
            continue
        fit(gpu_ctx, c)
        got = run(gpu_ctx, c)
        check_sweep(gpu_ctx, c, got)
        check_whole(c, got, reference(c))
        if c["kind"] == abi.POWEREXP:            # var is the closed-form entry's var
            lo, hi = T.box(c["X"])
            v = gpu_ctx.design_gain(lo, hi, c["Xq"])["var"]
            assert np.all(np.abs(got["var"] - v) <= RTOL * T.kappa(c["kind"], c["th"])), c["name"]


def test_targets_across_the_block_edge(gpu_ctx):
    """16 385 targets: two blocks of the store, nine panels of the default width"""
    c = T.big_cases()[0]
    fit(gpu_ctx, c)
    got = run(gpu_ctx, c)
    check_sweep(gpu_ctx, c, got)
    check_whole(c, got, reference(c, (np.arange(5), np.r_[0:100, T.BIG - 100:T.BIG])))
    tail = gpu_ctx.design_target_set(c["Xt"][16384:], c["w"][16384:])
    assert tail["var_t"][0] == got["var_t"][16384]                                # the target alone in its block: the same bits


def test_candidates_across_the_block_edge(gpu_ctx):
    """16 385 candidates: two blocks; the last candidate, alone in the second, has the bits of that point evaluated alone"""
    c = T.big_cases()[1]
    fit(gpu_ctx, c)
    got = run(gpu_ctx, c)
    check_sweep(gpu_ctx, c, got, M=1)
    check_whole(c, got, reference(c, (np.r_[0:100, T.BIG - 100:T.BIG], np.arange(7))))
    alone = gpu_ctx.design_target_gain(c["Xq"][16384:])
    assert all(np.array_equal(got[k][16384:], alone[k]) for k in KEYS)
    first = gpu_ctx.design_target_gain(c["Xq"][:64])
    assert all(np.array_equal(got[k][:64], first[k]) for k in KEYS)


@pytest.mark.parametrize("i", range(len(T.REFIT_CASES)))
def test_refit_on_the_device(gpu_ctx, second_ctx, i):
    """gain against target_var of this context minus target_var of a second context on the design with the candidate appended"""
    c = T.refit_cases()[i]
    fit(gpu_ctx, c)
    got = run(gpu_ctx, c)
    sc = T.kappa(c["kind"], c["th"]) * c["w"].sum()
    for q, x in enumerate(c["Xq"]):
        c2 = dict(c, X=np.vstack([c["X"], x[None, :]]), y=np.append(c["y"], 0.5))
        fit(second_ctx, c2)
        tv2 = second_ctx.design_target_set(c["Xt"], c["w"])["target_var"]
        gap = abs(got["gain"][q] - (got["target_var"] - tv2)) / sc
        print(f"{c['name']} candidate {q}: gain {got['gain'][q]:.6e}, refit {got['target_var'] - tv2:.6e}, gap {gap:.2e} (bar {REFIT_TOL:.1e})")
        assert gap < REFIT_TOL, (c["name"], q, gap)


@pytest.mark.parametrize("i", range(len(T.QUAD_CASES)))
def test_quadrature_link(gpu_ctx, i):
    """Gauss-Legendre targets of the box: the targeted gain is gpemu_design_gain's, on the closed form's scale"""
    c, lo, hi = T.quad_cases()[i]
    fit(gpu_ctx, c)
    got = run(gpu_ctx, c)
    cf = gpu_ctx.design_gain(lo, hi, c["Xq"])
    a, b = gpu_ctx.design_state(len(c["Xq"]))
    m = dict(A=float(np.exp(c["th"][0])), s=np.exp(-2.0 * c["th"][2:]))
    _, scale, _ = D.gain(R.NP, c["X"], m, lo, hi, None, c["Xq"], a, b, cf["var"])
    e = max(float(np.max(np.abs(got[k] - cf[k]) / scale[k])) for k in ("num", "gain"))
    print(f"{c['name']}: targeted against closed form {e:.2e} (bar {QUAD_TOL:.2e})")
    assert e < QUAD_TOL, (c["name"], e)
    assert np.array_equal(got["var"], cf["var"]) or np.all(np.abs(got["var"] - cf["var"]) <= RTOL * T.kappa(c["kind"], c["th"]))


# ---------------------------------------------------------------------------------------------------- 2. kernel edges
def test_panel_widths_give_the_same_bits(gpu_ctx):
    """S = 200 on panels of 64 and of 128 columns (four and two panels, the last one ragged) against the default width"""
    c = T.case(130, 3, 1, abi.MATERN32, 65, 200, 5)
    fit(gpu_ctx, c)
    first = run(gpu_ctx, c)
    for width in (64, 128):
        ctx = context_with_panel(width)
        try:
            fit(ctx, c)
            assert same(first, run(ctx, c), KEYS + ("var_t", "target_var")), width
        finally:
            ctx.close()


def test_a_smaller_set_after_a_larger_one(gpu_ctx, second_ctx):
    """S = 65 right after S = 200 on one context: nothing of the larger set's panel, partials or store enters"""
    big, c = T.case(130, 3, 1, abi.POWEREXP, 65, 200, 5), T.case(130, 3, 1, abi.POWEREXP, 65, 65, 6)
    fit(gpu_ctx, c)
    run(gpu_ctx, dict(big, th=c["th"]))
    got = run(gpu_ctx, c)
    fit(second_ctx, c)
    assert same(got, run(second_ctx, c), KEYS + ("var_t", "target_var"))
    check_whole(c, got, reference(c))


def test_a_whole_tile_of_zero_weights(gpu_ctx):
    c = T.case(65, 3, 1, abi.MATERN52, 65, 200, 7)
    c["w"][64:128] = 0.0
    c["name"] += "-zero-tile"
    fit(gpu_ctx, c)
    got = run(gpu_ctx, c)
    check_sweep(gpu_ctx, c, got)
    check_whole(c, got, reference(c))
    keep = np.r_[0:64, 128:200]
    part = run(gpu_ctx, dict(c, Xt=c["Xt"][keep], w=c["w"][keep]))
    assert np.allclose(part["num"], got["num"], rtol=1e-13, atol=0)               # (the tiles shift: another order, the same sum)


# ---------------------------------------------------------------------------------------------------- 3. bits
def test_same_bits(gpu_ctx):
    """two calls; the host and the _dev entries; num and var left out; after a release"""
    c = T.case(130, 8, 1, abi.MATERN52, 65, 200, 8)
    fit(gpu_ctx, c)
    first = run(gpu_ctx, c)
    assert same(first, run(gpu_ctx, c), KEYS + ("var_t", "target_var"))
    M, S = len(c["Xq"]), len(c["Xt"])
    xq_dev, xt_dev = gpu_ctx.dev_alloc(c["Xq"].nbytes), gpu_ctx.dev_alloc(c["Xt"].nbytes)
    out_dev, t_dev = gpu_ctx.dev_alloc(3 * M * 8), gpu_ctx.dev_alloc((S + 1) * 8)
    try:
        gpu_ctx.upload(xq_dev, c["Xq"])
        gpu_ctx.upload(xt_dev, c["Xt"])
        gpu_ctx.design_target_release()
        gpu_ctx.design_target_set_dev(S, xt_dev, c["w"], t_dev, C.c_void_p(t_dev.value + 8))
        t = gpu_ctx.download(t_dev, (S + 1,))
        assert t[0] == first["target_var"] and np.array_equal(t[1:], first["var_t"])
        gpu_ctx.design_target_gain_dev(M, xq_dev, out_dev, C.c_void_p(out_dev.value + M * 8), C.c_void_p(out_dev.value + 2 * M * 8))
        o3 = gpu_ctx.download(out_dev, (3, M))
        assert same(first, dict(gain=o3[0], num=o3[1], var=o3[2]))
        gpu_ctx.design_target_set_dev(S, xt_dev, c["w"])                          # the results may be left out
        gpu_ctx.design_target_gain_dev(M, xq_dev, out_dev)
        assert np.array_equal(gpu_ctx.download(out_dev, (M,)), first["gain"])
    finally:
        for p in (xq_dev, xt_dev, out_dev, t_dev):
            gpu_ctx.dev_free(p)
    equal = gpu_ctx.design_target_set(c["Xt"][:7])                                # weight NULL: 1 / S each
    given = gpu_ctx.design_target_set(c["Xt"][:7], np.full(7, 1.0 / 7))
    assert equal["target_var"] == given["target_var"]


def test_release_then_call_again(gpu_ctx):
    c = T.case(65, 3, 2, abi.POWEREXP, 64, 63, 9)
    fit(gpu_ctx, c)
    first = run(gpu_ctx, c)
    gpu_ctx.design_target_release()
    for call in (lambda: gpu_ctx.design_target_gain(c["Xq"]), lambda: gpu_ctx.design_target_state(0, 63)):
        with pytest.raises(abi.GpemuError) as ei:
            call()
        assert ei.value.code == abi.ERR_STATE
    assert same(first, run(gpu_ctx, c), KEYS + ("var_t", "target_var"))


def test_a_new_setup_rebuilds_the_store(gpu_ctx):
    """other thetas on the same design: the next gain call rebuilds u, r and Q r from the kept coordinates; and back"""
    c = T.case(65, 3, 1, abi.POWEREXP, 8, 65, 10)
    fit(gpu_ctx, c)
    first = run(gpu_ctx, c)
    th2 = c["th"].copy()
    th2[2:] += 0.2
    _, rc = gpu_ctx.predict_setup(th2)
    assert rc == abi.OK
    other = gpu_ctx.design_target_gain(c["Xq"])                                   # no new set call
    c2 = dict(c, th=th2, name=c["name"] + "-th2")
    ref2 = reference(c2)
    e = T.errors(other, ref2, ref2["scale"], KEYS)
    assert max(e.values()) < RTOL, e
    check_sweep(gpu_ctx, c2, other)
    _, rc = gpu_ctx.predict_setup(c["th"])
    assert rc == abi.OK
    assert same(first, gpu_ctx.design_target_gain(c["Xq"]))
    gpu_ctx.set_model(c["kind"], c["order"], c["X"], c["y"])                      # a new model frees the targets
    _, rc = gpu_ctx.predict_setup(c["th"])
    with pytest.raises(abi.GpemuError) as ei:
        gpu_ctx.design_target_gain(c["Xq"])
    assert ei.value.code == abi.ERR_STATE


def test_setup_by_batch_same_bits(gpu_ctx):
    """contexts set up by gpemu_predict_setup_batch, component 0 and a later one, against a context set up alone"""
    c = T.case(130, 3, 1, abi.POWEREXP, 65, 65, 11)
    ys = [c["y"], 0.5 * c["y"] + c["X"][:, 0], c["y"] * c["y"]]
    ctxs = [abi.Context(0) for _ in ys]
    try:
        for cx, yc in zip(ctxs, ys):
            cx.set_model(c["kind"], c["order"], c["X"], yc)
        _, _, status, rc = abi.predict_setup_batch(ctxs, np.tile(c["th"], (len(ys), 1)))
        assert rc == abi.OK and np.all(status == abi.OK)
        fit(gpu_ctx, c)
        alone = run(gpu_ctx, c)                                                   # (the gain does not depend on the training values)
        for cx in (ctxs[0], ctxs[2]):
            assert same(alone, run(cx, c), KEYS + ("var_t", "target_var"))
    finally:
        for cx in ctxs:
            cx.close()


# ---------------------------------------------------------------------------------------------------- 4. neighbours
def test_a_pending_batch_stays_collectable(gpu_ctx):
    c = T.case(130, 3, 1, abi.MATERN32, 65, 65, 12)
    fit(gpu_ctx, c)
    mean, var = gpu_ctx.predict(c["Xq"])
    gpu_ctx.predict_enqueue(c["Xq"])
    got = run(gpu_ctx, c)
    m2, v2 = gpu_ctx.predict_collect()
    assert np.array_equal(mean, m2) and np.array_equal(var, v2)
    assert same(got, run(gpu_ctx, c))


def test_neighbours_keep_their_bits(gpu_ctx):
    """gpemu_design_gain, gpemu_predict_cov and gpemu_predict_var_grad return the bits they returned before the calls"""
    c = T.case(130, 3, 2, abi.POWEREXP, 65, 65, 13)
    fit(gpu_ctx, c)
    lo, hi = T.box(c["X"])
    dg, vg, pc = gpu_ctx.design_gain(lo, hi, c["Xq"]), gpu_ctx.predict_var_grad(c["Xq"]), gpu_ctx.predict_cov(c["Xq"])
    run(gpu_ctx, c)
    dg2, vg2, pc2 = gpu_ctx.design_gain(lo, hi, c["Xq"]), gpu_ctx.predict_var_grad(c["Xq"]), gpu_ctx.predict_cov(c["Xq"])
    assert same(dg, dg2)
    assert all(np.array_equal(p, q) for p, q in zip(vg, vg2))
    assert all(np.array_equal(p, q) for p, q in zip(pc, pc2))


# ---------------------------------------------------------------------------------------------------- 5. errors
def test_errors(gpu_ctx, second_ctx):
    c = T.case(65, 3, 1, abi.POWEREXP, 5, 9, 14)
    L, p = gpu_ctx.L, abi._p
    Xt, Xq, w = (np.ascontiguousarray(v, dtype=np.float64) for v in (c["Xt"], c["Xq"], c["w"]))
    S, M = len(Xt), len(Xq)
    out = np.empty(M)
    fit(gpu_ctx, c)
    gpu_ctx.design_target_release()
    second_ctx.set_model(c["kind"], c["order"], c["X"], c["y"])                   # a model, no set-up
    for h in (gpu_ctx.h, second_ctx.h):                                           # whatever the state
        assert L.gpemu_design_target_set(h, S, None, p(w), None, None) == abi.ERR_ARG
        assert L.gpemu_design_target_set(h, 0, p(Xt), p(w), None, None) == abi.ERR_ARG
        assert L.gpemu_design_target_set(h, 65537, p(Xt), None, None, None) == abi.ERR_ARG
        assert L.gpemu_design_target_set_dev(h, S, None, p(w), None, None) == abi.ERR_ARG
        for bad in (-1.0, np.nan, np.inf):
            wb = w.copy()
            wb[3] = bad
            assert L.gpemu_design_target_set(h, S, p(Xt), p(wb), None, None) == abi.ERR_ARG
            assert L.gpemu_design_target_set_dev(h, S, C.c_void_p(8), p(wb), None, None) == abi.ERR_ARG
        assert L.gpemu_design_target_set(h, S, p(Xt), p(np.zeros(S)), None, None) == abi.ERR_ARG
        assert L.gpemu_design_target_gain(h, M, None, p(out), None, None) == abi.ERR_ARG
        assert L.gpemu_design_target_gain(h, M, p(Xq), None, None, None) == abi.ERR_ARG
        assert L.gpemu_design_target_gain(h, 0, p(Xq), p(out), None, None) == abi.ERR_ARG
        assert L.gpemu_design_target_gain_dev(h, M, None, None, None, None) == abi.ERR_ARG
    assert L.gpemu_design_target_set(None, S, p(Xt), p(w), None, None) == abi.ERR_ARG
    assert L.gpemu_design_target_release(None) == abi.ERR_ARG
    for bad in (np.nan, -np.inf):
        xb = Xt.copy()
        xb[2, 1] = bad
        assert L.gpemu_design_target_set(gpu_ctx.h, S, p(xb), p(w), None, None) == abi.ERR_ARG
    # no prediction set-up; a gain call without targets
    assert L.gpemu_design_target_set(second_ctx.h, S, p(Xt), p(w), None, None) == abi.ERR_STATE
    assert L.gpemu_design_target_gain(second_ctx.h, M, p(Xq), p(out), None, None) == abi.ERR_STATE
    assert L.gpemu_design_target_gain(gpu_ctx.h, M, p(Xq), p(out), None, None) == abi.ERR_STATE
    assert L.gpemu_design_target_gain_dev(gpu_ctx.h, M, C.c_void_p(8), C.c_void_p(8), None, None) == abi.ERR_STATE
    # and the entries work after all that; a non-finite candidate, the state of another size
    got = run(gpu_ctx, c)
    assert np.all(np.isfinite(got["gain"]))
    xb = Xq.copy()
    xb[0, 0] = np.nan
    assert L.gpemu_design_target_gain(gpu_ctx.h, M, p(xb), p(out), None, None) == abi.ERR_ARG
    u, r = np.empty((S + 1, 65)), np.empty((S + 1, 4))
    assert L.gpemu_test_design_target_state(gpu_ctx.h, 0, S + 1, p(u), p(r), p(r.copy())) == abi.ERR_STATE
    assert L.gpemu_test_design_target_state(gpu_ctx.h, 2, S, p(u), p(r), p(r.copy())) == abi.ERR_ARG
    assert L.gpemu_test_design_target_state(gpu_ctx.h, 0, S, None, p(r), p(r.copy())) == abi.ERR_ARG
