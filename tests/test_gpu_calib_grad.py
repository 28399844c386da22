"""Gradient of the calibration statistics on the device (gpemu_calib_grad, include/gpemu.h), through
abi.Context with the test's own means, variances and gradient arrays: only the new kernel is under test.

Reference: the direct nt x nt form in float64 (calibgradref.direct64), never the r x r form the kernel evaluates; the v = 1e30
family, which float64 cannot factor in the direct form, against the 50-digit repeat alone.  Error measure per (q, j):
|got - ref| / max(1, sum |terms|); bars calibgradref.BARS = 8 x the reference's own largest error against 50 digits, measured
on the CPU (tests/test_calibgradref.py keeps them honest)."""
import ctypes as C
import functools

import numpy as np
import pytest

import calibgradref as G
import calibref as R
from madaiemulator_amd import abi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.calib_release()


@functools.lru_cache(maxsize=None)
def reference(key):
    """the case with its gradient inputs and its float64 reference, computed once and shared (the arrays are read-only)"""
    c = G.make(key)
    g, scale = G.direct64(c)
    for a in (g, scale, c["mean"], c["var"], c["gmean"], c["gvar"]):
        a.setflags(write=False)
    return c, g, scale


def setup(ctx, c):
    rc, info = ctx.calib_setup(c["ybar"], c["A"], c["z"], S=c["S"], sd=c["sd"], rel=c["rel"])
    assert rc == abi.OK and info == 0


def grad(ctx, c, **kw):
    gc, gl = ctx.calib_grad(c["mean"], c["var"], kw.pop("gmean", c["gmean"]), kw.pop("gvar", c["gvar"]), M=c["M"], d=c["d"], **kw)
    return np.stack([gc, gl])


def check(what, got, ref, scale):
    e = G.err(got, ref, scale).max(axis=(1, 2))
    print(what, " ".join(f"{n} {x:.2e}/{b:.1e}" for n, x, b in zip(G.STATS, e, G.BARS)))
    assert np.all(e <= G.BARS), (what, e, G.BARS)


# ------------------------------------------------------------------ 1. every shape against the direct form
@pytest.mark.parametrize("key", [a[0] for a in R.CASES])
def test_shapes_against_direct_form(ctx, key):
    c, ref, scale = reference(key)
    setup(ctx, c)
    got = grad(ctx, c)
    assert got.shape == (2, c["M"], c["d"]) and np.all(np.isfinite(got))      # (finite: the 1e300 padding reached nothing)
    check(key, got, ref, scale)
    assert got.tobytes() == grad(ctx, c).tobytes()                             # a call repeated: the same bits


def test_dev_entry_returns_the_host_entry_bits(ctx):
    c, _, _ = reference("r16_nt65_full_rel")
    setup(ctx, c)
    M, d, nr, ld, ldg = c["M"], c["d"], c["nr"], c["mean"].shape[1], c["ldg"]
    host = grad(ctx, c)
    bufs = [ctx.dev_alloc(8 * n) for n in (nr * ld, nr * ld, nr * ldg, nr * ldg, M * d, M * d)]
    try:
        for p, a in zip(bufs, (c["mean"], c["var"], c["gmean"], c["gvar"])):
            ctx.upload(p, a)
        ctx.calib_grad_dev(M, d, bufs[0], bufs[1], ld, bufs[2], bufs[3], ldg, bufs[4], bufs[5])
        dev = np.stack([ctx.download(bufs[4], (M, d)), ctx.download(bufs[5], (M, d))])
    finally:
        for p in bufs:
            ctx.dev_free(p)
    assert host.tobytes() == dev.tobytes()


def test_either_output_alone_has_the_bits_of_both(ctx):
    for key in ("r8_nt64_full_rel", "r13_nt130_rel"):
        c, _, _ = reference(key)
        setup(ctx, c)
        both = grad(ctx, c)
        gc, none = ctx.calib_grad(c["mean"], c["var"], c["gmean"], c["gvar"], M=c["M"], d=c["d"], want=(True, False))
        assert none is None and gc.tobytes() == both[0].tobytes()
        none, gl = ctx.calib_grad(c["mean"], c["var"], c["gmean"], c["gvar"], M=c["M"], d=c["d"], want=(False, True))
        assert none is None and gl.tobytes() == both[1].tobytes()


@pytest.mark.parametrize("key", ["r8_nt130", "r16_nt65_full_rel", "r5_nt7"])
def test_a_point_alone_has_the_bits_it_has_among_many(ctx, key):
    """a point's bits depend neither on M nor on its position in the call (r8_nt130: M = 1000, four workgroups)"""
    c, _, _ = reference(key)
    setup(ctx, c)
    M, d, nr = c["M"], c["d"], c["nr"]
    full = grad(ctx, c)
    gm, gv = c["gmean"][:, :M * d].reshape(nr, M, d), c["gvar"][:, :M * d].reshape(nr, M, d)
    for q in (0, M // 2 + 1, M - 1):
        one = ctx.calib_grad(c["mean"][:, q:q + 1], c["var"][:, q:q + 1], gm[:, q:q + 1], gv[:, q:q + 1], M=1, d=d)
        assert np.stack(one)[:, 0].tobytes() == full[:, q].tobytes(), (key, q)
    # the last 70 points as a call of their own: other workgroups, other lanes
    tail = ctx.calib_grad(c["mean"][:, M - 70:M], c["var"][:, M - 70:M], gm[:, M - 70:], gv[:, M - 70:], M=min(70, M), d=d) if M >= 70 else None
    if tail is not None:
        assert np.stack(tail).tobytes() == np.ascontiguousarray(full[:, M - 70:]).tobytes()


# ------------------------------------------------------------------ 2. special inputs
def test_zero_variances(ctx):
    c, ref, scale = reference("special_v_zero")
    setup(ctx, c)
    check("v_zero", grad(ctx, c), ref, scale)


def test_negative_variances_give_their_gradients_weight_zero(ctx):
    """the reference clamps the variance and drops its dv_c terms; then the device's answer must not depend on gvar at all"""
    c, ref, scale = reference("special_v_negative")
    setup(ctx, c)
    got = grad(ctx, c)
    check("v_negative", got, ref, scale)
    other = grad(ctx, c, gvar=np.where(c["gvar"] == 1e300, 1e300, 7.0 * c["gvar"] + 1.0))
    assert got.tobytes() == other.tobytes()


def test_huge_variances_against_50_digits(ctx):
    c, _, _ = reference("special_v_huge")
    setup(ctx, c)
    got = grad(ctx, c)
    assert np.all(np.isfinite(got))
    pts = R.mp_points(c)
    ref, scale = G.direct_mp(c, pts)
    check("v_huge", got[:, pts], ref, scale)


def test_nan_in_one_point_only(ctx):
    c, ref, scale = reference("special_one_nan")
    setup(ctx, c)
    got = grad(ctx, c)
    assert np.all(np.isnan(got[:, 17]))                                        # all 2 d values of the point
    others = np.arange(c["M"]) != 17
    assert np.all(np.isfinite(got[:, others]))
    check("one_nan", got, ref, scale)
    # a NaN variance likewise (the clamp of negative variances must not swallow it)
    var = c["var"].copy()
    var[0, 3] = np.nan
    gc, gl = ctx.calib_grad(c["mean"], var, c["gmean"], c["gvar"], M=c["M"], d=c["d"])
    bad = np.isnan(np.stack([gc, gl])).all(axis=(0, 2))
    assert np.array_equal(np.flatnonzero(bad), [3, 17]) and np.all(np.isfinite(gc[4:17])) and np.all(np.isfinite(gl[4:17]))


def test_nan_in_one_gradient_input_stays_in_its_own_entry(ctx):
    for key, comp, q, j in (("r8_nt64_full_rel", 5, 300, 0), ("r13_nt130_rel", 12, 63, 2), ("r4_nt7_full", 0, 64, 7)):
        c, _, _ = reference(key)
        setup(ctx, c)
        d = c["d"]
        j = min(j, d - 1)
        clean = grad(ctx, c)
        gm = c["gmean"].copy()
        gm[comp, q * d + j] = np.nan
        got = grad(ctx, c, gmean=gm)
        assert np.all(np.isnan(got[:, q, j]))
        got[:, q, j] = clean[:, q, j]
        assert got.tobytes() == clean.tobytes(), key
        gv = c["gvar"].copy()
        gv[comp, q * d + j] = np.inf
        got = grad(ctx, c, gvar=gv)
        got[:, q, j] = clean[:, q, j]
        assert got.tobytes() == clean.tobytes(), key


def test_padding_of_both_leading_dimensions_is_never_read(ctx):
    """other values in the padding (and NaN in it) leave every bit alone"""
    c, _, _ = reference("r5_nt7")                          # ld = M + 3, ldg = M d + 5
    setup(ctx, c)
    M, d = c["M"], c["d"]
    clean = grad(ctx, c)
    arrs = {k: c[k].copy() for k in ("mean", "var", "gmean", "gvar")}
    arrs["mean"][:, M:] = np.nan; arrs["var"][:, M:] = np.nan
    arrs["gmean"][:, M * d:] = np.nan; arrs["gvar"][:, M * d:] = np.nan
    gc, gl = ctx.calib_grad(arrs["mean"], arrs["var"], arrs["gmean"], arrs["gvar"], M=M, d=d)
    assert np.stack([gc, gl]).tobytes() == clean.tobytes()


def test_evaluation_keeps_its_bits_around_a_gradient_call(ctx):
    c, _, _ = reference("r9_nt65_rel")
    setup(ctx, c)
    s1, w1 = ctx.calib_eval(c["mean"], c["var"], M=c["M"])
    grad(ctx, c)
    s2, w2 = ctx.calib_eval(c["mean"], c["var"], M=c["M"])
    assert s1.tobytes() == s2.tobytes() and w1.tobytes() == w2.tobytes()
    sref, _ = R.direct64(c)
    assert np.all(R.err(s2, sref).max(axis=1) <= R.BARS)


# ------------------------------------------------------------------ 3. error codes
def test_error_codes(ctx):
    L, h = ctx.L, ctx.h
    c, _, _ = reference("r4_nt7_full")
    M, d, ld, ldg = c["M"], c["d"], c["mean"].shape[1], c["ldg"]
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    gc, gl = np.empty((M, d)), np.empty((M, d))
    call = lambda M=M, d=d, mean=c["mean"], var=c["var"], ld=ld, gm=c["gmean"], gv=c["gvar"], ldg=ldg, gc=gc, gl=gl: \
        L.gpemu_calib_grad(h, M, d, dp(mean), dp(var), ld, dp(gm), dp(gv), ldg, dp(gc), dp(gl))
    ctx.calib_release()
    assert call() == abi.ERR_STATE                               # no set-up
    setup(ctx, c)
    assert call() == abi.OK and call(gc=None) == abi.OK and call(gl=None) == abi.OK
    assert call(gc=None, gl=None) == abi.ERR_ARG
    for kw in (dict(mean=None), dict(var=None), dict(gm=None), dict(gv=None), dict(M=0), dict(d=0), dict(ld=M - 1), dict(ldg=M * d - 1)):
        assert call(**kw) == abi.ERR_ARG, kw
    assert L.gpemu_calib_grad(None, M, d, dp(c["mean"]), dp(c["var"]), ld, dp(c["gmean"]), dp(c["gvar"]), ldg, dp(gc), dp(gl)) == abi.ERR_ARG
    one = C.c_void_p(8)                                          # (never dereferenced: the arguments are refused first)
    dev = lambda **kw: L.gpemu_calib_grad_dev(h, kw.get("M", M), kw.get("d", d), kw.get("mean", one), one, kw.get("ld", ld), one, one,
                                              kw.get("ldg", ldg), kw.get("gc", one), kw.get("gl", one))
    assert dev(M=0) == abi.ERR_ARG and dev(d=0) == abi.ERR_ARG and dev(ld=M - 1) == abi.ERR_ARG and dev(ldg=M * d - 1) == abi.ERR_ARG
    assert dev(mean=None) == abi.ERR_ARG and dev(gc=None, gl=None) == abi.ERR_ARG
    ctx.calib_release()
    assert call() == abi.ERR_STATE
