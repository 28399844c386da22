"""Hold-out validation and joint draws at query points (gpemu_predict_joint_factor[_dev], gpemu_predict_joint_draw[_dev],
gpemu_predict_joint_release; include/gpemu.h) against tests/jointref.py: S from predcovref plus noise, its
factor, the whitened errors, Mahalanobis distances, log determinant, log density and draws from LAPACK -- never the code
under test.

Bars, RTOL = vargradref.RTOL = 1e-8, the prediction family's:
  mean, var   as in tests/test_gpu_predict_cov.py: |mean - ref| <= RTOL max(1, |ref|), |var - ref| <= RTOL kappa
  werr        max |werr - ref| <= RTOL max(1, max |ref|)
  maha        |maha - ref| <= RTOL max(1, ref)
  logdet      |logdet - ref| <= RTOL M
  logpdf      = -1/2 (maha + logdet + M log 2 pi): half the sum of the two bars above
  out         |out - ref| <= RTOL sqrt(max S_pp) max(1, max |z|)
Every comparison first has jointref.reference assert kappa_2(S) <= 1e3, that the float64 reference agrees with its
extended-precision repeat to 1e-10 in the same measures, and that its logpdf is scipy.stats.multivariate_normal's.

Inputs: the models of tests/test_gpu_var_grad.py with FRESH queries drawn uniformly in the design's bounding box (the query
sets of the other prediction tests hold points on training points and copies of each other: their Sigma is singular).

Sizes: M = 1, 2, 63, 64, 65 (tile and pad edges), 128, 129 (the 128-column pair and one block more), 200, 321 (uneven
recursion), 577 (M' = 640 > 512: the right-looking outer panels of a single matrix), every one a call of its own against the
leading part of ONE reference; nobs = 0, 1, 3, 64; ndraw = 1, 17, 64, 65 and 1025 (a second block of draws); N from the ragged
set; d = 1, 8, 17; every covariance function at orders 0 and 2; the Matern log mode.

Every test prints its largest errors (pytest -s).  Measured on an MI355X, largest per group, in the bars' units (bars 1e-8):
every size (M = 1 .. 577) werr 2.1e-13, maha 2.4e-13 (M = 1), logdet 6.0e-14 per point, draws 1.1e-13, mean 6.9e-14, var 2.5e-15,
logpdf 1.8e-13; ragged N werr 4.9e-13, draws 4.8e-13; nobs x ndraw (64 rows, 1025 draws) werr 1.1e-13, draws 9.9e-14; kinds x
orders, d = 1, 8, 17 werr 1.4e-13, draws 1.6e-13; Matern log mode 7.2e-14, same bits as the literal mode; batched set-up werr
5.2e-13, draws 3.1e-13; round trip 1.2e-14 of max |yobs - mean|, 2.5e-14 at kappa_2 = 4.0e3; diagonal against
gpemu_predict_batch's variance 4.0e-16 kappa, mean 0.  The reference's own error on these inputs: tests/test_jointref.py."""
import ctypes as C

import numpy as np
import pytest

import jointref
import predcovref
from madaiemulator_amd import abi
from test_gpu_mean_grad import model
from test_gpu_predict_mean import setup
from test_gpu_var_grad import RAGGED, forms_inputs, kinds_inputs, log_mode_inputs, ragged_inputs, stale_inputs

RTOL = jointref.RTOL
pytestmark = pytest.mark.gpu
SIZES = (1, 2, 63, 64, 65, 128, 129, 200, 321, 577)
KINDS = [(k, o, 300, 8) for k in (1, 2, 3) for o in (0, 2)] + [(1, 1, 200, 1), (2, 1, 200, 17), (3, 1, 200, 17)]


# ------------------------------------------------------------------ inputs (also used by tests/test_jointref.py)
def fresh(inputs, M, seed):
    """(kind, order, X, y, th, old queries) -> the same model with M fresh queries"""
    kind, order, X, y, th = inputs[:5]
    return kind, order, X, y, th, jointref.fresh_queries(X, M, seed)


def sizes_inputs(kind):
    """the model every size is called on: pow-exp N = 513, Matern 5/2 N = 129, d = 3, 577 / 200 fresh queries"""
    return fresh(ragged_inputs(kind, 513 if kind == 1 else 129), 577 if kind == 1 else 200, 7100 + kind)


def ragged_joint_inputs(kind, N):
    return fresh(ragged_inputs(kind, N), 200, 7200 + N)


def kinds_joint_inputs(kind, order, N, d):
    return fresh(kinds_inputs(kind, order, N, d), 70, 7300 + 10 * kind + order)


def log_mode_joint_inputs(kind):
    return fresh(log_mode_inputs(kind), 70, 7400 + kind)


def entries_joint_inputs():
    kind, order, N, d = 3, 1, 513, 3
    X, y, th = model(kind, order, N, d)
    return kind, order, X, y, th, jointref.fresh_queries(X, 200, 7500)


def ill_inputs():
    """pow-exp, N = 63, d = 3, 600 fresh queries, nugget e^-10 = 4.5e-5: few training points under many correlated queries leave
    a large leading eigenvalue, so kappa_2(S) is of the order of 1e4 -- and S still safely positive definite: its smallest
    eigenvalue is the nugget, eleven orders above the rounding of its elements"""
    kind, order, X, y, th, _ = ragged_inputs(1, 63)
    th = th.copy()
    th[1] = -10.0
    return kind, order, X, y, th, jointref.fresh_queries(X, 600, 7600)


def normals(n, M, seed):
    return np.random.default_rng(seed).standard_normal((n, M))


# ------------------------------------------------------------------ the comparison
def check(what, got, ref, out=None):
    """got: predict_joint_factor's dict; ref: jointref's dict for the same M; out: the draws for ref['z']"""
    M = ref["mean"].size
    assert got["status"] == abi.OK and got["info"] == 0, (what, got["status"], got["info"])
    for k in ("mean", "var", "werr", "maha", "logpdf"):
        assert np.all(np.isfinite(got[k])), (what, k)
    emean = float(np.max(np.abs(got["mean"] - ref["mean"]) / np.maximum(1.0, np.abs(ref["mean"]))))
    evar = float(np.max(np.abs(got["var"] - ref["var"])) / ref["kappa"])
    g = dict(werr=got["werr"], maha=got["maha"], logdet=got["logdet"])
    if out is not None:
        g["out"] = out
    zmax = float(np.max(np.abs(ref["z"]))) if ref["z"].size else 1.0
    e = jointref.errors(g, ref, M, zmax, float(ref["var"].max()))
    elp = 0.0
    if ref["maha"].size:
        bar = 0.5 * RTOL * (np.maximum(1.0, ref["maha"]) + M)
        elp = float(np.max(np.abs(got["logpdf"] - ref["logpdf"]) / bar)) * RTOL
    print(f"{what}: mean {emean:.3e} var {evar:.3e} " + " ".join(f"{k} {v:.3e}" for k, v in e.items()) +
          f" logpdf {elp:.3e} of its bar's scale  (bars {RTOL:.1e})")
    assert emean <= RTOL and evar <= RTOL and elp <= RTOL and all(v <= RTOL for v in e.values()), (what, emean, evar, elp, e)
    return e


def run(ctx, Xq, noise, ref):
    """factor + draws for one reference"""
    got = ctx.predict_joint_factor(Xq, noise, ref["yobs"] if ref["yobs"].shape[0] else None)
    out = ctx.predict_joint_draw(ref["z"]) if ref["z"].shape[0] else None
    return got, out


# ------------------------------------------------------------------ 1. every size against the leading part of one reference
@pytest.mark.parametrize("kind", [1, 3])
def test_sizes(gpu_ctx, kind):
    """tile and pad edges, the 128-column pair, uneven recursion, and (pow-exp) the outer panels of M' = 640; noise on the
    pow-exp model, none on the Matern one; three observation rows, 17 draws"""
    kind, order, X, y, th, Xq = sizes_inputs(kind)
    Mmax = Xq.shape[0]
    noise = jointref.noise_for(predcovref.vargradref.kappa(kind, th), Mmax, 5) if kind == 1 else None
    full = jointref.reference(kind, order, X, y, th, Xq, noise, z=normals(17, Mmax, 6), nobs=3, seed=8)
    print(f"kind {kind}: kappa_2(S) {full['kappa2']:.1f}, reference errors {full['ref_err']}")
    setup(gpu_ctx, kind, order, X, y, th)
    for M in (m for m in SIZES if m <= Mmax):
        ref = jointref.leading(full, M)
        got, out = run(gpu_ctx, Xq[:M], None if noise is None else noise[:M], ref)
        check(f"kind {kind} M {M}", got, ref, out)


# ------------------------------------------------------------------ 2. ragged N
@pytest.mark.parametrize("kind,N", RAGGED)
def test_ragged_n(gpu_ctx, kind, N):
    """N around the 64-point block and N = 513 under M = 200 queries; one observation row, one draw"""
    kind, order, X, y, th, Xq = ragged_joint_inputs(kind, N)
    ref = jointref.reference(kind, order, X, y, th, Xq, None, z=normals(1, 200, N), nobs=1, seed=N)
    setup(gpu_ctx, kind, order, X, y, th)
    got, out = run(gpu_ctx, Xq, None, ref)
    check(f"kind {kind} N {N} kappa_2 {ref['kappa2']:.1f}", got, ref, out)


# ------------------------------------------------------------------ 3. nobs and ndraw
def test_nobs_and_ndraw(gpu_ctx):
    """nobs = 0, 1, 3 and all 64 right-hand-side rows; ndraw = 1, 17, 64, 65 (one tile of draws, its edge, two) at M = 200, and
    1025 draws at M = 65: the second block of gpemu_predict_joint_draw.  One reference with 64 rows and 1025 draws; fewer
    rows and draws are its leading rows (a row's numbers do not depend on the other rows)."""
    kind, order, X, y, th, Xq = entries_joint_inputs()
    M = Xq.shape[0]
    noise = jointref.noise_for(predcovref.vargradref.kappa(kind, th), M, 15)
    full = jointref.reference(kind, order, X, y, th, Xq, noise, z=normals(65, M, 16), nobs=64, seed=18)
    setup(gpu_ctx, kind, order, X, y, th)

    def rows(ref, nobs, nd):
        r = dict(ref)
        r.update(werr=ref["werr"][:nobs], maha=ref["maha"][:nobs], logpdf=ref["logpdf"][:nobs], yobs=ref["yobs"][:nobs],
                 z=ref["z"][:nd], out=ref["out"][:nd])
        return r

    for nobs, nd in ((0, 1), (1, 17), (3, 64), (64, 65)):
        ref = rows(full, nobs, nd)
        got, out = run(gpu_ctx, Xq, noise, ref)
        assert got["werr"].shape == (nobs, M) and out.shape == (nd, M)
        check(f"nobs {nobs} ndraw {nd}", got, ref, out)
    small = jointref.leading(full, 65)
    z = normals(1025, 65, 19)
    small.update(z=z, out=small["mean"] + z @ small["L"].T)
    got, out = run(gpu_ctx, Xq[:65], noise[:65], small)
    check("M 65 ndraw 1025", got, small, out)
    gpu_ctx.prof_begin(abi.PROF_JOINT)
    gpu_ctx.predict_joint_draw(z)
    assert gpu_ctx.prof_end()["n"] == 2                        # two blocks, one staging launch each
    gpu_ctx.prof_begin(abi.PROF_JOINT)
    gpu_ctx.predict_joint_factor(Xq, noise, full["yobs"])
    p = gpu_ctx.prof_end()
    assert p["n"] == 2 and p["ms"] > 0                          # staging and clean


# ------------------------------------------------------------------ 4. kinds, orders, dimensions
@pytest.mark.parametrize("kind,order,N,d", KINDS)
def test_kinds_and_orders(gpu_ctx, kind, order, N, d):
    """every covariance function at regression orders 0 and 2 (d = 8), d = 1 and d = 17; M = 70: two tile rows; noise on the
    order-2 cases"""
    kind, order, X, y, th, Xq = kinds_joint_inputs(kind, order, N, d)
    noise = jointref.noise_for(predcovref.vargradref.kappa(kind, th), 70, 25) if order == 2 else None
    ref = jointref.reference(kind, order, X, y, th, Xq, noise, z=normals(3, 70, 26), nobs=3, seed=28)
    setup(gpu_ctx, kind, order, X, y, th)
    got, out = run(gpu_ctx, Xq, noise, ref)
    check(f"kind {kind} order {order} N {N} d {d} kappa_2 {ref['kappa2']:.1f}", got, ref, out)


# ------------------------------------------------------------------ 5. Matern log mode
@pytest.mark.parametrize("kind", [2, 3])
def test_matern_log_mode(kind):
    """GPEMU_MODE_MATERN_LOG: the reference runs the literal kernel at the exponentials; the two modes return the same bits"""
    kind, order, X, y, th_raw, Xq = log_mode_joint_inputs(kind)
    th_log = np.array([0.3, -3.0, np.log(0.8)])
    ref = jointref.reference(kind, order, X, y, th_raw, Xq, None, z=normals(2, 70, 36), nobs=2, seed=38)
    a, b = abi.Context(0), abi.Context(0)
    try:
        a.set_mode(abi.MODE_MATERN_LOG)
        setup(a, kind, order, X, y, th_log)
        setup(b, kind, order, X, y, th_raw)
        ga, oa = run(a, Xq, None, ref)
        gb, ob = run(b, Xq, None, ref)
    finally:
        a.close()
        b.close()
    check(f"kind {kind} log mode", ga, ref, oa)
    check(f"kind {kind} literal mode", gb, ref, ob)
    assert np.array_equal(oa, ob) and all(np.array_equal(ga[k], gb[k]) for k in ga)


# ------------------------------------------------------------------ 6. round trip
def test_round_trip(gpu_ctx):
    """a draw with z = the call's own whitened errors returns the observations: L (L^-1 (y - mean)) + mean, within
    RTOL max |yobs - mean|.  Also where kappa_2(S) is 1e4 (nugget e^-10): the forward substitution and the product with the
    same factor are backward stable, so the round trip does not feel the conditioning; only it and finiteness are checked there."""
    for name, inputs, lo, hi in (("well conditioned", entries_joint_inputs(), 1.0, 1e3), ("nugget e^-10", ill_inputs(), 1e3, 1e6)):
        kind, order, X, y, th, Xq = inputs
        M = Xq.shape[0]
        cov = predcovref.predict(kind, order, X, y, th, Xq)
        lam = np.linalg.eigvalsh(0.5 * (cov["cov"] + cov["cov"].T))
        k2 = float(lam[-1] / lam[0])
        assert lam[0] > 0 and lo <= k2 <= hi, (name, k2)
        yobs = cov["mean"] + np.sqrt(cov["var"]) * normals(5, M, 46)
        setup(gpu_ctx, kind, order, X, y, th)
        got = gpu_ctx.predict_joint_factor(Xq, None, yobs)
        assert got["status"] == abi.OK and all(np.all(np.isfinite(got[k])) for k in ("mean", "var", "werr", "maha", "logpdf"))
        assert np.isfinite(got["logdet"])
        back = gpu_ctx.predict_joint_draw(got["werr"])
        err = float(np.max(np.abs(back - yobs)) / np.max(np.abs(yobs - got["mean"])))
        print(f"{name}: kappa_2(S) {k2:.3g}, round trip {err:.3e} of max |yobs - mean|  (bar {RTOL:.1e})")
        assert err <= RTOL


# ------------------------------------------------------------------ 7. the diagonal
def test_diagonal_is_the_variance(gpu_ctx):
    """var without noise is gpemu_predict_batch's variance, and the mean its mean, to the bars of test_gpu_predict_cov"""
    kind, order, X, y, th, Xq = entries_joint_inputs()
    setup(gpu_ctx, kind, order, X, y, th)
    pm, pv = gpu_ctx.predict(Xq)
    got = gpu_ctx.predict_joint_factor(Xq)
    kap = predcovref.vargradref.kappa(kind, th)
    ed = float(np.max(np.abs(got["var"] - pv)) / kap)
    em = float(np.max(np.abs(got["mean"] - pm) / np.maximum(1.0, np.abs(pm))))
    print(f"diagonal against gpemu_predict_batch's variance {ed:.3e} of kappa, mean {em:.3e}")
    assert got["status"] == abi.OK and ed <= RTOL and em <= RTOL
    noise = jointref.noise_for(kap, Xq.shape[0], 55)
    assert np.array_equal(gpu_ctx.predict_joint_factor(Xq, noise)["var"], got["var"] + noise)


# ------------------------------------------------------------------ 8. same bits everywhere
def dev_call(ctx, Xq, noise, yobs, z):
    """the _dev entries on buffers of the caller's -> (dict like predict_joint_factor's without logpdf, draws)"""
    M, d = Xq.shape
    nobs, nd = yobs.shape[0], z.shape[0]
    sizes = dict(xq=M * d, noise=M, yobs=nobs * M, mean=M, var=M, werr=nobs * M, stat=1 + nobs, info=2, z=nd * M, out=nd * M)
    buf = ctx.dev_alloc(8 * sum(sizes.values()))
    try:
        p, off = {}, 0
        for k, n in sizes.items():
            p[k] = buf.value + 8 * off
            off += n
        ctx.upload(p["xq"], Xq)
        ctx.upload(p["noise"], noise)
        ctx.upload(p["yobs"], yobs)
        ctx.upload(p["z"], z)
        ctx.predict_joint_factor_dev(M, p["xq"], p["noise"], nobs, p["yobs"], p["mean"], p["var"], p["werr"], p["stat"], p["info"])
        ctx.predict_joint_draw_dev(nd, p["z"], p["out"])
        ctx.sync()
        stat = ctx.download(p["stat"], (1 + nobs,))
        info = int(ctx.download(p["info"], (1,), dtype=np.int32)[0])
        got = dict(mean=ctx.download(p["mean"], (M,)), var=ctx.download(p["var"], (M,)), werr=ctx.download(p["werr"], (nobs, M)),
                   maha=stat[1:], logdet=float(stat[0]), info=0 if info >= 0x7f7f7f7f else info)
        return got, ctx.download(p["out"], (nd, M))
    finally:
        ctx.dev_free(buf)


def test_same_bits_everywhere(gpu_ctx):
    """two calls; the device-pointer entries; a shorter call after a longer one against a fresh context (nothing stale is
    read); and gpemu_predict_cov, gpemu_predict_batch and the gradients return the bits they returned before"""
    kind, order, X, y, th, Xq = entries_joint_inputs()
    M = Xq.shape[0]
    noise = jointref.noise_for(predcovref.vargradref.kappa(kind, th), M, 65)
    z = normals(17, M, 66)
    setup(gpu_ctx, kind, order, X, y, th)
    before = gpu_ctx.predict_cov(Xq) + gpu_ctx.predict(Xq) + gpu_ctx.predict_var_grad(Xq)
    yobs = before[0] + np.sqrt(np.diag(before[1])) * normals(3, M, 67)
    g1, o1 = gpu_ctx.predict_joint_factor(Xq, noise, yobs), gpu_ctx.predict_joint_draw(z)
    g2, o2 = gpu_ctx.predict_joint_factor(Xq, noise, yobs), gpu_ctx.predict_joint_draw(z)
    assert g1["status"] == abi.OK and np.array_equal(o1, o2) and all(np.array_equal(g1[k], g2[k]) for k in g1)
    after = gpu_ctx.predict_cov(Xq) + gpu_ctx.predict(Xq) + gpu_ctx.predict_var_grad(Xq)
    for u, w in zip(before, after):
        assert np.array_equal(u, w)
    gd, od = dev_call(gpu_ctx, Xq, noise, yobs, z)
    assert np.array_equal(od, o1) and all(np.array_equal(gd[k], g1[k]) for k in gd)
    # a shorter call after the longer one, against a context that has never held anything else
    g70, o70 = gpu_ctx.predict_joint_factor(Xq[:70], noise[:70], yobs[:, :70]), gpu_ctx.predict_joint_draw(z[:, :70])
    c = abi.Context(0)
    try:
        setup(c, kind, order, X, y, th)
        f70, p70 = c.predict_joint_factor(Xq[:70], noise[:70], yobs[:, :70]), c.predict_joint_draw(z[:, :70])
    finally:
        c.close()
    assert np.array_equal(o70, p70) and all(np.array_equal(g70[k], f70[k]) for k in g70)
    # the whitened errors of a leading block are the leading columns: forward substitution
    assert np.array_equal(g70["werr"], g1["werr"][:, :70]) and np.array_equal(g70["var"], g1["var"][:70])


def test_setup_by_batch_same_bits():
    """two contexts through gpemu_predict_setup_batch: each answers for its own state, in the bits of a context set up alone"""
    kind, order, X, y, th1, th2, y2, _ = stale_inputs()
    Xq = jointref.fresh_queries(X, 70, 7700)
    ys, ths = [y, y2], [th1, th2]
    z = normals(4, 70, 76)
    ctxs = [abi.Context(0) for _ in range(2)]
    try:
        for c, yc in zip(ctxs, ys):
            c.set_model(kind, order, X, yc)
        _, _, status, rc = abi.predict_setup_batch(ctxs, np.array(ths))
        assert rc == abi.OK and not status.any()
        for c, yc, tc in zip(ctxs, ys, ths):
            ref = jointref.reference(kind, order, X, yc, tc, Xq, None, z=z, nobs=2, seed=78)
            got, out = run(c, Xq, None, ref)
            check("component of a batched set-up", got, ref, out)
            alone = abi.Context(0)
            try:
                setup(alone, kind, order, X, yc, tc)
                want, wout = run(alone, Xq, None, ref)
            finally:
                alone.close()
            assert np.array_equal(out, wout) and all(np.array_equal(got[k], want[k]) for k in got)
    finally:
        for c in ctxs:
            c.close()


# ------------------------------------------------------------------ 9. a failed pivot
def test_failed_pivot(gpu_ctx):
    """noise_p = -2 var_p at p = 70 (0-based) of M = 200 makes S_pp negative: GPEMU_ERR_NOT_PD with info = 71, mean and var
    finite, the rest NaN, no factor left"""
    kind, order, X, y, th, Xq = entries_joint_inputs()
    M = Xq.shape[0]
    setup(gpu_ctx, kind, order, X, y, th)
    good = gpu_ctx.predict_joint_factor(Xq)
    assert good["status"] == abi.OK
    noise = np.zeros(M)
    noise[70] = -2.0 * good["var"][70]
    yobs = good["mean"] + normals(2, M, 86)
    got = gpu_ctx.predict_joint_factor(Xq, noise, yobs)
    assert got["status"] == abi.ERR_NOT_PD and got["info"] == 71
    assert np.all(np.isfinite(got["mean"])) and np.all(np.isfinite(got["var"]))
    assert np.array_equal(got["mean"], good["mean"]) and got["var"][70] == -good["var"][70]
    assert np.all(np.isnan(got["werr"])) and np.all(np.isnan(got["maha"])) and np.all(np.isnan(got["logpdf"])) and np.isnan(got["logdet"])
    with pytest.raises(abi.GpemuError) as ei:
        gpu_ctx.predict_joint_draw(np.zeros((1, M)))
    assert ei.value.code == abi.ERR_STATE
    again = gpu_ctx.predict_joint_factor(Xq)                      # usable afterwards, same bits
    assert again["status"] == abi.OK and all(np.array_equal(again[k], good[k]) for k in good)


# ------------------------------------------------------------------ 10. state and errors
def free_bytes():
    fr, tot = C.c_size_t(0), C.c_size_t(0)
    assert abi.load().gpemu_device_memory(0, C.byref(fr), C.byref(tot)) == abi.OK
    return fr.value


def test_state_and_errors():
    kind, order, N, d = 1, 1, 150, 3
    X, y, th = model(kind, order, N, d)
    Xq = jointref.fresh_queries(X, 40, 7800)
    z = normals(2, 40, 96)
    c = abi.Context(0)
    try:
        dp, L = abi._p, c.L
        info = C.c_int(0)
        buf = np.empty(40 * 40)

        def factor(M=40, xq=dp(Xq), nobs=0, yobs=None, inf=C.byref(info)):
            return L.gpemu_predict_joint_factor(c.h, M, xq, None, nobs, yobs, None, None, None, None, None, None, inf)

        c.set_model(kind, order, X, y)
        assert factor() == abi.ERR_STATE                           # before predict_setup
        assert L.gpemu_predict_joint_factor_dev(c.h, 40, 8, None, 0, None, None, None, None, None, 8) == abi.ERR_STATE
        assert L.gpemu_predict_joint_draw(c.h, 2, dp(z), dp(buf)) == abi.ERR_STATE
        setup(c, kind, order, X, y, th)
        assert L.gpemu_predict_joint_draw(c.h, 2, dp(z), dp(buf)) == abi.ERR_STATE      # set up, but no factor yet
        assert L.gpemu_predict_joint_draw_dev(c.h, 2, 8, 8) == abi.ERR_STATE
        c.sync()
        fr0 = free_bytes()
        assert L.gpemu_predict_joint_factor(None, 40, dp(Xq), None, 0, None, None, None, None, None, None, None, C.byref(info)) == abi.ERR_ARG
        assert factor(xq=None) == abi.ERR_ARG and factor(inf=None) == abi.ERR_ARG
        assert factor(M=0) == abi.ERR_ARG and factor(M=-3) == abi.ERR_ARG and factor(M=16385) == abi.ERR_ARG
        assert factor(nobs=-1) == abi.ERR_ARG and factor(nobs=65, yobs=dp(buf)) == abi.ERR_ARG and factor(nobs=1) == abi.ERR_ARG
        for args in ((0, 8, None, 0, None), (16385, 8, None, 0, None), (40, None, None, 0, None), (40, 8, None, 65, 8), (40, 8, None, 2, None)):
            assert L.gpemu_predict_joint_factor_dev(c.h, *args, None, None, None, None, 8) == abi.ERR_ARG
        assert L.gpemu_predict_joint_factor_dev(c.h, 40, 8, None, 0, None, None, None, None, None, None) == abi.ERR_ARG
        assert free_bytes() == fr0                                 # refused before anything was allocated
        g0 = c.predict_joint_factor(Xq)
        o0 = c.predict_joint_draw(z)
        assert g0["status"] == abi.OK
        assert L.gpemu_predict_joint_draw(c.h, 0, dp(z), dp(buf)) == abi.ERR_ARG
        assert L.gpemu_predict_joint_draw(c.h, 2, None, dp(buf)) == abi.ERR_ARG
        assert L.gpemu_predict_joint_draw(c.h, 2, dp(z), None) == abi.ERR_ARG
        assert L.gpemu_predict_joint_draw_dev(c.h, 2, None, 8) == abi.ERR_ARG
        assert L.gpemu_predict_joint_draw_dev(c.h, 2, 8, None) == abi.ERR_ARG
        assert L.gpemu_predict_joint_draw_dev(c.h, 0, 8, 8) == abi.ERR_ARG
        assert L.gpemu_predict_joint_release(None) == abi.ERR_ARG
        assert np.array_equal(c.predict_joint_draw(z), o0)         # the refusals left the factor alone
        # the host factor entry stages through the buffers of a pending batch: it and the host draw entry are refused while
        # one is pending, and the batch stays collectable; the refused calls also leave the resident factor alone
        for enq, col in ((c.predict_enqueue, c.predict_collect), (c.predict_mean_enqueue, c.predict_mean_collect),
                         (c.predict_mean_grad_enqueue, c.predict_mean_grad_collect), (c.predict_var_grad_enqueue, c.predict_var_grad_collect)):
            enq(Xq)
            want = col()
            enq(Xq)
            assert factor() == abi.ERR_STATE and factor(M=0) == abi.ERR_ARG
            assert L.gpemu_predict_joint_draw(c.h, 2, dp(z), dp(buf)) == abi.ERR_STATE
            assert L.gpemu_predict_joint_draw(c.h, 0, dp(z), dp(buf)) == abi.ERR_ARG
            got = col()
            for u, w in zip(got if isinstance(got, tuple) else (got,), want if isinstance(want, tuple) else (want,)):
                assert np.array_equal(u, w)
        assert np.array_equal(c.predict_joint_draw(z), o0)
        # what ends the factor's life: release, a new training vector, a new set-up
        c.predict_joint_release()
        assert L.gpemu_predict_joint_draw(c.h, 2, dp(z), dp(buf)) == abi.ERR_STATE
        g1 = c.predict_joint_factor(Xq)
        assert all(np.array_equal(g1[k], g0[k]) for k in g0) and np.array_equal(c.predict_joint_draw(z), o0)
        _, rc = c.predict_setup(th)
        assert rc == abi.OK
        assert L.gpemu_predict_joint_draw(c.h, 2, dp(z), dp(buf)) == abi.ERR_STATE
        c.predict_joint_factor(Xq)
        c.set_training(y + 1.0)
        assert L.gpemu_predict_joint_draw(c.h, 2, dp(z), dp(buf)) == abi.ERR_STATE
        assert factor() == abi.ERR_STATE
    finally:
        c.close()
