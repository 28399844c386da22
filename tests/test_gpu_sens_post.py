"""Emulator uncertainty of the main effects and Sobol indices in closed form (gpemu_sens_post / gpemu_sens_main_var,
include/gpemu.h) through the public entries, against tests/senspostref.py (numpy fp64; test_senspostref.py
pins it against mpmath and against quadrature of the posterior covariance itself).

What is compared.  S_u is a function of (design, amplitude, lengths, box, P, G, Q).  P, G and Q are taken from the device
(gpemu_test_sens_post_state), beta and gamma from gpemu_test_pred_state: the bar is a few ulp of the SCALE
|CC_u| + A^2 sum |P_ii'| KK_u + sum |Q_ab Hm_u| + 2 sum |G_ia HK_u|, and another factorisation's C^-1 differs from the device's
by far more.  Everything downstream -- the integrals, the weighted N x N sweep, the assembly -- is the reference's own.  That
P itself is C^-1 - W Q W^T is checked against gpemu_get_cinverse.

The bar.  NP_VS_MP is the largest scaled error of the numpy reference against mpmath at 50 digits over exactly the cases of
this file (`all_cases()`, with P, G, Q from a numpy fit in place of the device's), measured on the CPU by
`python tests/senspostref.py --measure`.  The device gets FACTOR = 8 times that, as in test_gpu_sens.py and for the same
reason: it sums in another order and its erf may differ from libm's by a few ulp per term.
  measured NP_VS_MP = 9.1e-16 -> TOL = 7.3e-15                                   
The worst case is the disjoint box at order 0; most cases sit at 5e-16 to 8e-16 whatever the order, which is the relative
error of UU_l (two terms of nearly equal size are subtracted); the S_u themselves are closer than that.  The scale is large
against the values -- P holds entries of size 1 / nugget with alternating signs -- so the bar is some 1e-11 of an S_u.
The two routes to C^-1 (the U U^T corner behind gpemu_sens_post, the product with L^-1 behind gpemu_sens_main_var and
gpemu_predict_batch) are compared at 8 x ROUTES_NP, the discrepancy of the same two computations in numpy (`--measure`).
  measured ROUTES_NP = 2.0e-17 -> ROUTES_TOL = 1.6e-16   (of the same scale: some 1e-13 of the values compared)"""
import numpy as np
import pytest

import sensref as R
import senspostref as SP
from madaiemulator_amd import abi, synth

NP_VS_MP = 9.1e-16
FACTOR = 8
TOL = FACTOR * NP_VS_MP
ROUTES_NP = 2.0e-17
ROUTES_TOL = FACTOR * ROUTES_NP
RTOL = 1e-8                      # the project's parity bar (tests/test_gpu_loo.py): where a figure depends on the fit itself
NUGGET = 1e-3

pytestmark = pytest.mark.gpu

NS = [1, 63, 64, 65, 130, 200]
DS = [1, 2, 3, 8, 17]
ORDERS = [0, 1, 2, 3]
BAND_CASES = [(130, 3, 2, 5), (65, 2, 1, 32), (64, 17, 0, 1), (1, 2, 0, 5), (200, 8, 1, 5)]      # N, d, order, ngrid
ROUTE_CASES = [(130, 2, 1), (65, 2, 2), (200, 2, 0)]


# ---------------------------------------------------------------------------------------------------- inputs
def thetas(d):
    """amplitude 1, nugget 1e-3 (C stays well conditioned), lengths that grow with d so that no k falls under 1e-10 on the unit
    cube: the exponent is at most sum_l 1 / (2 length_l^2) <= 4.2"""
    return np.array([0.0, np.log(NUGGET)] + [np.log(0.6 * max(1.0, np.sqrt(d / 3.0))) + 0.03 * l for l in range(d)])


def data(N, d):
    if N == 1:                                   # (synth.design standardises y: one point has no spread)
        return synth.uniform(900 + d, (1, d)), np.array([0.7])
    X, y = synth.design(N, d, 900 + 31 * N + d)
    return X, y + 1.0


def shape_cases():
    return [(N, d, o) for N in NS for d in DS for o in ORDERS if 1 + o * d <= N]


def model_of(th):
    return dict(A=float(np.exp(th[0])), s=np.exp(-2.0 * th[2:]))


def band_grid(X, lo, hi, ngrid):
    """ngrid values per coordinate: the ends of the box first, then values in between"""
    t = np.array([0.0, 1.0, 0.5, 0.3, 0.81] + list(np.linspace(0.02, 0.98, max(ngrid - 5, 0))))[:ngrid]
    return lo[:, None] + t[None, :] * (hi - lo)[:, None]


def all_cases():
    """every (name, X, y, th, order, lo, hi, ngrid) whose numbers this file compares with senspostref at TOL (ngrid = 0: no band)"""
    out = []
    for N, d, o in shape_cases():
        X, y = data(N, d)
        out.append((f"N{N}-d{d}-o{o}", X, y, thetas(d), o) + R.boxes(X)["design"] + (0,))
    for box in ("narrow", "disjoint"):
        for o in (0, 2):
            X, y = data(130, 3)
            out.append((f"{box}-o{o}", X, y, thetas(3), o) + R.boxes(X)[box] + (5,))
    for N, d, o, ng in BAND_CASES:
        X, y = data(N, d)
        out.append((f"band-N{N}-d{d}-o{o}", X, y, thetas(d), o) + R.boxes(X)["design"] + (ng,))
    return out


def _measure_one(case):
    name, X, y, th, o, lo, hi, ng = case
    m = model_of(th)
    P, G, Q, beta, gamma, _, _ = SP.fit_state(X, y, o, m["A"], m["s"], NUGGET)
    val, scale = SP.post(R.NP, X, m, P, G, Q, lo, hi)
    mp, _ = SP.post(R.MP(), X, m, P, G, Q, lo, hi)
    e = SP.scaled_errors(val, mp, scale)
    d = X.shape[1]
    uu_np, uu_mp = SP.uu(R.NP, m["s"], lo, hi), R.MP.tofloat(SP.uu(R.MP(), R.MP().arr(m["s"]), R.MP().arr(lo), R.MP().arr(hi)))
    e = max(e, float(np.max(np.abs(uu_np - uu_mp) / np.abs(uu_mp))))
    if ng:
        grid = band_grid(X, lo, hi, min(ng, 5))
        bv, bs = SP.band(R.NP, X, m, P, G, Q, beta, gamma, lo, hi, grid)
        bm, _ = SP.band(R.MP(), X, m, P, G, Q, beta, gamma, lo, hi, grid)
        e = max(e, SP.scaled_errors(bv, bm, bs, keys=("var", "var_e0", "main")))
    return name, e


def routes_numpy(X, th, order, lo, hi):
    """the two routes to C^-1 in numpy: -> the scaled discrepancies of (s_first against the Gauss-Legendre average of the
    Cholesky band, s_all + nugget against the Gauss-Legendre average of the Cholesky prediction variance); d = 2"""
    m = model_of(th)
    d = X.shape[1]
    y = np.zeros(len(X))
    P, G, Q = SP.fit_state(X, y, order, m["A"], m["s"], NUGGET)[:3]
    val, scale = SP.post(R.NP, X, m, P, G, Q, lo, hi)
    nodes = [SP.gauss_nodes(lo[l], hi[l]) for l in range(d)]
    grid = np.stack([n for n, _ in nodes])
    T, hm, cc = SP.band_tables(X, m, order, lo, hi, grid)
    e1 = 0.0
    for j in range(d):
        avg = nodes[j][1] @ SP.chol_variance(X, order, m["A"], m["s"], NUGGET, T[j], hm[j], cc[j])
        e1 = max(e1, abs(avg - val["s_first"][j]) / scale["s_first"][j])
    mesh = np.stack([g.ravel() for g in np.meshgrid(*grid, indexing="ij")], axis=1)
    w2 = np.multiply.outer(nodes[0][1], nodes[1][1]).ravel()
    pv = SP.chol_variance(X, order, m["A"], m["s"], NUGGET, m["A"] * SP.kmatrix(mesh, X, m["s"]), SP.hmatrix(mesh, order), m["A"] + NUGGET)
    return e1, abs(w2 @ pv - (val["s_all"] + NUGGET)) / scale["s_all"]


def measure():
    """the figures NP_VS_MP and ROUTES_NP are set from (CPU, minutes)"""
    import multiprocessing as mpc
    import sys
    cases = sorted(all_cases(), key=lambda c: -c[1].size * len(c[1]))
    if "--only" in sys.argv:
        cases = [c for c in cases if c[0].startswith(tuple(sys.argv[sys.argv.index("--only") + 1].split(",")))]
    worst = ("", 0.0)
    with mpc.Pool(min(8, mpc.cpu_count())) as pool:
        for name, e in pool.imap_unordered(_measure_one, cases):
            print(f"{name}: {e:.3e}", flush=True)
            if e > worst[1]:
                worst = (name, e)
    print(f"largest scaled error of numpy against mpmath over {len(cases)} cases: {worst[1]:.3e} ({worst[0]})")
    r = 0.0
    for N, d, o in ROUTE_CASES:
        X, _ = data(N, d)
        e = routes_numpy(X, thetas(d), o, *R.boxes(X)["design"])
        print(f"routes N {N} d {d} order {o}: s_first {e[0]:.3e}, s_all {e[1]:.3e}")
        r = max(r, *e)
    print(f"largest discrepancy of the two routes to C^-1 in numpy: {r:.3e}")


# ---------------------------------------------------------------------------------------------------- helpers
def fit(ctx, order, X, y, th, kind=1):
    ctx.set_model(kind, order, X, y)
    _, rc = ctx.predict_setup(th)
    assert rc == abi.OK, rc
    return model_of(th)


def check(what, got, ref, scale, keys=SP.KEYS, tol=TOL):
    e = SP.scaled_errors(got, ref, scale, keys)
    print(f"{what}: scaled error {e:.2e} (bar {tol:.1e})")
    for k in keys:
        assert np.all(np.isfinite(got[k])), (what, k)
    assert e < tol, (what, e)
    return e


def ordered(what, got, scale):
    """s_none <= s_first[j], s_rest[j] <= s_all and every S >= 0, up to the bar times the scale"""
    for k in ("s_first", "s_rest"):
        slack = TOL * (scale[k] + scale["s_all"] + scale["s_none"])
        assert np.all(got["s_none"] <= got[k] + slack) and np.all(got[k] <= got["s_all"] + slack), (what, k, got)
    for k in SP.KEYS:
        assert np.all(np.asarray(got[k]) >= -TOL * np.asarray(scale[k])), (what, k, got[k])


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in SP.KEYS)


def post_and_reference(ctx, X, m, lo, hi):
    got = ctx.sens_post(lo, hi)
    P, G, Q = ctx.sens_post_state()
    ref, scale = SP.post(R.NP, X, m, P, G, Q, lo, hi)
    return got, ref, scale, (P, G, Q)


# ---------------------------------------------------------------------------------------------------- 1. shapes
@pytest.mark.parametrize("N", NS)
def test_shapes(gpu_ctx, N):
    """one tile, a ragged second one, three tile rows (diagonal, off-diagonal and edge tiles), d = 8, 16 < d = 17 (rolled)"""
    worst = 0.0
    for n, d, o in shape_cases():
        if n != N:
            continue
        X, y = data(N, d)
        lo, hi = R.boxes(X)["design"]
        m = fit(gpu_ctx, o, X, y, thetas(d))
        got, ref, scale, _ = post_and_reference(gpu_ctx, X, m, lo, hi)
        worst = max(worst, check(f"N {N} d {d} order {o}", got, ref, scale))
        ordered(f"N {N} d {d} order {o}", got, scale)
        if d == 1:
            slack = 2 * TOL * scale["s_all"]
            assert abs(got["s_first"][0] - got["s_all"]) <= slack and abs(got["s_rest"][0] - got["s_none"]) <= slack
    print(f"N {N}: worst scaled error {worst:.2e}")


@pytest.mark.parametrize("box", ["narrow", "disjoint"])
@pytest.mark.parametrize("order", [0, 2])
def test_boxes(gpu_ctx, box, order):
    """a narrow box, and one that leaves the design outside (the erfc path)"""
    X, y = data(130, 3)
    lo, hi = R.boxes(X)[box]
    m = fit(gpu_ctx, order, X, y, thetas(3))
    got, ref, scale, (P, G, Q) = post_and_reference(gpu_ctx, X, m, lo, hi)
    check(f"{box} order {order}", got, ref, scale)
    ordered(box, got, scale)
    grid = band_grid(X, lo, hi, 5)
    main, var, ve0 = gpu_ctx.sens_main_var(lo, hi, grid)
    beta, gamma = gpu_ctx.pred_state()
    bref, bscale = SP.band(R.NP, X, m, P, G, Q, beta, gamma, lo, hi, grid)
    check(f"{box} order {order} band", dict(var=var, var_e0=ve0), bref, bscale, keys=("var", "var_e0"))


# ---------------------------------------------------------------------------------------------------- 2. state
def test_p_is_cinverse_minus_wqw(gpu_ctx):
    """P from the hook against numpy's C^-1 - W Q W^T built from gpemu_get_cinverse, to rounding, G against W Q likewise.
    W = C^-1 H is itself a cancelling sum of N terms (numpy's and the corner's differ by N ulp of |C^-1| |H|), so the errors are
    taken element by element relative to  Wa |Q|  and  |C^-1| + Wa |Q| Wa^T  with Wa = |C^-1| |H|; the bar is the rounding of
    the chained sums of N and nreg terms on either side, 4 (N + nreg) 2^-52."""
    for N, d, o in [(130, 3, 2), (65, 8, 1), (1, 2, 0)]:
        X, y = data(N, d)
        lo, hi = R.boxes(X)["design"]
        fit(gpu_ctx, o, X, y, thetas(d))
        gpu_ctx.sens_post(lo, hi)
        P, G, Q = gpu_ctx.sens_post_state()
        Cinv = gpu_ctx.cinverse()
        H = SP.hmatrix(X, o)
        W, Wa = Cinv @ H, np.abs(Cinv) @ np.abs(H)
        nreg = Q.shape[0]
        assert np.array_equal(P, P.T)
        eg = np.abs(G - W @ Q) / (Wa @ np.abs(Q))
        ep = np.abs(P - (Cinv - W @ Q @ W.T)) / (np.abs(Cinv) + Wa @ np.abs(Q) @ Wa.T)
        print(f"N {N} d {d} order {o}: G {eg.max():.2e}, P {ep.max():.2e}")
        assert eg.max() < 4 * (N + nreg) * 2.0 ** -52 and ep.max() < 4 * (N + nreg) * 2.0 ** -52


# ---------------------------------------------------------------------------------------------------- 3. the band
@pytest.mark.parametrize("N,d,order,ngrid", BAND_CASES)
def test_band(gpu_ctx, N, d, order, ngrid):
    """var against the reference on the device's P, G, Q; the curve against gpemu_sens_main and var_e0 against s_none to
    rounding; d = 2 with ngrid = 32 gives 65 rows and crosses the 64-row tile"""
    X, y = data(N, d)
    lo, hi = R.boxes(X)["design"]
    m = fit(gpu_ctx, order, X, y, thetas(d))
    got, _, scale, (P, G, Q) = post_and_reference(gpu_ctx, X, m, lo, hi)
    beta, gamma = gpu_ctx.pred_state()
    grid = band_grid(X, lo, hi, ngrid)
    main, var, ve0 = gpu_ctx.sens_main_var(lo, hi, grid)
    ref, bscale = SP.band(R.NP, X, m, P, G, Q, beta, gamma, lo, hi, grid)
    check(f"band N {N} d {d} order {order} ngrid {ngrid}", dict(main=main, var=var, var_e0=ve0), ref, bscale, keys=("var", "var_e0", "main"))
    e0, curve = gpu_ctx.sens_main(lo, hi, grid)
    assert np.all(np.abs(main - curve) <= TOL * bscale["main"])
    assert abs(ve0 - got["s_none"]) <= TOL * (scale["s_none"] + bscale["var_e0"])
    assert np.all(var >= -TOL * bscale["var"])
    again = gpu_ctx.sens_main_var(lo, hi, grid)
    assert np.array_equal(again[0], main) and np.array_equal(again[1], var) and again[2] == ve0
    # a row's bits do not depend on how many rows the call has; main may be left out
    one = gpu_ctx.sens_main_var(lo, hi, grid[:, :1])
    assert np.array_equal(one[1][:, 0], var[:, 0]) and one[2] == ve0


# ---------------------------------------------------------------------------------------------------- 4. two routes to C^-1
@pytest.mark.parametrize("N,d,order", ROUTE_CASES)
def test_two_routes_agree(gpu_ctx, N, d, order):
    """s_first[j] (the U U^T corner) against 24-point Gauss-Legendre quadrature over x_j of gpemu_sens_main_var's own output
    (L^-1 T); s_all + nugget against the Gauss-Legendre average of gpemu_predict_batch's variance over 24^2 nodes"""
    X, y = data(N, d)
    lo, hi = R.boxes(X)["design"]
    m = fit(gpu_ctx, order, X, y, thetas(d))
    got, _, scale, _ = post_and_reference(gpu_ctx, X, m, lo, hi)
    nodes = [SP.gauss_nodes(lo[l], hi[l]) for l in range(d)]
    grid = np.stack([n for n, _ in nodes])
    _, var, _ = gpu_ctx.sens_main_var(lo, hi, grid)
    for j in range(d):
        e = abs(nodes[j][1] @ var[j] - got["s_first"][j]) / scale["s_first"][j]
        print(f"N {N} order {order}: s_first[{j}] against the band's average {e:.2e} (bar {ROUTES_TOL:.1e})")
        assert e < ROUTES_TOL
    mesh = np.stack([g.ravel() for g in np.meshgrid(*grid, indexing="ij")], axis=1)
    w2 = np.multiply.outer(nodes[0][1], nodes[1][1]).ravel()
    _, pv = gpu_ctx.predict(mesh)
    e = abs(w2 @ pv - (got["s_all"] + NUGGET)) / scale["s_all"]
    print(f"N {N} order {order}: s_all + nugget against the average prediction variance {e:.2e} (bar {ROUTES_TOL:.1e})")
    assert e < ROUTES_TOL


# ---------------------------------------------------------------------------------------------------- 5. bits, bystanders
def _dev_call(ctx, lo, hi):
    d = ctx.d
    buf = ctx.dev_alloc((2 + 2 * d) * 8)
    try:
        ctx.sens_post_dev(lo, hi, buf)
        o = ctx.download(buf, (2 + 2 * d,))
    finally:
        ctx.dev_free(buf)
    return dict(s_none=o[0], s_all=o[1], s_first=o[2:2 + d], s_rest=o[2 + d:])


def test_same_bits_and_bystanders(gpu_ctx):
    N, d, order = 200, 3, 1
    X, y = data(N, d)
    fit(gpu_ctx, order, X, y, thetas(d))
    lo, hi = R.boxes(X)["narrow"]
    Xq = X[:9] + 0.01
    cov_before, cinv_before = gpu_ctx.sens_cov(lo, hi), gpu_ctx.cinverse()
    a = gpu_ctx.sens_post(lo, hi)
    assert same_bits(a, gpu_ctx.sens_post(lo, hi))
    assert same_bits(a, _dev_call(gpu_ctx, lo, hi))
    gpu_ctx.sens_release()
    with pytest.raises(abi.GpemuError) as ei:
        gpu_ctx.sens_post_state()
    assert ei.value.code == abi.ERR_STATE
    assert same_bits(a, gpu_ctx.sens_post(lo, hi))
    # gpemu_sens_cov and gpemu_get_cinverse return the same bits before and after
    cov_after = gpu_ctx.sens_cov(lo, hi)
    assert all(np.array_equal(cov_before[k], cov_after[k]) for k in R.KEYS)
    assert np.array_equal(cinv_before, gpu_ctx.cinverse())
    # a pending prediction batch stays collectable across the band entry (which uses the batch buffers in stream order)
    want = gpu_ctx.predict(Xq)
    gpu_ctx.predict_enqueue(Xq)
    gpu_ctx.sens_main_var(lo, hi, band_grid(X, lo, hi, 5))
    gpu_ctx.sens_post(lo, hi)
    got = gpu_ctx.predict_collect()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # profiling class: four launches for the S terms, three for one block of the band
    gpu_ctx.prof_begin(abi.PROF_SENS_POST)
    gpu_ctx.sens_post(lo, hi)
    p = gpu_ctx.prof_end()
    print("PROF_SENS_POST:", p)
    assert p["n"] == 4 and p["ms"] > 0
    gpu_ctx.prof_begin(abi.PROF_SENS_POST)
    gpu_ctx.sens_main_var(lo, hi, band_grid(X, lo, hi, 5))
    assert gpu_ctx.prof_end()["n"] == 3


def test_setup_by_batch_same_bits():
    """components set up by gpemu_predict_setup_batch against contexts set up alone: component 0, and a later component
    (which factors alone before its corner is built)"""
    N, d, order = 130, 3, 1
    X, y = data(N, d)
    ys, ths = [y, np.cos(2.0 * y) + 0.3 * X[:, 0]], [thetas(d), thetas(d) + np.array([0, 0, 0.2, 0.2, 0.2])]
    lo, hi = R.boxes(X)["design"]
    grid = band_grid(X, lo, hi, 5)
    ctxs, alone = [abi.Context(0) for _ in ys], [abi.Context(0) for _ in ys]
    try:
        for c, yc in zip(ctxs, ys):
            c.set_model(1, order, X, yc)
        _, _, status, rc = abi.predict_setup_batch(ctxs, np.array(ths))
        assert rc == abi.OK and not status.any()
        for c, yc, tc in zip(alone, ys, ths):
            fit(c, order, X, yc, tc)
        for i in (0, 1):
            bm, bv, b0 = ctxs[i].sens_main_var(lo, hi, grid)
            am, av, a0 = alone[i].sens_main_var(lo, hi, grid)
            assert np.array_equal(bm, am) and np.array_equal(bv, av) and b0 == a0
            assert same_bits(ctxs[i].sens_post(lo, hi), alone[i].sens_post(lo, hi))
    finally:
        for c in ctxs + alone:
            c.close()


# ---------------------------------------------------------------------------------------------------- 6. errors
def _post_rc(a, lo, hi, sn=True, sa=True, sf=True, sr=True):
    d = max(a.d, 1)
    bufs = [np.empty(1), np.empty(1), np.empty(d), np.empty(d)]
    ptr = [abi._p(x) if on else None for x, on in zip(bufs, (sn, sa, sf, sr))]
    lo = None if lo is None else abi._a(lo)
    hi = None if hi is None else abi._a(hi)
    return a.L.gpemu_sens_post(a.h, None if lo is None else abi._p(lo), None if hi is None else abi._p(hi), *ptr)


def _band_rc(a, lo, hi, ngrid, grid=True, main=True, var=True, ve0=True):
    d = max(a.d, 1)
    g, m, v, e = np.full(d * max(ngrid, 1), 0.5), np.empty(d * max(ngrid, 1)), np.empty(d * max(ngrid, 1)), np.empty(1)
    lo, hi = abi._a(lo), abi._a(hi)
    return a.L.gpemu_sens_main_var(a.h, abi._p(lo), abi._p(hi), ngrid, abi._p(g) if grid else None, abi._p(m) if main else None,
                                   abi._p(v) if var else None, abi._p(e) if ve0 else None)


def test_errors(gpu_ctx):
    N, d, order = 90, 3, 1
    X, y = data(N, d)
    th = thetas(d)
    lo, hi = R.boxes(X)["design"]
    L = gpu_ctx.L
    fresh = abi.Context(0)
    try:
        fresh.set_model(1, order, X, y)
        fit(gpu_ctx, order, X, y, th)
        # NULL pointers come first, whatever the state
        for kw in (dict(sn=False), dict(sa=False), dict(sf=False), dict(sr=False)):
            assert _post_rc(fresh, lo, hi, **kw) == abi.ERR_ARG
        assert _post_rc(fresh, None, hi) == abi.ERR_ARG and _post_rc(fresh, lo, None) == abi.ERR_ARG
        assert L.gpemu_sens_post(None, None, None, None, None, None, None) == abi.ERR_ARG
        assert L.gpemu_sens_post_dev(fresh.h, abi._p(lo), abi._p(hi), None) == abi.ERR_ARG
        assert L.gpemu_sens_post_dev(None, abi._p(lo), abi._p(hi), None) == abi.ERR_ARG
        for kw in (dict(grid=False), dict(var=False)):
            assert _band_rc(fresh, lo, hi, 3, **kw) == abi.ERR_ARG
        assert _band_rc(fresh, lo, hi, 0) == abi.ERR_ARG and _band_rc(gpu_ctx, lo, hi, 0) == abi.ERR_ARG
        assert L.gpemu_test_sens_post_state(None, None, None, None) == abi.ERR_ARG
        # no prediction set-up
        assert _post_rc(fresh, lo, hi) == abi.ERR_STATE and _band_rc(fresh, lo, hi, 3) == abi.ERR_STATE
        with pytest.raises(abi.GpemuError) as ei:
            fresh.sens_post(lo, hi)
        assert ei.value.code == abi.ERR_STATE
    finally:
        fresh.close()
    assert _post_rc(gpu_ctx, lo, hi) == abi.OK and _band_rc(gpu_ctx, lo, hi, 3) == abi.OK
    assert _band_rc(gpu_ctx, lo, hi, 3, main=False, ve0=False) == abi.OK      # both may be NULL
    for l in range(d):
        for bad in (np.nan, np.inf, -np.inf):
            b = lo.copy(); b[l] = bad
            assert _post_rc(gpu_ctx, b, hi) == abi.ERR_ARG and _band_rc(gpu_ctx, b, hi, 3) == abi.ERR_ARG
            b = hi.copy(); b[l] = bad
            assert _post_rc(gpu_ctx, lo, b) == abi.ERR_ARG
        b = hi.copy(); b[l] = lo[l]
        assert _post_rc(gpu_ctx, lo, b) == abi.ERR_ARG and _band_rc(gpu_ctx, lo, b, 3) == abi.ERR_ARG
    # a Matern model
    gpu_ctx.set_model(3, order, X, y)
    _, rc = gpu_ctx.predict_setup(synth.default_thetas(3, d))
    assert rc == abi.OK
    assert _post_rc(gpu_ctx, lo, hi) == abi.ERR_ARG and _band_rc(gpu_ctx, lo, hi, 3) == abi.ERR_ARG
    assert "power-exponential covariance only" in L.gpemu_last_error(gpu_ctx.h).decode()
    # a refused call has left everything as it was; release, then a second call; a new training vector ends the set-up
    fit(gpu_ctx, order, X, y, th)
    a = gpu_ctx.sens_post(lo, hi)
    gpu_ctx.sens_release()
    assert same_bits(a, gpu_ctx.sens_post(lo, hi))
    gpu_ctx.set_training(y + 1.0)
    assert _post_rc(gpu_ctx, lo, hi) == abi.ERR_STATE
