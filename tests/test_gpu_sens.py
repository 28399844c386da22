"""Main effects and Sobol indices of the posterior mean in closed form (gpemu_sens_cov / gpemu_sens_main, include/gpemu.h,
DESIGN.md 4.14) through the public entries, against tests/sensref.py (numpy fp64 with scipy's erf / erfc; test_sensref.py pins
it against mpmath and against quadrature of the function itself).

What is compared.  The closed form is a function of (design, beta, gamma, amplitude, lengths, box).  beta and gamma are taken
from the device's own prediction state (gpemu_test_pred_state): the bar below is a few ulp, and another factorisation's gamma
differs from the device's by many orders of magnitude more than that.  Everything downstream of the two vectors -- the
integrals, the N x N sweep, the assembly -- is the reference's own.  Errors are relative to the SCALE sensref returns beside
every value (the sum of the absolute values of the parts the value is made of).

The bar.  NP_VS_MP is the largest scaled error of the numpy reference against mpmath at 50 digits over exactly the cases of
this file (every entry of `all_cases()`, with beta and gamma from a LAPACK fit in place of the device's), measured on the CPU
by `python tests/sensref.py --measure`.  The device gets FACTOR = 8 times that: it sums in another order and its erf may
differ from libm's by a few ulp per term.
  measured NP_VS_MP = 1.7e-11 -> TOL = 1.4e-10                                    
The worst case is the disjoint box with beta_0 = 0: order 0 forces sum_i gamma_i = 0, so E0 is a cancelling sum of kernel
integrals and the scale, which takes the parts as they come out, is small.  Next comes the narrow box (3.1e-12: the erf
differences and the J^p recurrence lose digits as 1 / (s w^2) grows); on the design's own box every case stays below 2e-14.
The case at N = 1000, d = 8 is compared with numpy only (mpmath is too slow there) at the same TOL."""
import numpy as np
import pytest

import sensref as R
from madaiemulator_amd import abi, synth

NP_VS_MP = 1.7e-11
FACTOR = 8
TOL = FACTOR * NP_VS_MP
RTOL = 1e-8                      # the project's parity bar (tests/test_gpu_loo.py): where a figure depends on the fit itself

pytestmark = pytest.mark.gpu

NS = [1, 63, 64, 65, 130, 200]
DS = [1, 2, 3, 8, 17]
ORDERS = [0, 1, 2, 3]


# ---------------------------------------------------------------------------------------------------- inputs
def thetas(d, shift=0.0):
    return np.array([0.0, -4.0] + [np.log(0.6) + shift + 0.03 * l for l in range(d)])


def data(N, d, variant=0):
    if N == 1:                                   # (synth.design standardises y: one point has no spread)
        return synth.uniform(700 + d, (1, d)), np.array([0.7 + variant])
    X, y = synth.design(N, d, 700 + 31 * N + d)
    if variant:
        y = np.cos(2.0 * y) + 0.3 * X[:, 0]
    return X, y + 1.0


def shape_cases():
    """(N, d, order) with at least as many points as regression functions (fewer: there is no emulator to analyse)"""
    return [(N, d, o) for N in NS for d in DS for o in ORDERS if 1 + o * d <= N]


def extra_cases():
    """(name, N, d, order, box, cross): the boxes and the two-context case"""
    return [(f"{box}{'-cross' if cross else ''}", 130, 3, order, box, cross)
            for box in ("design", "narrow", "disjoint") for cross in (False, True) for order in (0, 2)]


def model_of(th, beta, gamma):
    return dict(beta=beta, gamma=gamma, A=float(np.exp(th[0])), s=np.exp(-2.0 * th[2:]))


def main_grid(X, lo, hi):
    """the values the main-effect curves are compared at: the ends of the box, a design point, the centre, one more"""
    return np.stack([lo, hi, X[len(X) // 2], (lo + hi) / 2, lo + 0.3 * (hi - lo)], axis=1)


MAIN_CASES = [(130, 3, 2), (65, 8, 1), (64, 17, 0), (1, 2, 0)]


def linear_case():
    X, _ = data(90, 2)
    return X, 2.0 + 3.0 * X[:, 0] - X[:, 1], thetas(2), np.array([0.1, 0.2]), np.array([0.9, 0.7])


def unused_case():
    X, _ = data(130, 3)
    th = thetas(3)
    th[4] = 3.0
    return X, np.sin(3.0 * X[:, 0]) + X[:, 1] ** 2, th


def all_cases():
    """every (name, X, [(y, th), ...one or two...], order, lo, hi, zero_beta0) whose numbers this file compares with sensref
    at TOL; zero_beta0: the training values are shifted by the fitted beta_0 and fitted again"""
    out = []
    for N, d, o in shape_cases():
        X, y = data(N, d)
        lo, hi = R.boxes(X)["design"]
        out.append((f"N{N}-d{d}-o{o}", X, [(y, thetas(d))], o, lo, hi, False))
    for name, N, d, o, box, cross in extra_cases():
        X, y = data(N, d)
        lo, hi = R.boxes(X)[box]
        fits = [(y, thetas(d))] + ([(data(N, d, 1)[1], thetas(d, 0.2))] if cross else [])
        out.append((name + f"-o{o}", X, fits, o, lo, hi, False))
    X, y = data(130, 3)
    out.append(("disjoint-beta0-zero", X, [(y, thetas(3))], 0) + R.boxes(X)["disjoint"] + (True,))
    X, y, th, lo, hi = linear_case()
    out.append(("linear", X, [(y, th)], 1, lo, hi, False))
    X, y, th = unused_case()
    out.append(("unused", X, [(y, th)], 1) + R.boxes(X)["design"] + (False,))
    for N, d, o in MAIN_CASES:
        X, y = data(N, d)
        out.append((f"main-N{N}-d{d}-o{o}-narrow", X, [(y, thetas(d))], o) + R.boxes(X)["narrow"] + (False,))
        if (N, d, o) not in shape_cases():
            out.append((f"main-N{N}-d{d}-o{o}-design", X, [(y, thetas(d))], o) + R.boxes(X)["design"] + (False,))
    return out


def _measure_one(case):
    import meanref
    name, X, fits, o, lo, hi, zero = case
    ms = []
    for y, th in fits:
        beta, gamma = meanref.trained(1, o, X, y, th)
        if zero:
            beta, gamma = meanref.trained(1, o, X, y - beta[0], th)
        ms.append(model_of(th, beta, gamma))
    val, scale = R.covariances(R.NP, X, ms[0], ms[-1], lo, hi)
    mp, _ = R.covariances(R.MP(), X, ms[0], ms[-1], lo, hi)
    e = R.scaled_errors(val, mp, scale)
    grid = main_grid(X, lo, hi)
    mv, msc = R.main_effects(R.NP, X, ms[0], lo, hi, grid)
    mm, _ = R.main_effects(R.MP(), X, ms[0], lo, hi, grid)
    return name, max(e, R.scaled_errors(mv, mm, msc, keys=("e0", "main")))


def measure_np_against_mp():
    """the figure NP_VS_MP is set from (CPU, minutes)"""
    import multiprocessing as mpc
    from oracle import oracle as O
    O.build()
    import sys
    cases = sorted(all_cases(), key=lambda c: -c[1].size * len(c[1]))
    if "--only" in sys.argv:                     # names that start with the given prefixes
        cases = [c for c in cases if c[0].startswith(tuple(sys.argv[sys.argv.index("--only") + 1].split(",")))]
    worst = ("", 0.0)
    with mpc.Pool(min(8, mpc.cpu_count())) as pool:
        for name, e in pool.imap_unordered(_measure_one, cases):
            print(f"{name}: {e:.3e}", flush=True)
            if e > worst[1]:
                worst = (name, e)
    print(f"largest scaled error of numpy against mpmath over {len(cases)} cases: {worst[1]:.3e} ({worst[0]})")


# ---------------------------------------------------------------------------------------------------- helpers
def fit(ctx, order, X, y, th, kind=1):
    ctx.set_model(kind, order, X, y)
    _, rc = ctx.predict_setup(th)
    assert rc == abi.OK, rc
    return model_of(th, *ctx.pred_state()) if kind == 1 else None


def check(what, got, ref, scale, keys=R.KEYS, tol=TOL):
    e = R.scaled_errors(got, ref, scale, keys)
    print(f"{what}: scaled error {e:.2e} (bar {tol:.1e})")
    for k in keys:
        assert np.all(np.isfinite(got[k])), (what, k)
    assert e < tol, (what, e)
    return e


def ordered(what, got, scale):
    """V_j <= VT_j <= V and V_j >= 0 up to the bar"""
    V, slack = got["cov_all"], 2 * TOL * scale["cov_all"]
    first, total = got["cov_first"], V - got["cov_rest"]
    assert V >= -slack, what
    assert np.all(first >= -slack) and np.all(first <= total + slack) and np.all(total <= V + slack), (what, V, first, total)


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in R.KEYS)


@pytest.fixture(scope="module")
def second_ctx():
    ctx = abi.Context(0)
    yield ctx
    ctx.close()


# ---------------------------------------------------------------------------------------------------- 1. shapes
@pytest.mark.parametrize("N", NS)
def test_shapes(gpu_ctx, N):
    """ragged tiles in both directions, one point, d = 8 and 16 < d = 17 (the rolled kernel), nreg up to 52"""
    worst = 0.0
    for n, d, o in shape_cases():
        if n != N:
            continue
        X, y = data(N, d)
        lo, hi = R.boxes(X)["design"]
        m = fit(gpu_ctx, o, X, y, thetas(d))
        got = gpu_ctx.sens_cov(lo, hi)
        ref, scale = R.covariances(R.NP, X, m, m, lo, hi)
        worst = max(worst, check(f"N {N} d {d} order {o}", got, ref, scale))
        assert got["e0"][0] == got["e0"][1]
        ordered(f"N {N} d {d} order {o}", got, scale)
        if d == 1:
            slack = 2 * TOL * scale["cov_all"]
            assert abs(got["cov_first"][0] - got["cov_all"]) <= slack and abs(got["cov_rest"][0]) <= slack
    print(f"N {N}: worst scaled error {worst:.2e}")


# ---------------------------------------------------------------------------------------------------- 2. boxes, two contexts
@pytest.mark.parametrize("name,N,d,order,box,cross", extra_cases())
def test_boxes_and_two_contexts(gpu_ctx, second_ctx, name, N, d, order, box, cross):
    X, y = data(N, d)
    lo, hi = R.boxes(X)[box]
    ma = fit(gpu_ctx, order, X, y, thetas(d))
    mb, other = ma, None
    if cross:
        mb, other = fit(second_ctx, order, X, data(N, d, 1)[1], thetas(d, 0.2)), second_ctx
    got = gpu_ctx.sens_cov(lo, hi, other)
    ref, scale = R.covariances(R.NP, X, ma, mb, lo, hi)
    check(f"{name} order {order}", got, ref, scale)
    if cross:
        # the other way round: the same numbers to the bar, e0 swapped
        back = second_ctx.sens_cov(lo, hi, gpu_ctx)
        back["e0"] = back["e0"][::-1]
        check(f"{name} order {order}, contexts swapped", back, ref, scale)
    else:
        ordered(name, got, scale)


def test_erfc_form_separates(gpu_ctx):
    """Order 0 with the training values shifted so that beta_0 = 0 to rounding, on the disjoint box: every value is then made of
    kernel integrals six length scales and more from the design, nothing of the polynomial's size hides them.  On the CPU the
    plain erf difference misses the bar on this case while the erfc form meets it (asserted here on the device's own beta
    and gamma), so a device that took the plain difference fails."""
    N, d = 130, 3
    X, y = data(N, d)
    th = thetas(d)
    gpu_ctx.set_model(1, 0, X, y)
    beta, rc = gpu_ctx.predict_setup(th)
    assert rc == abi.OK
    m = fit(gpu_ctx, 0, X, y - beta[0], th)
    assert abs(m["beta"][0]) < 1e-9
    lo, hi = R.boxes(X)["disjoint"]
    ref, scale = R.covariances(R.NP, X, m, m, lo, hi)
    naive, _ = R.covariances(R.NPNaive, X, m, m, lo, hi)
    e_naive = R.scaled_errors(naive, ref, scale)
    print(f"plain erf difference against the erfc form on the CPU: {e_naive:.2e} (bar {TOL:.1e})")
    assert e_naive > 100 * TOL
    check("disjoint box, beta_0 = 0", gpu_ctx.sens_cov(lo, hi), ref, scale)
    grid = main_grid(X, lo, hi)
    mref, mscale = R.main_effects(R.NP, X, m, lo, hi, grid)
    e0, main = gpu_ctx.sens_main(lo, hi, grid)
    check("disjoint box, beta_0 = 0, main effects", dict(e0=e0, main=main), mref, mscale, keys=("e0", "main"))


def test_n1000_d8_against_numpy(gpu_ctx):
    N, d, order = 1000, 8, 1
    X, y = data(N, d)
    lo, hi = R.boxes(X)["design"]
    m = fit(gpu_ctx, order, X, y, thetas(d))
    got = gpu_ctx.sens_cov(lo, hi)
    ref, scale = R.covariances(R.NP, X, m, m, lo, hi)
    check("N 1000 d 8", got, ref, scale)
    ordered("N 1000 d 8", got, scale)


# ---------------------------------------------------------------------------------------------------- 3. known answers
def test_exactly_linear_data(gpu_ctx):
    """y = 2 + 3 x_0 - x_1 at order 1: the fit is the plane (gamma = 0 to the rounding of the solve), V_j = beta_j^2 w_j^2 / 12 and
    VT_j = V_j.  Against sensref at TOL; against the formula at the parity bar (gamma is zero only to the solve's rounding)."""
    X, y, th, lo, hi = linear_case()
    m = fit(gpu_ctx, 1, X, y, th)
    assert np.allclose(m["beta"], [2.0, 3.0, -1.0], rtol=0, atol=RTOL)
    got = gpu_ctx.sens_cov(lo, hi)
    ref, scale = R.covariances(R.NP, X, m, m, lo, hi)
    check("linear data", got, ref, scale)
    want = m["beta"][1:] ** 2 * (hi - lo) ** 2 / 12
    assert np.all(np.abs(got["cov_first"] - want) < RTOL * scale["cov_first"])
    assert np.all(np.abs(got["cov_all"] - got["cov_rest"] - want) < RTOL * scale["cov_rest"])
    assert abs(got["cov_all"] - want.sum()) < RTOL * scale["cov_all"]
    assert abs(got["e0"][0] - (2.0 + 3.0 * 0.5 - 0.45)) < RTOL * scale["e0"][0]


def test_unused_coordinate(gpu_ctx):
    """the data ignore x_2 and its length scale is long (e^3): its indices vanish against the variance"""
    X, y, th = unused_case()
    m = fit(gpu_ctx, 1, X, y, th)
    lo, hi = R.boxes(X)["design"]
    got = gpu_ctx.sens_cov(lo, hi)
    ref, scale = R.covariances(R.NP, X, m, m, lo, hi)
    check("unused coordinate", got, ref, scale)
    V = got["cov_all"]
    print("indices:", got["cov_first"] / V, (V - got["cov_rest"]) / V)
    assert got["cov_first"][2] < 1e-3 * V and V - got["cov_rest"][2] < 1e-3 * V
    assert got["cov_first"][0] > 0.05 * V and got["cov_first"][1] > 0.05 * V


def test_main_effects(gpu_ctx):
    """the curves at the ends of the box, at a design point and in between; their E0 is gpemu_sens_cov's"""
    for N, d, order in MAIN_CASES:
        X, y = data(N, d)
        m = fit(gpu_ctx, order, X, y, thetas(d))
        for box in ("design", "narrow"):
            lo, hi = R.boxes(X)[box]
            grid = main_grid(X, lo, hi)
            e0, main = gpu_ctx.sens_main(lo, hi, grid)
            ref, scale = R.main_effects(R.NP, X, m, lo, hi, grid)
            check(f"main effects N {N} d {d} order {order} {box}", dict(e0=e0, main=main), ref, scale, keys=("e0", "main"))
            assert e0 == gpu_ctx.sens_cov(lo, hi)["e0"][0]
            again = gpu_ctx.sens_main(lo, hi, grid)
            assert again[0] == e0 and np.array_equal(again[1], main)
    e0, one = gpu_ctx.sens_main(lo, hi, grid[:, :1])                       # ngrid = 1
    assert np.array_equal(one[:, 0], main[:, 0])


# ---------------------------------------------------------------------------------------------------- 4. Monte Carlo
def test_monte_carlo_cross_check(gpu_ctx):
    """A wrong definition, not rounding: 2^16 seeded points through gpemu_predict_mean (lengths 0.6 on the unit cube: no k value
    comes within five orders of the 1e-10 clamp).  E0 and V from the plain sample, V_j from the pick-freeze products, VT_j from
    Jansen's squared differences, a main effect from the sample with x_j fixed; each within five of its own standard errors."""
    N, d, n = 200, 3, 1 << 16
    X, y = data(N, d)
    th = thetas(d)
    fit(gpu_ctx, 1, X, y, th)
    lo, hi = R.boxes(X)["design"]
    got = gpu_ctx.sens_cov(lo, hi)
    e0, V = got["e0"][0], got["cov_all"]
    rng = np.random.default_rng(20261019)
    A, B = (lo + (hi - lo) * rng.random((n, d)) for _ in range(2))
    fA = gpu_ctx.predict_mean(A)

    def within(what, sample, value):
        est, se = sample.mean(), sample.std(ddof=1) / np.sqrt(n)
        print(f"{what}: closed form {value:.6f}, sample {est:.6f} +- {se:.6f}")
        assert abs(est - value) < 5 * se, what

    within("E0", fA, e0)
    within("V", (fA - e0) ** 2, V)
    for j in range(d):
        frozen = B.copy()
        frozen[:, j] = A[:, j]                                              # shares x_j with A
        within(f"V_{j}", (fA - e0) * (gpu_ctx.predict_mean(frozen) - e0), got["cov_first"][j])
        moved = A.copy()
        moved[:, j] = B[:, j]                                               # differs from A in x_j alone
        within(f"VT_{j}", 0.5 * (fA - gpu_ctx.predict_mean(moved)) ** 2, V - got["cov_rest"][j])
    g = lo + 0.3 * (hi - lo)
    _, main = gpu_ctx.sens_main(lo, hi, g.reshape(d, 1))
    for j in range(d):
        fixed = A.copy()
        fixed[:, j] = g[j]
        within(f"E[m | x_{j} = {g[j]:.3f}]", gpu_ctx.predict_mean(fixed), main[j, 0])


# ---------------------------------------------------------------------------------------------------- 5. bits, bystanders
def _dev_call(ctx, lo, hi, other=None):
    d = ctx.d
    buf = ctx.dev_alloc((3 + 2 * d) * 8)
    try:
        ctx.sens_cov_dev(lo, hi, buf, other)
        o = ctx.download(buf, (3 + 2 * d,))
    finally:
        ctx.dev_free(buf)
    return dict(e0=o[:2], cov_all=o[2], cov_first=o[3:3 + d], cov_rest=o[3 + d:])


def test_same_bits_and_bystanders(gpu_ctx, second_ctx):
    N, d, order = 200, 3, 1
    X, y = data(N, d)
    th = thetas(d)
    fit(gpu_ctx, order, X, y, th)
    fit(second_ctx, order, X, data(N, d, 1)[1], thetas(d, 0.2))
    lo, hi = R.boxes(X)["narrow"]
    Xq = X[:9] + 0.01
    group = (np.arange(N) % 5).astype(np.int32)
    before = (gpu_ctx.predict(Xq), gpu_ctx.loo(), gpu_ctx.lgo(group))
    for other in (None, second_ctx):
        a = gpu_ctx.sens_cov(lo, hi, other)
        assert same_bits(a, gpu_ctx.sens_cov(lo, hi, other))
        assert same_bits(a, _dev_call(gpu_ctx, lo, hi, other))
        gpu_ctx.sens_release()
        assert same_bits(a, gpu_ctx.sens_cov(lo, hi, other))
    # a pending prediction batch stays collectable across both entries
    want = gpu_ctx.predict(Xq)
    gpu_ctx.predict_enqueue(Xq)
    gpu_ctx.sens_cov(lo, hi, second_ctx)
    gpu_ctx.sens_main(lo, hi, np.stack([lo, hi], axis=1))
    got = gpu_ctx.predict_collect()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # nothing another entry reads has changed
    after = (gpu_ctx.predict(Xq), gpu_ctx.loo(), gpu_ctx.lgo(group))
    assert all(np.array_equal(p, q) for p, q in zip(before[0] + before[1], after[0] + after[1]))
    assert all(np.array_equal(before[2][k], after[2][k], equal_nan=True) for k in ("mean", "var", "werr", "maha", "logdet", "logpdf"))
    # profiling class: three launches for the covariances, two for the curves
    gpu_ctx.prof_begin(abi.PROF_SENS)
    gpu_ctx.sens_cov(lo, hi)
    p = gpu_ctx.prof_end()
    print("PROF_SENS:", p)
    T = ((N + 63) // 64) ** 2 * (2 * d + 1)
    assert p["n"] == 3 and p["ms"] > 0
    assert p["flops"] == 88.0 * N * d + N * N * (19.0 * d + 2.0) + T and p["bytes"] == 8.0 * (11 * N * d + 2 * T)
    gpu_ctx.prof_begin(abi.PROF_SENS)
    gpu_ctx.sens_main(lo, hi, np.stack([lo, hi], axis=1))
    assert gpu_ctx.prof_end()["n"] == 2


def test_setup_by_batch_same_bits():
    """components set up by gpemu_predict_setup_batch against contexts set up alone, the cross case included"""
    N, d, order = 130, 3, 1
    X, y = data(N, d)
    ys, ths = [y, data(N, d, 1)[1]], [thetas(d), thetas(d, 0.2)]
    lo, hi = R.boxes(X)["design"]
    ctxs, alone = [abi.Context(0) for _ in ys], [abi.Context(0) for _ in ys]
    try:
        for c, yc in zip(ctxs, ys):
            c.set_model(1, order, X, yc)
        _, _, status, rc = abi.predict_setup_batch(ctxs, np.array(ths))
        assert rc == abi.OK and not status.any()
        for c, yc, tc in zip(alone, ys, ths):
            fit(c, order, X, yc, tc)
        for i in (0, 1):
            assert same_bits(ctxs[i].sens_cov(lo, hi), alone[i].sens_cov(lo, hi))
        assert same_bits(ctxs[0].sens_cov(lo, hi, ctxs[1]), alone[0].sens_cov(lo, hi, alone[1]))
        assert same_bits(ctxs[1].sens_cov(lo, hi, ctxs[0]), alone[1].sens_cov(lo, hi, alone[0]))
    finally:
        for c in ctxs + alone:
            c.close()


# ---------------------------------------------------------------------------------------------------- 6. errors
def _cov_rc(a, b, lo, hi, e0=True, ca=True, cf=True, cr=True):
    d = max(a.d, 1)
    bufs = [np.empty(2), np.empty(1), np.empty(d), np.empty(d)]
    ptr = [abi._p(x) if on else None for x, on in zip(bufs, (e0, ca, cf, cr))]
    lo = None if lo is None else abi._a(lo)
    hi = None if hi is None else abi._a(hi)
    return a.L.gpemu_sens_cov(a.h, b.h if b is not None else None, None if lo is None else abi._p(lo), None if hi is None else abi._p(hi), *ptr)


def _main_rc(a, lo, hi, ngrid, grid=True, e0=True, main=True):
    d = max(a.d, 1)
    g, e, m = np.full(d * max(ngrid, 1), 0.5), np.empty(1), np.empty(d * max(ngrid, 1))
    lo, hi = abi._a(lo), abi._a(hi)
    return a.L.gpemu_sens_main(a.h, abi._p(lo), abi._p(hi), ngrid, abi._p(g) if grid else None, abi._p(e) if e0 else None,
                               abi._p(m) if main else None)


def test_errors(gpu_ctx, second_ctx):
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
        for kw in (dict(e0=False), dict(ca=False), dict(cf=False), dict(cr=False)):
            assert _cov_rc(fresh, fresh, lo, hi, **kw) == abi.ERR_ARG
        assert _cov_rc(fresh, None, lo, hi) == abi.ERR_ARG
        assert _cov_rc(fresh, fresh, None, hi) == abi.ERR_ARG and _cov_rc(fresh, fresh, lo, None) == abi.ERR_ARG
        assert L.gpemu_sens_cov(None, None, None, None, None, None, None, None) == abi.ERR_ARG
        assert L.gpemu_sens_cov_dev(fresh.h, fresh.h, abi._p(lo), abi._p(hi), None) == abi.ERR_ARG
        assert L.gpemu_sens_cov_dev(None, fresh.h, abi._p(lo), abi._p(hi), None) == abi.ERR_ARG
        for kw in (dict(grid=False), dict(e0=False), dict(main=False)):
            assert _main_rc(fresh, lo, hi, 3, **kw) == abi.ERR_ARG
        assert _main_rc(fresh, lo, hi, 0) == abi.ERR_ARG and _main_rc(gpu_ctx, lo, hi, 0) == abi.ERR_ARG
        assert L.gpemu_sens_release(None) == abi.ERR_ARG
        # no prediction set-up on either context
        assert _cov_rc(fresh, fresh, lo, hi) == abi.ERR_STATE
        assert _cov_rc(gpu_ctx, fresh, lo, hi) == abi.ERR_STATE and _cov_rc(fresh, gpu_ctx, lo, hi) == abi.ERR_STATE
        assert _main_rc(fresh, lo, hi, 3) == abi.ERR_STATE
        with pytest.raises(abi.GpemuError) as ei:
            fresh.sens_cov(lo, hi)
        assert ei.value.code == abi.ERR_STATE
        assert fresh.L.gpemu_sens_release(fresh.h) == abi.OK            # nothing to give back is no error
    finally:
        fresh.close()
    assert _cov_rc(gpu_ctx, gpu_ctx, lo, hi) == abi.OK and _main_rc(gpu_ctx, lo, hi, 3) == abi.OK
    # bounds
    for l in range(d):
        for bad in (np.nan, np.inf, -np.inf):
            b = lo.copy(); b[l] = bad
            assert _cov_rc(gpu_ctx, gpu_ctx, b, hi) == abi.ERR_ARG and _main_rc(gpu_ctx, b, hi, 3) == abi.ERR_ARG
            b = hi.copy(); b[l] = bad
            assert _cov_rc(gpu_ctx, gpu_ctx, lo, b) == abi.ERR_ARG
        b = hi.copy(); b[l] = lo[l]
        assert _cov_rc(gpu_ctx, gpu_ctx, lo, b) == abi.ERR_ARG                  # hi = lo
        b[l] = lo[l] - 0.1
        assert _cov_rc(gpu_ctx, gpu_ctx, lo, b) == abi.ERR_ARG                  # hi < lo
    # the other context: another N, another d, another coordinate, another regression order, a Matern model
    fit(second_ctx, order, X[:-1], y[:-1], th)
    assert _cov_rc(gpu_ctx, second_ctx, lo, hi) == abi.ERR_ARG
    fit(second_ctx, order, X[:, :2], y, thetas(2))
    assert _cov_rc(gpu_ctx, second_ctx, lo, hi) == abi.ERR_ARG
    X2 = X.copy(); X2[17, 1] = np.nextafter(X2[17, 1], 2.0)
    fit(second_ctx, order, X2, y, th)
    assert _cov_rc(gpu_ctx, second_ctx, lo, hi) == abi.ERR_ARG and _cov_rc(second_ctx, gpu_ctx, lo, hi) == abi.ERR_ARG
    assert "design" in gpu_ctx.L.gpemu_last_error(gpu_ctx.h).decode()
    fit(second_ctx, 2, X, y, th)
    assert _cov_rc(gpu_ctx, second_ctx, lo, hi) == abi.ERR_ARG
    assert "order" in gpu_ctx.L.gpemu_last_error(gpu_ctx.h).decode()
    fit(second_ctx, order, X, y, synth.default_thetas(3, d), kind=3)
    assert _cov_rc(gpu_ctx, second_ctx, lo, hi) == abi.ERR_ARG
    assert "power-exponential covariance only" in gpu_ctx.L.gpemu_last_error(gpu_ctx.h).decode()
    assert _cov_rc(second_ctx, second_ctx, lo, hi) == abi.ERR_ARG and _main_rc(second_ctx, lo, hi, 3) == abi.ERR_ARG
    assert "power-exponential covariance only" in second_ctx.L.gpemu_last_error(second_ctx.h).decode()
    # contexts on different devices: only where there are two
    if L.gpemu_device_count() > 1:
        far = abi.Context(1)
        try:
            fit(far, order, X, y, th)
            assert _cov_rc(gpu_ctx, far, lo, hi) == abi.ERR_ARG
        finally:
            far.close()
    # a refused call has left everything as it was; a new training vector ends the set-up
    fit(second_ctx, order, X, y, th)
    assert _cov_rc(gpu_ctx, second_ctx, lo, hi) == abi.OK and _cov_rc(gpu_ctx, gpu_ctx, lo, hi) == abi.OK
    gpu_ctx.set_training(y + 1.0)
    assert _cov_rc(gpu_ctx, gpu_ctx, lo, hi) == abi.ERR_STATE
