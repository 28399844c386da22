"""The closed-form sensitivity analysis under Gaussian and mixed input measures (gpemu_sens_set_measure, include/gpemu.h,
DESIGN.md 4.17) through the public entries, against tests/sensmeasureref.py (numpy fp64; test_sensmeasureref.py pins it
against mpmath and against Gauss-Hermite / Gauss-Legendre quadrature of the functions themselves).

What is compared, as in test_gpu_sens.py, test_gpu_sens_post.py and test_gpu_sens_pairs.py, whose inputs (`data`, `thetas`,
`fit`) this file uses: beta and gamma come from the device's own prediction state, P, G and Q from
gpemu_test_sens_post_state; everything downstream of them is the reference's own.  Errors are relative to the SCALE the
reference returns beside every value.

Shapes.  N in {1, 63, 64, 65, 130, 200} times d in {1, 2, 3, 8, 9, 17} (d = 8 / 9 straddles the pair sweep's second launch,
d = 17 takes the rolled sweep), every regression order 0 .. 3 that fits under N points.  Measures per shape: every
coordinate Gaussian (mean at the centre of the design, sd = 0.3 of its range); alternating kinds (coordinate 0 uniform on the
design's range, 1 Gaussian, ...; d >= 2); at d = 9 and 17 also the first block of 8 coordinates uniform and the rest
Gaussian, so that one 8 x 8 block of the pair sweep is pure and the off-diagonal one mixed.  Entries per shape and measure:
gpemu_sens_cov, _main, _pairs, _joint on a fit of test_gpu_sens.py's data, gpemu_sens_post, _main_var, _pairs_post on a fit of
test_gpu_sens_post.py's; the _dev forms return the host forms' bits, and so does a second call.

The bars.  NP_VS_MP is the largest scaled error of the numpy reference against mpmath at 50 digits over exactly the cases of
this file (`plug_cases()` with beta and gamma from a LAPACK fit, `post_cases()` with P, G, Q from a numpy fit), measured on
the CPU by `python tests/sensmeasureref.py --measure`; the device gets the project's FACTOR = 8 times that (another
summation order, an exp a few ulp from libm's), one constant for the plug-in quantities (cov, main, cov_pair, joint, inter)
and one for the S quantities (s_*, the band):
  measured NP_VS_MP_PLUG = 5.3e-12 -> TOL   = 4.3e-11   (worst: the far measure with beta_0 = 0; the shapes stay below 6e-13)
  measured NP_VS_MP_POST = 8.1e-16 -> TOL_S = 6.5e-15   (worst: one point, d = 17, first block uniform; the far measure 6.3e-16)
Two device results compared with each other get twice the bar.

A finding, the all-Gaussian WIDE measure (sd = 100 ranges).  There the numpy reference itself is far from mpmath: 2.7e-10 at
order 0 and 2.3e-5 at order 2 (`--measure` prints them apart from the figure above).  The references assemble every value in
RAW form, E[m_u^a m_u^b] - E0a E0b, and their SCALE takes each part after it has been summed.  Under N(mu, (100 w)^2) the
quadratic q_l has E q_l of 1e4 and a second moment of 1e8 to 1e9, the parts of `pp` are of that size and cancel among
themselves before the scale sees them (order 2); and at order 0, where sum_i gamma_i = 0 and I_l(i) is the same for every
point to 1e-4, F = A sum_i gamma_i prod_l I_l(i) is itself a cancelled sum, and so is the scale of `inter`.  The device centres
before it forms a second moment and is the more accurate of the two, but it can be HELD only to what the reference resolves:
these two cases get FACTOR times their own measured figure, NP_VS_MP_WIDE, every other case the bar above (the mixed wide
cases, 5.1e-14 and 8.4e-12, need no figure of their own).  Device against numpy on these two: 1.5e-10 and 8.8e-6; on every other case the device stays below 8.5e-12 (plug-in) and 8e-16 (S)."""
import numpy as np
import pytest

import sensref as R
import sensmeasureref as M
import senspairref as SPR
import senspostref as SP
import test_gpu_sens as TS
import test_gpu_sens_post as TP
from madaiemulator_amd import abi

NP_VS_MP_PLUG = 5.3e-12
NP_VS_MP_POST = 8.1e-16
NP_VS_MP_WIDE = {"wide-gauss-o0": 2.7e-10, "wide-gauss-o2": 2.3e-5}
FACTOR = 8
TOL = FACTOR * NP_VS_MP_PLUG
TOL_S = FACTOR * NP_VS_MP_POST


def plug_tol(name):
    return FACTOR * max(NP_VS_MP_PLUG, NP_VS_MP_WIDE.get(name, 0.0))

pytestmark = pytest.mark.gpu

NS = [1, 63, 64, 65, 130, 200]
DS = [1, 2, 3, 8, 9, 17]
ORDERS = [0, 1, 2, 3]
PLUG_KEYS = R.KEYS
SPECIAL = ("centred", "narrow", "far", "wide")


# ---------------------------------------------------------------------------------------------------- inputs
def shape_cases():
    return [(N, d, o) for N in NS for d in DS for o in ORDERS if 1 + o * d <= N]


def kinds(name, d):
    if name == "gauss":
        return np.ones(d, dtype=np.int32)
    if name == "mixed":
        return (np.arange(d) % 2).astype(np.int32)
    assert name == "block" and d > 8
    return (np.arange(d) >= 8).astype(np.int32)


def measures_for(d):
    return ["gauss"] + (["mixed"] if d >= 2 else []) + (["block"] if d in (9, 17) else [])


def measure_of(kind, X, special="centred"):
    """-> (lo, hi) of the entries: the design's range on a uniform coordinate; on a Gaussian one the mean and the sd --
    centred: the centre of the design and 0.3 of its range; narrow: sd 0.02 of the range; wide: sd 100 ranges; far: the mean
    of the first Gaussian coordinate six of the default length scales (6 * 0.6) above the largest design value, sd 0.1 of the range"""
    lo, hi = R.boxes(X)["design"]
    mid, w = (lo + hi) / 2, hi - lo
    sd = dict(centred=0.3, narrow=0.02, far=0.1, wide=100.0)[special] * w
    mean = mid.copy()
    g = np.asarray(kind) == M.GAUSS
    if special == "far":
        first = int(np.flatnonzero(g)[0])
        mean[first] = hi[first] + 3.6
    return np.where(g, mean, lo), np.where(g, sd, hi)


def span(kind, lo, hi):
    """where curves and surfaces are looked at: the box, or mean -+ 2 sd on a Gaussian coordinate"""
    g = np.asarray(kind) == M.GAUSS
    return np.where(g, lo - 2 * hi, lo), np.where(g, lo + 2 * hi, hi)


def grids(kind, X, lo, hi, j, k):
    glo, ghi = span(kind, lo, hi)
    return TS.main_grid(X, glo, ghi), TP.band_grid(X, glo, ghi, 3), TSP_points(X, glo, ghi, j, k)


def TSP_points(X, glo, ghi, j, k):
    t, u = np.array([0.0, 1.0, 0.5, 0.3]), np.array([0.0, 0.0, 0.5, 0.9])
    return (np.append(glo[j] + t * (ghi[j] - glo[j]), X[len(X) // 2, j]), np.append(glo[k] + u * (ghi[k] - glo[k]), X[len(X) // 2, k]))


def plug_cases():
    """every (name, X, [(y, th), ...one or two...], order, kind, lo, hi, zero_beta0) of the plug-in quantities"""
    out = []
    for N, d, o in shape_cases():
        X, y = TS.data(N, d)
        for mn in measures_for(d):
            kind = kinds(mn, d)
            out.append((f"N{N}-d{d}-o{o}-{mn}", X, [(y, TS.thetas(d))], o, kind) + measure_of(kind, X) + (False,))
    X, y = TS.data(130, 3)
    for sp in SPECIAL:
        for mn in ("gauss", "mixed"):
            kind = kinds(mn, 3)
            for o in (0, 2):
                out.append((f"{sp}-{mn}-o{o}", X, [(y, TS.thetas(3))], o, kind) + measure_of(kind, X, sp) + (False,))
                if sp in ("centred", "narrow"):
                    out.append((f"{sp}-{mn}-cross-o{o}", X, [(y, TS.thetas(3)), (TS.data(130, 3, 1)[1], TS.thetas(3, 0.2))], o, kind)
                               + measure_of(kind, X, sp) + (False,))
    kind = kinds("gauss", 3)
    out.append(("far-gauss-beta0-zero", X, [(y, TS.thetas(3))], 0, kind) + measure_of(kind, X, "far") + (True,))
    return out


def post_cases():
    """every (name, X, y, th, order, kind, lo, hi) of the S quantities"""
    out = []
    for N, d, o in shape_cases():
        X, y = TP.data(N, d)
        for mn in measures_for(d):
            kind = kinds(mn, d)
            out.append((f"N{N}-d{d}-o{o}-{mn}", X, y, TP.thetas(d), o, kind) + measure_of(kind, X))
    X, y = TP.data(130, 3)
    for sp in SPECIAL:
        for mn in ("gauss", "mixed"):
            kind = kinds(mn, 3)
            for o in (0, 2):
                out.append((f"{sp}-{mn}-o{o}", X, y, TP.thetas(3), o, kind) + measure_of(kind, X, sp))
    return out


def plug_reference(B, kind, X, ma, mb, lo, hi):
    """-> (values, scales, keys) of everything the plug-in entries return for the case: cov, main, cov_pair, joint"""
    d = X.shape[1]
    j, k = 0, d - 1
    grid, _, (xj, xk) = grids(kind, X, lo, hi, j, k)
    val, scale = M.covariances(kind, B, X, ma, mb, lo, hi)
    keys = list(PLUG_KEYS)
    mv, ms = M.main_effects(kind, B, X, ma, lo, hi, grid)
    val.update(main=mv["main"], e0_main=mv["e0"])
    scale.update(main=ms["main"], e0_main=ms["e0"])
    keys += ["main", "e0_main"]
    if d >= 2:
        pv, ps = M.pair_covariances(kind, B, X, ma, mb, lo, hi)
        jv, js = M.joint_surface(kind, B, X, ma, lo, hi, j, k, xj, xk)
        val.update(cov_pair=pv["cov_pair"], joint=jv["joint"], inter=jv["inter"], e0_joint=jv["e0"])
        scale.update(cov_pair=ps["cov_pair"], joint=js["joint"], inter=js["inter"], e0_joint=js["e0"])
        keys += ["cov_pair", "joint", "inter", "e0_joint"]
    return val, scale, tuple(keys)


def post_reference(B, kind, X, m, P, G, Q, beta, gamma, lo, hi):
    d = X.shape[1]
    _, bgrid, _ = grids(kind, X, lo, hi, 0, d - 1)
    val, scale = M.post(kind, B, X, m, P, G, Q, lo, hi)
    keys = list(SP.KEYS)
    bv, bs = M.band(kind, B, X, m, P, G, Q, beta, gamma, lo, hi, bgrid)
    val.update(var=bv["var"], var_e0=bv["var_e0"], band_main=bv["main"])
    scale.update(var=bs["var"], var_e0=bs["var_e0"], band_main=bs["main"])
    keys += ["var", "var_e0", "band_main"]
    if d >= 2:
        pv, ps = M.pair_post(kind, B, X, m, P, G, Q, lo, hi)
        val["s_pair"], scale["s_pair"] = pv["s_pair"], ps["s_pair"]
        keys.append("s_pair")
    return val, scale, tuple(keys)


def _measure_plug(case):
    import meanref
    name, X, fits, o, kind, lo, hi, zero = case
    ms = []
    for y, th in fits:
        beta, gamma = meanref.trained(1, o, X, y, th)
        if zero:
            beta, gamma = meanref.trained(1, o, X, y - beta[0], th)
        ms.append(TS.model_of(th, beta, gamma))
    val, scale, keys = plug_reference(R.NP, kind, X, ms[0], ms[-1], lo, hi)
    mp, _, _ = plug_reference(R.MP(), kind, X, ms[0], ms[-1], lo, hi)
    return name, M.scaled_errors(val, mp, scale, keys)


def _measure_post(case):
    name, X, y, th, o, kind, lo, hi = case
    m = TP.model_of(th)
    P, G, Q, beta, gamma, _, _ = SP.fit_state(X, y, o, m["A"], m["s"], TP.NUGGET)
    val, scale, keys = post_reference(R.NP, kind, X, m, P, G, Q, beta, gamma, lo, hi)
    mp, _, _ = post_reference(R.MP(), kind, X, m, P, G, Q, beta, gamma, lo, hi)
    return name, M.scaled_errors(val, mp, scale, keys)


def measure_np_against_mp():
    """the figures NP_VS_MP_PLUG and NP_VS_MP_POST are set from (CPU; mpmath over every case: tens of minutes)"""
    import multiprocessing as mpc
    import sys
    from oracle import oracle as O
    O.build()
    for what, fn, cases in (("plug-in", _measure_plug, plug_cases()), ("S", _measure_post, post_cases())):
        cases = sorted(cases, key=lambda c: -c[1].size * len(c[1]))
        if "--only" in sys.argv:                     # names that start with the given prefixes
            cases = [c for c in cases if c[0].startswith(tuple(sys.argv[sys.argv.index("--only") + 1].split(",")))]
        worst = ("", 0.0)
        with mpc.Pool(min(16, mpc.cpu_count())) as pool:
            for name, e in pool.imap_unordered(fn, cases):
                print(f"{what} {name}: {e:.3e}", flush=True)
                if what == "plug-in" and name in NP_VS_MP_WIDE:          # (the finding of the docstring: a figure of its own)
                    print(f"{what}: {name} apart: {e:.3e}", flush=True)
                elif e > worst[1]:
                    worst = (name, e)
        print(f"{what}: largest scaled error of numpy against mpmath over {len(cases)} cases: {worst[1]:.3e} ({worst[0]})", flush=True)


# ---------------------------------------------------------------------------------------------------- helpers
def check(what, got, ref, scale, keys, tol):
    e = M.scaled_errors(got, ref, scale, keys)
    print(f"{what}: scaled error {e:.2e} (bar {tol:.1e})")
    for k in keys:
        assert np.all(np.isfinite(got[k])), (what, k)
    assert e < tol, (what, e)
    return e


def _dev(ctx, n, call):
    buf = ctx.dev_alloc(n * 8)
    try:
        call(buf)
        return ctx.download(buf, (n,))
    finally:
        ctx.dev_free(buf)


def plug_entries(ctx, kind, X, lo, hi, other=None, dev=True):
    """every plug-in entry of the context under its stored measure -> dict as plug_reference's; with dev, the _dev forms and a
    second call are held to the same bits"""
    d = X.shape[1]
    j, k = 0, d - 1
    grid, _, (xj, xk) = grids(kind, X, lo, hi, j, k)
    got = ctx.sens_cov(lo, hi, other)
    got["e0_main"], got["main"] = ctx.sens_main(lo, hi, grid)
    if d >= 2:
        got["cov_pair"] = ctx.sens_pairs(lo, hi, other)
        got["e0_joint"], got["joint"], got["inter"] = ctx.sens_joint(lo, hi, j, k, xj, xk)
    if dev:
        o = _dev(ctx, 3 + 2 * d, lambda buf: ctx.sens_cov_dev(lo, hi, buf, other))
        assert np.array_equal(o, np.concatenate([got["e0"], [got["cov_all"]], got["cov_first"], got["cov_rest"]]))
        again = ctx.sens_cov(lo, hi, other)
        assert all(np.array_equal(again[key], got[key]) for key in PLUG_KEYS)
        assert np.array_equal(ctx.sens_main(lo, hi, grid)[1], got["main"])
        if d >= 2:
            assert np.array_equal(_dev(ctx, d * (d - 1) // 2, lambda buf: ctx.sens_pairs_dev(lo, hi, buf, other)), got["cov_pair"])
            assert np.array_equal(ctx.sens_pairs(lo, hi, other), got["cov_pair"])
            again = ctx.sens_joint(lo, hi, j, k, xj, xk)
            assert np.array_equal(again[1], got["joint"]) and np.array_equal(again[2], got["inter"])
    return got


def post_entries(ctx, kind, X, lo, hi, dev=True):
    d = X.shape[1]
    _, bgrid, _ = grids(kind, X, lo, hi, 0, d - 1)
    got = ctx.sens_post(lo, hi)
    got["band_main"], got["var"], got["var_e0"] = ctx.sens_main_var(lo, hi, bgrid)
    if d >= 2:
        got["s_pair"] = ctx.sens_pairs_post(lo, hi)
    if dev:
        o = _dev(ctx, 2 + 2 * d, lambda buf: ctx.sens_post_dev(lo, hi, buf))
        assert np.array_equal(o, np.concatenate([[got["s_none"], got["s_all"]], got["s_first"], got["s_rest"]]))
        again = ctx.sens_post(lo, hi)
        assert all(np.array_equal(again[key], got[key]) for key in SP.KEYS)
        again = ctx.sens_main_var(lo, hi, bgrid)
        assert np.array_equal(again[1], got["var"]) and again[2] == got["var_e0"]
        if d >= 2:
            assert np.array_equal(_dev(ctx, d * (d - 1) // 2, lambda buf: ctx.sens_pairs_post_dev(lo, hi, buf)), got["s_pair"])
            assert np.array_equal(ctx.sens_pairs_post(lo, hi), got["s_pair"])
    return got


def plug_ordered(what, got, scale, TOL):
    """V_j <= VT_j <= V, V_j >= 0, V_jk - V_j - V_k >= 0 and V_jk <= V, up to the bar times the scales"""
    V, slack = got["cov_all"], 2 * TOL * scale["cov_all"]
    first, total = got["cov_first"], V - got["cov_rest"]
    assert V >= -slack, what
    assert np.all(first >= -slack) and np.all(first <= total + slack) and np.all(total <= V + slack), (what, V, first, total)
    d = len(first)
    for j, k in SPR.pairs(d):
        p = SPR.pair_index(j, k, d)
        sl = TOL * (scale["cov_pair"][p] + scale["cov_first"][j] + scale["cov_first"][k])
        assert got["cov_pair"][p] - first[j] - first[k] >= -sl, (what, j, k)
        assert got["cov_pair"][p] <= V + TOL * (scale["cov_pair"][p] + scale["cov_all"]), (what, j, k)


def post_ordered(what, got, scale):
    """s_none <= s_first[j] <= s_pair[j, k] <= s_all and s_none <= s_rest[j] <= s_all (Jensen), every S >= 0"""
    for key in ("s_first", "s_rest"):
        slack = TOL_S * (scale[key] + scale["s_all"] + scale["s_none"])
        assert np.all(got["s_none"] <= got[key] + slack) and np.all(got[key] <= got["s_all"] + slack), (what, key, got)
    assert got["s_none"] >= -TOL_S * scale["s_none"] and np.all(got["var"] >= -TOL_S * scale["var"])
    d = len(got["s_first"])
    for j, k in SPR.pairs(d):
        p = SPR.pair_index(j, k, d)
        slack = TOL_S * (scale["s_pair"][p] + scale["s_all"] + scale["s_first"][j] + scale["s_first"][k])
        assert max(got["s_first"][j], got["s_first"][k]) <= got["s_pair"][p] + slack and got["s_pair"][p] <= got["s_all"] + slack, (what, j, k)


def plug_case(ctx, what, kind, X, fits, o, lo, hi, zero=False, second=None):
    """fit, set the measure, run every plug-in entry, hold it to the reference"""
    y, th = fits[0]
    ma = TS.fit(ctx, o, X, y, th)
    if zero:
        ma = TS.fit(ctx, o, X, y - ma["beta"][0], th)
        assert abs(ma["beta"][0]) < 1e-9
    assert not ctx.sens_get_measure().any()                                 # gpemu_set_model starts the measure over
    ctx.sens_set_measure(kind)
    mb, other = ma, None
    if len(fits) > 1:
        mb, other = TS.fit(second, o, X, *fits[1]), second
        second.sens_set_measure(kind)
    got = plug_entries(ctx, kind, X, lo, hi, other)
    ref, scale, keys = plug_reference(R.NP, kind, X, ma, mb, lo, hi)
    tol = plug_tol(what)
    e = check(what, got, ref, scale, keys, tol)
    if other is None:
        plug_ordered(what, got, scale, tol)
    else:
        # the other way round: the same numbers to the bar, e0 swapped
        back = second.sens_cov(lo, hi, ctx)
        back["e0"] = back["e0"][::-1]
        back["cov_pair"] = second.sens_pairs(lo, hi, ctx)
        check(what + ", contexts swapped", back, ref, scale, PLUG_KEYS + ("cov_pair",), tol)
    return e


def post_case(ctx, what, kind, X, y, th, o, lo, hi):
    m = TP.fit(ctx, o, X, y, th)
    ctx.sens_set_measure(kind)
    got = post_entries(ctx, kind, X, lo, hi)
    P, G, Q = ctx.sens_post_state()
    beta, gamma = ctx.pred_state()
    ref, scale, keys = post_reference(R.NP, kind, X, m, P, G, Q, beta, gamma, lo, hi)
    e = check(what, got, ref, scale, keys, TOL_S)
    post_ordered(what, got, scale)
    # the band's curve is gpemu_sens_main's and Var*[E0] is s_none, to rounding
    _, bgrid, _ = grids(kind, X, lo, hi, 0, X.shape[1] - 1)
    assert np.all(np.abs(got["band_main"] - ctx.sens_main(lo, hi, bgrid)[1]) <= 2 * TOL_S * scale["band_main"])
    assert abs(got["var_e0"] - got["s_none"]) <= 2 * TOL_S * (scale["s_none"] + scale["var_e0"])
    return e


@pytest.fixture(scope="module")
def second_ctx():
    ctx = abi.Context(0)
    yield ctx
    ctx.close()


# ---------------------------------------------------------------------------------------------------- 1. shapes x measures
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("N", NS)
def test_plug_shapes(gpu_ctx, N, d):
    worst = 0.0
    for name, X, fits, o, kind, lo, hi, zero in plug_cases():
        if name.startswith(f"N{N}-d{d}-"):
            worst = max(worst, plug_case(gpu_ctx, name, kind, X, fits, o, lo, hi, zero))
    print(f"N {N} d {d}: worst scaled error {worst:.2e}")


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("N", NS)
def test_post_shapes(gpu_ctx, N, d):
    worst = 0.0
    for name, X, y, th, o, kind, lo, hi in post_cases():
        if name.startswith(f"N{N}-d{d}-"):
            worst = max(worst, post_case(gpu_ctx, name, kind, X, y, th, o, lo, hi))
    print(f"N {N} d {d}: worst scaled error {worst:.2e}")


# ---------------------------------------------------------------------------------------------------- 2. special measures
@pytest.mark.parametrize("special", SPECIAL)
def test_special_measures(gpu_ctx, second_ctx, special):
    """centred on the design, narrow (sd 0.02 ranges), far (six length scales outside, and with beta_0 = 0 so that nothing of
    the polynomial's size hides the kernel integrals), wide (sd 100 ranges); the two-context case both ways round"""
    for name, X, fits, o, kind, lo, hi, zero in plug_cases():
        if name.startswith(special + "-"):
            plug_case(gpu_ctx, name, kind, X, fits, o, lo, hi, zero, second_ctx)
    for name, X, y, th, o, kind, lo, hi in post_cases():
        if name.startswith(special + "-"):
            post_case(gpu_ctx, "S " + name, kind, X, y, th, o, lo, hi)


# ---------------------------------------------------------------------------------------------------- 3. unchanged behaviour
def _all_entries(ctx, kind, X, lo, hi):
    a, b = plug_entries(ctx, kind, X, lo, hi, dev=False), post_entries(ctx, kind, X, lo, hi, dev=False)
    return [a[key] for key in sorted(a)] + [b[key] for key in sorted(b)]


@pytest.mark.parametrize("N,d,order", [(130, 3, 2), (65, 9, 1), (64, 17, 0)])
def test_uniform_kinds_return_the_bits_of_a_context_without_a_measure(N, d, order):
    """a context that never called the setter, then all-uniform kinds (NULL and an array of zeros), then Gaussian and back: every
    entry returns the same bits; under the Gaussian measure in between it does not"""
    X, y = TP.data(N, d)
    lo, hi = R.boxes(X)["narrow"]
    kind0 = np.zeros(d, dtype=np.int32)
    ctx = abi.Context(0)
    try:
        TP.fit(ctx, order, X, y, TP.thetas(d))
        base = _all_entries(ctx, kind0, X, lo, hi)
        for setter in (lambda: ctx.sens_set_measure(kind0), lambda: ctx.sens_set_measure(None)):
            setter()
            assert all(np.array_equal(p, q) for p, q in zip(base, _all_entries(ctx, kind0, X, lo, hi)))
        ctx.sens_set_measure(kinds("gauss", d))
        assert np.array_equal(ctx.sens_get_measure(), kinds("gauss", d))
        assert ctx.sens_cov(lo, hi)["cov_all"] != base[0]
        ctx.sens_set_measure(kind0)
        assert all(np.array_equal(p, q) for p, q in zip(base, _all_entries(ctx, kind0, X, lo, hi)))
    finally:
        ctx.close()


def test_what_resets_the_measure_and_what_keeps_it(gpu_ctx):
    N, d, order = 65, 3, 1
    X, y = TS.data(N, d)
    th = TS.thetas(d)
    kind = kinds("mixed", d)
    lo, hi = measure_of(kind, X)
    TS.fit(gpu_ctx, order, X, y, th)
    gpu_ctx.sens_set_measure(kind)
    want = gpu_ctx.sens_cov(lo, hi)
    gpu_ctx.sens_release()
    assert np.array_equal(gpu_ctx.sens_get_measure(), kind)
    gpu_ctx.set_training(y + 1.0)
    assert np.array_equal(gpu_ctx.sens_get_measure(), kind)
    gpu_ctx.set_training(y)
    assert gpu_ctx.predict_setup(th)[1] == abi.OK
    assert np.array_equal(gpu_ctx.sens_get_measure(), kind)
    again = gpu_ctx.sens_cov(lo, hi)
    assert all(np.array_equal(want[k], again[k]) for k in PLUG_KEYS)
    _, _, status, rc = abi.predict_setup_batch([gpu_ctx], np.array([th]))
    assert rc == abi.OK and not status.any() and np.array_equal(gpu_ctx.sens_get_measure(), kind)
    gpu_ctx.set_model(1, order, X, y)
    assert not gpu_ctx.sens_get_measure().any()
    gpu_ctx.set_model(1, order, X[:, :2], y)                                # d changes
    assert gpu_ctx.sens_get_measure().shape == (2,) and not gpu_ctx.sens_get_measure().any()


# ---------------------------------------------------------------------------------------------------- 4. set up by a batch
@pytest.mark.parametrize("N,d,mn", [(130, 3, "gauss"), (130, 3, "mixed"), (65, 9, "block")])
def test_setup_by_batch_same_bits(N, d, mn):
    """components set up by gpemu_predict_setup_batch against contexts set up alone: every entry, the cross case both ways"""
    order = 1
    X, y = TP.data(N, d)
    ys, ths = [y, np.cos(2.0 * y)], [TP.thetas(d), TP.thetas(d) + 0.1]
    kind = kinds(mn, d)
    lo, hi = measure_of(kind, X)
    ctxs, alone = [abi.Context(0) for _ in ys], [abi.Context(0) for _ in ys]
    try:
        for c, yc in zip(ctxs, ys):
            c.set_model(1, order, X, yc)
            c.sens_set_measure(kind)                                        # before the set-up: it keeps the kinds
        _, _, status, rc = abi.predict_setup_batch(ctxs, np.array(ths))
        assert rc == abi.OK and not status.any()
        for c, yc, tc in zip(alone, ys, ths):
            TP.fit(c, order, X, yc, tc)
            c.sens_set_measure(kind)
        for i in (0, 1):
            assert all(np.array_equal(p, q) for p, q in zip(_all_entries(ctxs[i], kind, X, lo, hi), _all_entries(alone[i], kind, X, lo, hi)))
        for i in (0, 1):
            p, q = plug_entries(ctxs[i], kind, X, lo, hi, ctxs[1 - i], dev=False), plug_entries(alone[i], kind, X, lo, hi, alone[1 - i], dev=False)
            assert all(np.array_equal(p[key], q[key]) for key in p)
    finally:
        for c in ctxs + alone:
            c.close()


# ---------------------------------------------------------------------------------------------------- 5. Monte Carlo
def test_monte_carlo_cross_check(gpu_ctx):
    """A wrong definition, not rounding: 2^16 seeded Gaussian draws through gpemu_predict_mean.  E0 and V from the plain sample,
    V_j from the pick-freeze products, VT_j from Jansen's squared differences, a main effect from the sample with x_j fixed;
    each within five of its own standard errors (test_gpu_sens.py's rule)."""
    N, d, n = 200, 3, 1 << 16
    X, y = TS.data(N, d)
    th = TS.thetas(d)
    TS.fit(gpu_ctx, 1, X, y, th)
    kind = kinds("gauss", d)
    gpu_ctx.sens_set_measure(kind)
    box_lo, box_hi = R.boxes(X)["design"]
    lo, hi = (box_lo + box_hi) / 2, 0.2 * (box_hi - box_lo)
    got = gpu_ctx.sens_cov(lo, hi)
    e0, V = got["e0"][0], got["cov_all"]
    rng = np.random.default_rng(20261020)
    A, B = (M.sample(kind, lo, hi, rng, n) for _ in range(2))
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
    g = lo + 0.7 * hi
    _, main = gpu_ctx.sens_main(lo, hi, g.reshape(d, 1))
    for j in range(d):
        fixed = A.copy()
        fixed[:, j] = g[j]
        within(f"E[m | x_{j} = {g[j]:.3f}]", gpu_ctx.predict_mean(fixed), main[j, 0])


# ---------------------------------------------------------------------------------------------------- 6. errors
def _rcs(a, b, lo, hi):
    """the return codes of every entry, host and _dev, for these bounds (nothing is launched where a check refuses)"""
    d = a.d
    npairs = max(d * (d - 1) // 2, 1)
    lo, hi = abi._a(lo), abi._a(hi)
    L, p = a.L, abi._p
    o = [np.empty(4 + 2 * d + npairs) for _ in range(6)]
    g = np.full(d, 0.5)
    buf = a.dev_alloc((4 + 2 * d + npairs) * 8)
    try:
        rcs = dict(
            cov=L.gpemu_sens_cov(a.h, b.h, p(lo), p(hi), p(o[0]), p(o[1]), p(o[2]), p(o[3])),
            cov_dev=L.gpemu_sens_cov_dev(a.h, b.h, p(lo), p(hi), buf),
            pairs=L.gpemu_sens_pairs(a.h, b.h, p(lo), p(hi), p(o[0])),
            pairs_dev=L.gpemu_sens_pairs_dev(a.h, b.h, p(lo), p(hi), buf))
        if a is b:
            rcs.update(
                main=L.gpemu_sens_main(a.h, p(lo), p(hi), 1, p(g), p(o[0]), p(o[1])),
                post=L.gpemu_sens_post(a.h, p(lo), p(hi), p(o[0]), p(o[1]), p(o[2]), p(o[3])),
                post_dev=L.gpemu_sens_post_dev(a.h, p(lo), p(hi), buf),
                main_var=L.gpemu_sens_main_var(a.h, p(lo), p(hi), 1, p(g), p(o[0]), p(o[1]), p(o[2])),
                pairs_post=L.gpemu_sens_pairs_post(a.h, p(lo), p(hi), p(o[0])),
                pairs_post_dev=L.gpemu_sens_pairs_post_dev(a.h, p(lo), p(hi), buf),
                joint=L.gpemu_sens_joint(a.h, p(lo), p(hi), 0, 1, 1, p(g), p(g), p(o[0]), p(o[1]), p(o[2])))
        a.sync()
    finally:
        a.dev_free(buf)
    return rcs


def test_errors(gpu_ctx, second_ctx):
    N, d, order = 90, 3, 1
    X, y = TP.data(N, d)
    th = TP.thetas(d)
    L = gpu_ctx.L
    two = (abi.C.c_int * 2)(0, 1)
    # the setter and the getter
    assert L.gpemu_sens_set_measure(None, None) == abi.ERR_ARG and L.gpemu_sens_set_measure(None, two) == abi.ERR_ARG
    assert L.gpemu_sens_get_measure(None, two) == abi.ERR_ARG
    fresh = abi.Context(0)
    try:
        assert L.gpemu_sens_set_measure(fresh.h, None) == abi.ERR_STATE and L.gpemu_sens_set_measure(fresh.h, two) == abi.ERR_STATE
        assert L.gpemu_sens_get_measure(fresh.h, two) == abi.ERR_STATE
        assert L.gpemu_sens_get_measure(fresh.h, None) == abi.ERR_ARG
    finally:
        fresh.close()
    TP.fit(gpu_ctx, order, X, y, th)
    mixed = kinds("mixed", d)                                               # uniform, Gaussian, uniform
    gpu_ctx.sens_set_measure(mixed)
    for bad in (2, -1, 7):
        k = mixed.copy()
        k[1] = bad
        with pytest.raises(abi.GpemuError) as ei:
            gpu_ctx.sens_set_measure(k)
        assert ei.value.code == abi.ERR_ARG
        assert np.array_equal(gpu_ctx.sens_get_measure(), mixed)            # nothing was stored
    lo, hi = measure_of(mixed, X)
    assert set(_rcs(gpu_ctx, gpu_ctx, lo, hi).values()) == {abi.OK}
    # a Gaussian coordinate: hi <= lo is fine (mean 0.5, sd 0.1), sd <= 0 or anything non-finite is not
    ok_lo, ok_hi = lo.copy(), hi.copy()
    ok_lo[1], ok_hi[1] = 0.5, 0.1
    assert set(_rcs(gpu_ctx, gpu_ctx, ok_lo, ok_hi).values()) == {abi.OK}
    for bad in (0.0, -0.1, np.nan, np.inf, -np.inf):
        b = hi.copy()
        b[1] = bad
        assert set(_rcs(gpu_ctx, gpu_ctx, lo, b).values()) == {abi.ERR_ARG}, bad
    assert "standard deviation" in L.gpemu_last_error(gpu_ctx.h).decode()
    for bad in (np.nan, np.inf, -np.inf):
        b = lo.copy()
        b[1] = bad
        assert set(_rcs(gpu_ctx, gpu_ctx, b, hi).values()) == {abi.ERR_ARG}, bad
    # a uniform coordinate of the same call keeps its check
    b = hi.copy()
    b[0] = lo[0]
    assert set(_rcs(gpu_ctx, gpu_ctx, lo, b).values()) == {abi.ERR_ARG}
    b[0] = lo[0] - 0.1
    assert set(_rcs(gpu_ctx, gpu_ctx, lo, b).values()) == {abi.ERR_ARG}
    assert "hi > lo" in L.gpemu_last_error(gpu_ctx.h).decode()
    # two contexts: the kinds must agree
    TP.fit(second_ctx, order, X, np.cos(y), th)
    assert set(_rcs(gpu_ctx, second_ctx, lo, hi).values()) == {abi.ERR_ARG}
    assert "measure" in L.gpemu_last_error(gpu_ctx.h).decode()
    assert set(_rcs(second_ctx, gpu_ctx, lo, hi).values()) == {abi.ERR_ARG}
    second_ctx.sens_set_measure(kinds("gauss", d))
    assert set(_rcs(gpu_ctx, second_ctx, lo, hi).values()) == {abi.ERR_ARG}
    second_ctx.sens_set_measure(mixed)
    assert set(_rcs(gpu_ctx, second_ctx, lo, hi).values()) == {abi.OK}
    # a refused call has left everything as it was
    assert set(_rcs(gpu_ctx, gpu_ctx, lo, hi).values()) == {abi.OK}


def test_prof_counts_a_gaussian_factor_as_one_exp(gpu_ctx):
    """the flop rule at GPEMU_PROF_SENS*: 19 per uniform coordinate's pair factor, 12 per Gaussian one's"""
    N, d = 130, 3
    X, y = TS.data(N, d)
    TS.fit(gpu_ctx, 1, X, y, TS.thetas(d))
    T = ((N + 63) // 64) ** 2 * (2 * d + 1)
    for mn, per_pair in (("gauss", 12.0 * 3), ("mixed", 19.0 * 2 + 12.0)):
        kind = kinds(mn, d)
        gpu_ctx.sens_set_measure(kind)
        lo, hi = measure_of(kind, X)
        gpu_ctx.prof_begin(abi.PROF_SENS)
        gpu_ctx.sens_cov(lo, hi)
        p = gpu_ctx.prof_end()
        assert p["n"] == 3 and p["flops"] == 88.0 * N * d + N * N * (per_pair + 2.0) + T, (mn, p)
