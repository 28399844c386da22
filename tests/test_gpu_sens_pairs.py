"""Second-order Sobol indices and interaction surfaces in closed form (gpemu_sens_pairs / gpemu_sens_pairs_post /
gpemu_sens_joint, include/gpemu.h) through the public entries, against tests/senspairref.py (numpy fp64;
test_senspairref.py pins it against mpmath and against quadrature).

What is compared, as in test_gpu_sens.py and test_gpu_sens_post.py, whose inputs (`data`, `thetas`, `fit`) this file uses:
beta and gamma come from the device's own prediction state, P, G and Q from gpemu_test_sens_post_state; everything downstream
of them -- the integrals, the leave-two-out products, the N x N sweep, the assembly -- is the reference's own.  Errors are
relative to the SCALE the reference returns beside every value.

Shapes.  N in {1, 63, 64, 65, 130} (one point, the edges of the 64 x 64 tiles, three tile rows) times d in {2, 3, 8, 9, 16, 17}
(one coordinate block and its edge, the first off-diagonal block and its edge, three blocks and one coordinate of a fourth).
The regression order touches the finish alone, never the sweep, so it cycles through 0 .. 3 over the shapes (every N and
every d meets every order that fits under N points) instead of multiplying them.

The bars.  NP_VS_MP is the largest scaled error of the numpy reference against mpmath at 50 digits over exactly the cases of
this file (`plug_cases()` with beta and gamma from a LAPACK fit, `post_cases()` with P, G, Q from a numpy fit), measured on
the CPU by `python tests/senspairref.py --measure`; the device gets FACTOR = 8 times that, one constant for the plug-in
quantities (cov_pair, joint, inter) and one for the S quantities (s_pair).
  measured NP_VS_MP_PLUG = 3.1e-12 -> TOL   = 2.5e-11   (worst: the narrow box with two contexts at order 2; the design's box stays below 2.5e-13)
  measured NP_VS_MP_POST = 5.8e-16 -> TOL_S = 4.6e-15   (worst: the disjoint box at order 0; most cases sit at 1e-17 to 5e-16)
Two device results compared with each other (the d = 2 and d = 3 identities) get twice the bar."""
import numpy as np
import pytest

import sensref as R
import senspairref as SPR
import senspostref as SP
import test_gpu_sens as TS
import test_gpu_sens_post as TP
from madaiemulator_amd import abi, synth

NP_VS_MP_PLUG = 3.1e-12
NP_VS_MP_POST = 5.8e-16
FACTOR = 8
TOL = FACTOR * NP_VS_MP_PLUG
TOL_S = FACTOR * NP_VS_MP_POST

pytestmark = pytest.mark.gpu

NS = [1, 63, 64, 65, 130]
DS = [2, 3, 8, 9, 16, 17]
JOINT_CASES = [(130, 3, 2, 0, 2), (65, 8, 1, 2, 7), (64, 17, 0, 7, 16), (63, 2, 3, 0, 1), (1, 2, 0, 0, 1)]      # N, d, order, j, k


# ---------------------------------------------------------------------------------------------------- inputs
def shape_cases():
    """(N, d, order): the order cycles over the shapes, lowered until there are as many points as regression functions"""
    out = []
    for a, N in enumerate(NS):
        for b, d in enumerate(DS):
            o = (a + b) % 4
            while 1 + o * d > N:
                o -= 1
            out.append((N, d, o))
    return out


def extra_cases():
    """(name, N, d, order, box, cross): the three boxes and the two-context case"""
    return [(f"{box}{'-cross' if cross else ''}", 130, 3, order, box, cross)
            for box in ("design", "narrow", "disjoint") for cross in (False, True) for order in (0, 2)]


def joint_points(X, lo, hi, j, k):
    """the points the surface is compared at: corners of the box, a design point, the centre, two more"""
    t = np.array([0.0, 1.0, 1.0, 0.5, 0.3, 0.81])
    u = np.array([0.0, 1.0, 0.0, 0.5, 0.9, 0.17])
    xj, xk = lo[j] + t * (hi[j] - lo[j]), lo[k] + u * (hi[k] - lo[k])
    return np.append(xj, X[len(X) // 2, j]), np.append(xk, X[len(X) // 2, k])


def plug_cases():
    """every (name, X, [(y, th), ...one or two...], order, lo, hi, joint (j, k) or None) of the plug-in quantities"""
    out = []
    for N, d, o in shape_cases():
        X, y = TS.data(N, d)
        out.append((f"N{N}-d{d}-o{o}", X, [(y, TS.thetas(d))], o) + R.boxes(X)["design"] + (None,))
    for name, N, d, o, box, cross in extra_cases():
        X, y = TS.data(N, d)
        fits = [(y, TS.thetas(d))] + ([(TS.data(N, d, 1)[1], TS.thetas(d, 0.2))] if cross else [])
        out.append((name + f"-o{o}", X, fits, o) + R.boxes(X)[box] + (None,))
    X, y, th = TS.unused_case()
    out.append(("unused", X, [(y, th)], 1) + R.boxes(X)["design"] + (None,))
    for N, d, o, j, k in JOINT_CASES:
        X, y = TS.data(N, d)
        for box in ("design", "narrow"):
            out.append((f"joint-N{N}-d{d}-o{o}-{box}", X, [(y, TS.thetas(d))], o) + R.boxes(X)[box] + ((j, k),))
    return out


def post_cases():
    """every (name, X, y, th, order, lo, hi) of the S quantities"""
    out = []
    for N, d, o in shape_cases():
        X, y = TP.data(N, d)
        out.append((f"N{N}-d{d}-o{o}", X, y, TP.thetas(d), o) + R.boxes(X)["design"])
    for box in ("narrow", "disjoint"):
        for o in (0, 2):
            X, y = TP.data(130, 3)
            out.append((f"{box}-o{o}", X, y, TP.thetas(3), o) + R.boxes(X)[box])
    return out


def _measure_plug(case):
    import meanref
    name, X, fits, o, lo, hi, jk = case
    ms = []
    for y, th in fits:
        beta, gamma = meanref.trained(1, o, X, y, th)
        ms.append(TS.model_of(th, beta, gamma))
    if jk is None:
        val, scale = SPR.pair_covariances(R.NP, X, ms[0], ms[-1], lo, hi)
        mp, _ = SPR.pair_covariances(R.MP(), X, ms[0], ms[-1], lo, hi)
        return name, SPR.scaled_errors(val, mp, scale, ("cov_pair",))
    xj, xk = joint_points(X, lo, hi, *jk)
    val, scale = SPR.joint_surface(R.NP, X, ms[0], lo, hi, *jk, xj, xk)
    mp, _ = SPR.joint_surface(R.MP(), X, ms[0], lo, hi, *jk, xj, xk)
    return name, SPR.scaled_errors(val, mp, scale, ("e0", "joint", "inter"))


def _measure_post(case):
    name, X, y, th, o, lo, hi = case
    m = TP.model_of(th)
    P, G, Q = SP.fit_state(X, y, o, m["A"], m["s"], TP.NUGGET)[:3]
    val, scale = SPR.pair_post(R.NP, X, m, P, G, Q, lo, hi)
    mp, _ = SPR.pair_post(R.MP(), X, m, P, G, Q, lo, hi)
    return name, SPR.scaled_errors(val, mp, scale, ("s_pair",))


def measure_np_against_mp():
    """the figures NP_VS_MP_PLUG and NP_VS_MP_POST are set from (CPU, minutes)"""
    import multiprocessing as mpc
    import sys
    from oracle import oracle as O
    O.build()
    for what, fn, cases in (("plug-in", _measure_plug, plug_cases()), ("S", _measure_post, post_cases())):
        cases = sorted(cases, key=lambda c: -c[1].size * len(c[1]))
        if "--only" in sys.argv:                     # names that start with the given prefixes
            cases = [c for c in cases if c[0].startswith(tuple(sys.argv[sys.argv.index("--only") + 1].split(",")))]
        worst = ("", 0.0)
        with mpc.Pool(min(8, mpc.cpu_count())) as pool:
            for name, e in pool.imap_unordered(fn, cases):
                print(f"{what} {name}: {e:.3e}", flush=True)
                if e > worst[1]:
                    worst = (name, e)
        print(f"{what}: largest scaled error of numpy against mpmath over {len(cases)} cases: {worst[1]:.3e} ({worst[0]})", flush=True)


# ---------------------------------------------------------------------------------------------------- helpers
def check(what, got, ref, scale, keys, tol):
    e = SPR.scaled_errors(got, ref, scale, keys)
    print(f"{what}: scaled error {e:.2e} (bar {tol:.1e})")
    for k in keys:
        assert np.all(np.isfinite(got[k])), (what, k)
    assert e < tol, (what, e)
    return e


def interactions(what, pair, pscale, cov, cscale):
    """V_jk - V_j - V_k >= 0 and V_jk <= V up to the bar times the scales of what is subtracted"""
    d = len(cov["cov_first"])
    for j, k in SPR.pairs(d):
        p = SPR.pair_index(j, k, d)
        slack = TOL * (pscale["cov_pair"][p] + cscale["cov_first"][j] + cscale["cov_first"][k])
        assert pair[p] - cov["cov_first"][j] - cov["cov_first"][k] >= -slack, (what, j, k)
        assert pair[p] <= cov["cov_all"] + TOL * (pscale["cov_pair"][p] + cscale["cov_all"]), (what, j, k)


def identities(what, pair, pscale, all_, all_scale, rest, rest_scale, tol):
    """d = 2: the pair is everything; d = 3: the pair (j, k) is all but the third coordinate.  Two device results: twice the bar"""
    d = len(rest)
    if d == 2:
        assert abs(pair[0] - all_) <= 2 * tol * (pscale[0] + all_scale), what
    if d == 3:
        for j, k in SPR.pairs(3):
            p, l = SPR.pair_index(j, k, 3), 3 - j - k
            assert abs(pair[p] - rest[l]) <= 2 * tol * (pscale[p] + rest_scale[l]), (what, j, k)


@pytest.fixture(scope="module")
def second_ctx():
    ctx = abi.Context(0)
    yield ctx
    ctx.close()


# ---------------------------------------------------------------------------------------------------- 1. pair covariances
@pytest.mark.parametrize("N", NS)
def test_pair_shapes(gpu_ctx, N):
    for n, d, o in shape_cases():
        if n != N:
            continue
        X, y = TS.data(N, d)
        lo, hi = R.boxes(X)["design"]
        m = TS.fit(gpu_ctx, o, X, y, TS.thetas(d))
        got = dict(cov_pair=gpu_ctx.sens_pairs(lo, hi))
        ref, scale = SPR.pair_covariances(R.NP, X, m, m, lo, hi)
        what = f"N {N} d {d} order {o}"
        assert got["cov_pair"].shape == (d * (d - 1) // 2,)
        check(what, got, ref, scale, ("cov_pair",), TOL)
        cov = gpu_ctx.sens_cov(lo, hi)
        _, cscale = R.covariances(R.NP, X, m, m, lo, hi)
        interactions(what, got["cov_pair"], scale, cov, cscale)
        identities(what, got["cov_pair"], scale["cov_pair"], cov["cov_all"], cscale["cov_all"], cov["cov_rest"], cscale["cov_rest"], TOL)


@pytest.mark.parametrize("name,N,d,order,box,cross", extra_cases())
def test_pair_boxes_and_two_contexts(gpu_ctx, second_ctx, name, N, d, order, box, cross):
    X, y = TS.data(N, d)
    lo, hi = R.boxes(X)[box]
    ma = TS.fit(gpu_ctx, order, X, y, TS.thetas(d))
    mb, other = ma, None
    if cross:
        mb, other = TS.fit(second_ctx, order, X, TS.data(N, d, 1)[1], TS.thetas(d, 0.2)), second_ctx
    got = dict(cov_pair=gpu_ctx.sens_pairs(lo, hi, other))
    ref, scale = SPR.pair_covariances(R.NP, X, ma, mb, lo, hi)
    check(f"{name} order {order}", got, ref, scale, ("cov_pair",), TOL)
    cov = gpu_ctx.sens_cov(lo, hi, other)
    _, cscale = R.covariances(R.NP, X, ma, mb, lo, hi)
    identities(name, got["cov_pair"], scale["cov_pair"], cov["cov_all"], cscale["cov_all"], cov["cov_rest"], cscale["cov_rest"], TOL)
    if cross:
        # the other way round: the same numbers to the bar
        back = dict(cov_pair=second_ctx.sens_pairs(lo, hi, gpu_ctx))
        check(f"{name} order {order}, contexts swapped", back, ref, scale, ("cov_pair",), TOL)
    else:
        interactions(name, got["cov_pair"], scale, cov, cscale)


def test_unused_coordinate(gpu_ctx):
    """the data ignore x_2 and its length scale is long (e^3 against a box of width 1): its interactions vanish against the
    variance.  They are not 0 to rounding: k_2 varies over the box by w^2 / (2 e^6) = 1.2e-3 of itself, an interaction
    variance is of the square of that, 1.5e-6 of the kernel part's variance -- mpmath gives 7e-9 V and 4e-7 V, far above
    TOL times the scale.  So the device's values are held to the reference's at TOL, and to 1e-5 V in size (1.5e-6 with a
    margin of six; test_gpu_sens.py's case of the same name asks 1e-3 V of the first-order and total indices)."""
    X, y, th = TS.unused_case()
    m = TS.fit(gpu_ctx, 1, X, y, th)
    lo, hi = R.boxes(X)["design"]
    pair = gpu_ctx.sens_pairs(lo, hi)
    ref, scale = SPR.pair_covariances(R.NP, X, m, m, lo, hi)
    check("unused coordinate", dict(cov_pair=pair), ref, scale, ("cov_pair",), TOL)
    cov = gpu_ctx.sens_cov(lo, hi)
    V, first = cov["cov_all"], cov["cov_first"]
    inter = {(j, k): pair[SPR.pair_index(j, k, 3)] - first[j] - first[k] for j, k in SPR.pairs(3)}
    print("second-order indices:", {jk: v / V for jk, v in inter.items()})
    assert abs(inter[(0, 2)]) < 1e-5 * V and abs(inter[(1, 2)]) < 1e-5 * V


# ---------------------------------------------------------------------------------------------------- 2. the surface
@pytest.mark.parametrize("N,d,order,j,k", JOINT_CASES)
def test_joint_surface(gpu_ctx, N, d, order, j, k):
    """joint and inter against the reference; joint - inter against gpemu_sens_main's curves; E0 is gpemu_sens_cov's; the
    pair the other way round and a second call give the same bits; inter may be left out"""
    X, y = TS.data(N, d)
    m = TS.fit(gpu_ctx, order, X, y, TS.thetas(d))
    for box in ("design", "narrow"):
        lo, hi = R.boxes(X)[box]
        xj, xk = joint_points(X, lo, hi, j, k)
        e0, joint, inter = gpu_ctx.sens_joint(lo, hi, j, k, xj, xk)
        ref, scale = SPR.joint_surface(R.NP, X, m, lo, hi, j, k, xj, xk)
        what = f"surface N {N} d {d} order {order} ({j}, {k}) {box}"
        check(what, dict(e0=e0, joint=joint, inter=inter), ref, scale, ("e0", "joint", "inter"), TOL)
        grid = np.tile(lo[:, None], (1, len(xj)))
        grid[j], grid[k] = xj, xk
        me0, main = gpu_ctx.sens_main(lo, hi, grid)
        _, mscale = R.main_effects(R.NP, X, m, lo, hi, grid)
        slack = 2 * TOL * (scale["joint"] + scale["inter"] + mscale["main"][j] + mscale["main"][k] + mscale["e0"])
        assert np.all(np.abs((joint - inter) - (main[j] + main[k] - me0)) <= slack), what
        assert e0 == me0 == gpu_ctx.sens_cov(lo, hi)["e0"][0]
        for again in (gpu_ctx.sens_joint(lo, hi, j, k, xj, xk), gpu_ctx.sens_joint(lo, hi, k, j, xk, xj)):
            assert again[0] == e0 and np.array_equal(again[1], joint) and np.array_equal(again[2], inter)
        one = gpu_ctx.sens_joint(lo, hi, j, k, xj[:1], xk[:1])                   # npts = 1
        assert one[1][0] == joint[0] and one[2][0] == inter[0]
    lo_, hi_, e, jt = abi._a(lo), abi._a(hi), np.empty(1), np.empty(len(xj))
    assert gpu_ctx.L.gpemu_sens_joint(gpu_ctx.h, abi._p(lo_), abi._p(hi_), j, k, len(xj), abi._p(xj), abi._p(xk), abi._p(e), abi._p(jt), None) == abi.OK
    assert np.array_equal(jt, joint)


# ---------------------------------------------------------------------------------------------------- 3. uncertainty
def post_and_reference(ctx, X, m, lo, hi):
    got = dict(s_pair=ctx.sens_pairs_post(lo, hi))
    P, G, Q = ctx.sens_post_state()
    ref, scale = SPR.pair_post(R.NP, X, m, P, G, Q, lo, hi)
    return got, ref, scale, (P, G, Q)


def post_checks(what, ctx, X, m, lo, hi):
    d = X.shape[1]
    got, ref, scale, (P, G, Q) = post_and_reference(ctx, X, m, lo, hi)
    check(what, got, ref, scale, ("s_pair",), TOL_S)
    post = ctx.sens_post(lo, hi)
    _, pscale = SP.post(R.NP, X, m, P, G, Q, lo, hi)
    s = got["s_pair"]
    # Jensen: s_none <= s_first[j], s_first[k] <= s_pair <= s_all
    for j, k in SPR.pairs(d):
        p = SPR.pair_index(j, k, d)
        slack = TOL_S * (scale["s_pair"][p] + pscale["s_all"] + pscale["s_first"][j] + pscale["s_first"][k])
        assert max(post["s_first"][j], post["s_first"][k]) <= s[p] + slack and s[p] <= post["s_all"] + slack, (what, j, k)
        assert s[p] >= -TOL_S * scale["s_pair"][p]
    identities(what, s, scale["s_pair"], post["s_all"], pscale["s_all"], post["s_rest"], pscale["s_rest"], TOL_S)


@pytest.mark.parametrize("N", NS)
def test_pair_post_shapes(gpu_ctx, N):
    for n, d, o in shape_cases():
        if n != N:
            continue
        X, y = TP.data(N, d)
        lo, hi = R.boxes(X)["design"]
        m = TP.fit(gpu_ctx, o, X, y, TP.thetas(d))
        post_checks(f"S N {N} d {d} order {o}", gpu_ctx, X, m, lo, hi)


@pytest.mark.parametrize("box", ["narrow", "disjoint"])
@pytest.mark.parametrize("order", [0, 2])
def test_pair_post_boxes(gpu_ctx, box, order):
    X, y = TP.data(130, 3)
    lo, hi = R.boxes(X)[box]
    m = TP.fit(gpu_ctx, order, X, y, TP.thetas(3))
    post_checks(f"S {box} order {order}", gpu_ctx, X, m, lo, hi)


# ---------------------------------------------------------------------------------------------------- 4. bits, bystanders
def _dev(ctx, n, call):
    buf = ctx.dev_alloc(n * 8)
    try:
        call(buf)
        return ctx.download(buf, (n,))
    finally:
        ctx.dev_free(buf)


def test_same_bits_and_bystanders(gpu_ctx, second_ctx):
    N, d, order = 200, 9, 1
    npairs = d * (d - 1) // 2
    X, y = TS.data(N, d)
    TS.fit(gpu_ctx, order, X, y, TS.thetas(d))
    TS.fit(second_ctx, order, X, TS.data(N, d, 1)[1], TS.thetas(d, 0.2))
    lo, hi = R.boxes(X)["narrow"]
    Xq = X[:9] + 0.01
    cov_before, post_before = gpu_ctx.sens_cov(lo, hi), gpu_ctx.sens_post(lo, hi)
    for other in (None, second_ctx):
        a = gpu_ctx.sens_pairs(lo, hi, other)
        assert np.array_equal(a, gpu_ctx.sens_pairs(lo, hi, other))
        assert np.array_equal(a, _dev(gpu_ctx, npairs, lambda buf: gpu_ctx.sens_pairs_dev(lo, hi, buf, other)))
        gpu_ctx.sens_release()
        assert np.array_equal(a, gpu_ctx.sens_pairs(lo, hi, other))
    s = gpu_ctx.sens_pairs_post(lo, hi)
    assert np.array_equal(s, gpu_ctx.sens_pairs_post(lo, hi))
    assert np.array_equal(s, _dev(gpu_ctx, npairs, lambda buf: gpu_ctx.sens_pairs_post_dev(lo, hi, buf)))
    gpu_ctx.sens_release()
    assert np.array_equal(s, gpu_ctx.sens_pairs_post(lo, hi))
    # a pending prediction batch stays collectable across all three entries
    want = gpu_ctx.predict(Xq)
    gpu_ctx.predict_enqueue(Xq)
    gpu_ctx.sens_pairs(lo, hi, second_ctx)
    gpu_ctx.sens_pairs_post(lo, hi)
    gpu_ctx.sens_joint(lo, hi, 1, 8, lo[[1, 1]], hi[[8, 8]])
    got = gpu_ctx.predict_collect()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # gpemu_sens_cov and gpemu_sens_post return the same bits before and after
    cov_after, post_after = gpu_ctx.sens_cov(lo, hi), gpu_ctx.sens_post(lo, hi)
    assert all(np.array_equal(cov_before[k], cov_after[k]) for k in R.KEYS)
    assert all(np.array_equal(post_before[k], post_after[k]) for k in SP.KEYS)
    # profiling classes: prep, pair prep, sweep (both launches of d > 8 under one scope), finish; pmat besides for S
    gpu_ctx.prof_begin(abi.PROF_SENS)
    gpu_ctx.sens_pairs(lo, hi)
    p = gpu_ctx.prof_end()
    assert p["n"] == 4 and p["ms"] > 0
    gpu_ctx.prof_begin(abi.PROF_SENS_POST)
    gpu_ctx.sens_pairs_post(lo, hi)
    assert gpu_ctx.prof_end()["n"] == 5


def test_setup_by_batch_same_bits():
    """components set up by gpemu_predict_setup_batch against contexts set up alone, the cross case included"""
    N, d, order = 130, 3, 1
    X, y = TS.data(N, d)
    ys, ths = [y, TS.data(N, d, 1)[1]], [TS.thetas(d), TS.thetas(d, 0.2)]
    lo, hi = R.boxes(X)["design"]
    xj, xk = joint_points(X, lo, hi, 0, 2)
    ctxs, alone = [abi.Context(0) for _ in ys], [abi.Context(0) for _ in ys]
    try:
        for c, yc in zip(ctxs, ys):
            c.set_model(1, order, X, yc)
        _, _, status, rc = abi.predict_setup_batch(ctxs, np.array(ths))
        assert rc == abi.OK and not status.any()
        for c, yc, tc in zip(alone, ys, ths):
            TS.fit(c, order, X, yc, tc)
        for i in (0, 1):
            assert np.array_equal(ctxs[i].sens_pairs(lo, hi), alone[i].sens_pairs(lo, hi))
            assert np.array_equal(ctxs[i].sens_pairs_post(lo, hi), alone[i].sens_pairs_post(lo, hi))
            assert all(np.array_equal(p, q) for p, q in zip(ctxs[i].sens_joint(lo, hi, 0, 2, xj, xk), alone[i].sens_joint(lo, hi, 0, 2, xj, xk)))
        assert np.array_equal(ctxs[0].sens_pairs(lo, hi, ctxs[1]), alone[0].sens_pairs(lo, hi, alone[1]))
        assert np.array_equal(ctxs[1].sens_pairs(lo, hi, ctxs[0]), alone[1].sens_pairs(lo, hi, alone[0]))
    finally:
        for c in ctxs + alone:
            c.close()


# ---------------------------------------------------------------------------------------------------- 5. errors
def _pairs_rc(a, b, lo, hi, out=True):
    d = max(a.d, 2)
    o = np.empty(d * (d - 1) // 2)
    lo = None if lo is None else abi._a(lo)
    hi = None if hi is None else abi._a(hi)
    return a.L.gpemu_sens_pairs(a.h, b.h if b is not None else None, None if lo is None else abi._p(lo), None if hi is None else abi._p(hi),
                                abi._p(o) if out else None)


def _post_rc(a, lo, hi, out=True):
    d = max(a.d, 2)
    o = np.empty(d * (d - 1) // 2)
    lo = None if lo is None else abi._a(lo)
    hi = None if hi is None else abi._a(hi)
    return a.L.gpemu_sens_pairs_post(a.h, None if lo is None else abi._p(lo), None if hi is None else abi._p(hi), abi._p(o) if out else None)


def _joint_rc(a, lo, hi, j, k, npts, xj=True, xk=True, e0=True, joint=True, inter=True):
    n = max(npts, 1)
    x, z, e, jt, it = np.full(n, 0.5), np.full(n, 0.5), np.empty(1), np.empty(n), np.empty(n)
    lo, hi = abi._a(lo), abi._a(hi)
    ptr = [abi._p(v) if on else None for v, on in zip((x, z, e, jt, it), (xj, xk, e0, joint, inter))]
    return a.L.gpemu_sens_joint(a.h, abi._p(lo), abi._p(hi), j, k, npts, *ptr)


def test_errors(gpu_ctx, second_ctx):
    N, d, order = 90, 3, 1
    X, y = TS.data(N, d)
    th = TS.thetas(d)
    lo, hi = R.boxes(X)["design"]
    L = gpu_ctx.L
    fresh = abi.Context(0)
    try:
        fresh.set_model(1, order, X, y)
        TS.fit(gpu_ctx, order, X, y, th)
        # NULL pointers come first, whatever the state
        assert _pairs_rc(fresh, fresh, lo, hi, out=False) == abi.ERR_ARG and _pairs_rc(fresh, None, lo, hi) == abi.ERR_ARG
        assert _pairs_rc(fresh, fresh, None, hi) == abi.ERR_ARG and _pairs_rc(fresh, fresh, lo, None) == abi.ERR_ARG
        assert L.gpemu_sens_pairs(None, None, None, None, None) == abi.ERR_ARG
        assert L.gpemu_sens_pairs_dev(fresh.h, fresh.h, abi._p(lo), abi._p(hi), None) == abi.ERR_ARG
        assert L.gpemu_sens_pairs_dev(None, fresh.h, abi._p(lo), abi._p(hi), None) == abi.ERR_ARG
        assert _post_rc(fresh, lo, hi, out=False) == abi.ERR_ARG and _post_rc(fresh, None, hi) == abi.ERR_ARG and _post_rc(fresh, lo, None) == abi.ERR_ARG
        assert L.gpemu_sens_pairs_post(None, None, None, None) == abi.ERR_ARG
        assert L.gpemu_sens_pairs_post_dev(fresh.h, abi._p(lo), abi._p(hi), None) == abi.ERR_ARG
        assert L.gpemu_sens_pairs_post_dev(None, abi._p(lo), abi._p(hi), None) == abi.ERR_ARG
        for kw in (dict(xj=False), dict(xk=False), dict(e0=False), dict(joint=False)):
            assert _joint_rc(fresh, lo, hi, 0, 1, 3, **kw) == abi.ERR_ARG
        assert L.gpemu_sens_joint(None, None, None, 0, 1, 1, None, None, None, None, None) == abi.ERR_ARG
        # no prediction set-up on either context
        assert _pairs_rc(fresh, fresh, lo, hi) == abi.ERR_STATE
        assert _pairs_rc(gpu_ctx, fresh, lo, hi) == abi.ERR_STATE and _pairs_rc(fresh, gpu_ctx, lo, hi) == abi.ERR_STATE
        assert _post_rc(fresh, lo, hi) == abi.ERR_STATE and _joint_rc(fresh, lo, hi, 0, 1, 3) == abi.ERR_STATE
        assert _joint_rc(fresh, lo, hi, 0, 0, 0) == abi.ERR_STATE                # (the state before the indices)
        with pytest.raises(abi.GpemuError) as ei:
            fresh.sens_pairs(lo, hi)
        assert ei.value.code == abi.ERR_STATE
    finally:
        fresh.close()
    assert _pairs_rc(gpu_ctx, gpu_ctx, lo, hi) == abi.OK and _post_rc(gpu_ctx, lo, hi) == abi.OK
    assert _joint_rc(gpu_ctx, lo, hi, 0, 2, 3) == abi.OK and _joint_rc(gpu_ctx, lo, hi, 2, 0, 1, inter=False) == abi.OK
    # the pair and the number of points
    for j, k in ((0, 0), (2, 2), (-1, 1), (1, -1), (0, 3), (3, 0), (7, 9)):
        assert _joint_rc(gpu_ctx, lo, hi, j, k, 3) == abi.ERR_ARG, (j, k)
    assert _joint_rc(gpu_ctx, lo, hi, 0, 1, 0) == abi.ERR_ARG and _joint_rc(gpu_ctx, lo, hi, 0, 1, -4) == abi.ERR_ARG
    # bounds
    for l in range(d):
        for bad in (np.nan, np.inf, -np.inf):
            b = lo.copy(); b[l] = bad
            assert _pairs_rc(gpu_ctx, gpu_ctx, b, hi) == abi.ERR_ARG and _post_rc(gpu_ctx, b, hi) == abi.ERR_ARG
            assert _joint_rc(gpu_ctx, b, hi, 0, 1, 3) == abi.ERR_ARG
            b = hi.copy(); b[l] = bad
            assert _pairs_rc(gpu_ctx, gpu_ctx, lo, b) == abi.ERR_ARG and _post_rc(gpu_ctx, lo, b) == abi.ERR_ARG
        b = hi.copy(); b[l] = lo[l]
        assert _pairs_rc(gpu_ctx, gpu_ctx, lo, b) == abi.ERR_ARG and _post_rc(gpu_ctx, lo, b) == abi.ERR_ARG      # hi = lo
        b[l] = lo[l] - 0.1
        assert _pairs_rc(gpu_ctx, gpu_ctx, lo, b) == abi.ERR_ARG and _joint_rc(gpu_ctx, lo, b, 0, 1, 3) == abi.ERR_ARG   # hi < lo
    # the other context: another N, another d, another coordinate, another regression order, a Matern model
    TS.fit(second_ctx, order, X[:-1], y[:-1], th)
    assert _pairs_rc(gpu_ctx, second_ctx, lo, hi) == abi.ERR_ARG
    TS.fit(second_ctx, order, X[:, :2], y, TS.thetas(2))
    assert _pairs_rc(gpu_ctx, second_ctx, lo, hi) == abi.ERR_ARG
    X2 = X.copy(); X2[17, 1] = np.nextafter(X2[17, 1], 2.0)
    TS.fit(second_ctx, order, X2, y, th)
    assert _pairs_rc(gpu_ctx, second_ctx, lo, hi) == abi.ERR_ARG and _pairs_rc(second_ctx, gpu_ctx, lo, hi) == abi.ERR_ARG
    assert "design" in L.gpemu_last_error(gpu_ctx.h).decode()
    TS.fit(second_ctx, 2, X, y, th)
    assert _pairs_rc(gpu_ctx, second_ctx, lo, hi) == abi.ERR_ARG
    assert "order" in L.gpemu_last_error(gpu_ctx.h).decode()
    TS.fit(second_ctx, order, X, y, synth.default_thetas(3, d), kind=3)
    assert _pairs_rc(gpu_ctx, second_ctx, lo, hi) == abi.ERR_ARG
    assert "power-exponential covariance only" in L.gpemu_last_error(gpu_ctx.h).decode()
    assert _pairs_rc(second_ctx, second_ctx, lo, hi) == abi.ERR_ARG and _post_rc(second_ctx, lo, hi) == abi.ERR_ARG
    assert _joint_rc(second_ctx, lo, hi, 0, 1, 3) == abi.ERR_ARG
    assert "power-exponential covariance only" in L.gpemu_last_error(second_ctx.h).decode()
    # one parameter: there is no pair
    X1, y1 = TS.data(N, 1)
    TS.fit(second_ctx, order, X1, y1, TS.thetas(1))
    lo1, hi1 = R.boxes(X1)["design"]
    assert _pairs_rc(second_ctx, second_ctx, lo1, hi1) == abi.ERR_ARG and _post_rc(second_ctx, lo1, hi1) == abi.ERR_ARG
    assert _joint_rc(second_ctx, lo1, hi1, 0, 1, 3) == abi.ERR_ARG
    assert "two parameters" in L.gpemu_last_error(second_ctx.h).decode()
    # contexts on different devices: only where there are two
    if L.gpemu_device_count() > 1:
        far = abi.Context(1)
        try:
            TS.fit(far, order, X, y, th)
            assert _pairs_rc(gpu_ctx, far, lo, hi) == abi.ERR_ARG
        finally:
            far.close()
    # a refused call has left everything as it was; a new training vector ends the set-up
    TS.fit(second_ctx, order, X, y, th)
    assert _pairs_rc(gpu_ctx, second_ctx, lo, hi) == abi.OK and _pairs_rc(gpu_ctx, gpu_ctx, lo, hi) == abi.OK
    gpu_ctx.set_training(y + 1.0)
    assert _pairs_rc(gpu_ctx, gpu_ctx, lo, hi) == abi.ERR_STATE and _post_rc(gpu_ctx, lo, hi) == abi.ERR_STATE
    assert _joint_rc(gpu_ctx, lo, hi, 0, 1, 3) == abi.ERR_STATE
