"""Expected reduction of the IMSE by one more run, in closed form (gpemu_design_gain, include/gpemu.h) through
the public entries, against tests/designref.py (numpy fp64; test_designref.py pins it against mpmath, against quadrature of
c*(x, x*)^2 and against the refit identity).

What is compared.  num is a function of (design, amplitude, lengths, measure, candidates, a, b).  a and b are taken from the
device (gpemu_test_design_state) and var from the call itself: errors are relative to the SCALE, the sum of the absolute values
of the six parts of num (designref.py; divided by var for gain), and another factorisation's a differs from the device's by
far more than the bar.  Everything downstream -- the pair integrals, the three-way sum, the assembly -- is the reference's own,
in another form (the raw Gram form).  That a and b themselves are C^-1 k* + W Q r and Q r is checked against numpy on
gpemu_get_cinverse, and var against gpemu_predict_batch.

The bars.  Measured on the CPU over exactly the cases of this file (`all_cases()`, a and b from a numpy fit in place of the
device's) by `python tests/designref.py --measure`; the device gets FACTOR = 8 times each, as in test_gpu_sens_post.py and for
the same reason: it sums in another order and its erf may differ from libm's by a few ulp per term.
  NP_VS_MP = 5.7e-13  the largest scaled error of the numpy reference against mpmath at 50 digits (N = 64, d = 17, order 3;
                      5.2e-13 on the narrow box; the parts cancel inside -- over all candidates of these cases the sum of the parts is up to
                      1.8e4 times smaller than the sum of their terms' absolute values (N = 64, d = 17, order 3; median
                      390) --, so a few ulp of the terms are this much of the parts; most cases sit at 1e-15 to 5e-14)                                                               -> TOL = 4.6e-12
  REFIT_NP = 5.9e-18  the largest gap |gain - (s_all - s_all')| over the sum of the three values' scales, N + 1 points refitted
                      in numpy (`refit_cases()`)                                                           -> REFIT_TOL = 4.7e-17
  AB_NP    = 1.3e-13  the largest discrepancy of a and b between numpy's inverse and numpy's Cholesky route, on the scales of
                      designref.ab_scales                                                                  -> AB_TOL = 1.0e-12
(see DESIGN.md 4.20)."""
import ctypes as C

import numpy as np
import pytest

import designref as D
import sensref as R
import sensmeasureref as SM
import senspostref as SP
import test_gpu_sens_measure as TM
import test_gpu_sens_post as TP
from madaiemulator_amd import abi, synth

NP_VS_MP = 5.7e-13
REFIT_NP = 5.9e-18
AB_NP = 1.3e-13
FACTOR = 8
TOL = FACTOR * NP_VS_MP
REFIT_TOL = FACTOR * REFIT_NP
AB_TOL = FACTOR * AB_NP
RTOL = 1e-8                      # the project's parity bar (tests/test_gpu_loo.py): where a figure depends on the fit itself
NUGGET = TP.NUGGET

pytestmark = pytest.mark.gpu

NS = [1, 63, 64, 65, 130, 200]
DS = [1, 2, 3, 8, 17]
ORDERS = [0, 1, 2, 3]
MS = [1, 63, 64, 65, 200]
MEASURE_CASES = [(130, 3, 2), (65, 2, 1), (64, 17, 0), (200, 8, 1)]
REFIT_CASES = [(65, 2, 1), (130, 3, 2), (64, 8, 0)]


# ---------------------------------------------------------------------------------------------------- inputs
def shape_cases():
    return [(N, d, o) for N in NS for d in DS for o in ORDERS if 1 + o * d <= N]


def m_of(N, d):
    """every M of MS meets every N and every d somewhere"""
    return MS[(NS.index(N) + DS.index(d)) % len(MS)]


def candidates(X, M, seed=0):
    """M points of the design's range widened by a quarter on either side: inside and outside every box of the tests"""
    lo, hi = R.boxes(X)["design"]
    w = hi - lo
    return (lo - 0.25 * w) + 1.5 * w * np.random.default_rng(4000 + seed + 7 * len(X) + X.shape[1]).random((M, X.shape[1]))


def uniform(d):
    return np.zeros(d, dtype=np.int32)


def all_cases():
    """every (name, X, y, th, order, kind, lo, hi, Xq) whose numbers this file compares with designref at TOL"""
    out = []
    for N, d, o in shape_cases():
        X, y = TP.data(N, d)
        out.append((f"N{N}-d{d}-o{o}", X, y, TP.thetas(d), o, uniform(d)) + R.boxes(X)["design"] + (candidates(X, m_of(N, d)),))
    for box in ("narrow", "disjoint"):
        for o in (0, 2):
            X, y = TP.data(130, 3)
            out.append((f"{box}-o{o}", X, y, TP.thetas(3), o, uniform(3)) + R.boxes(X)[box] + (candidates(X, 65, 1),))
    for N, d, o in MEASURE_CASES:
        for name in ("gauss", "mixed"):
            X, y = TP.data(N, d)
            kind = TM.kinds(name, d)
            out.append((f"{name}-N{N}-d{d}-o{o}", X, y, TP.thetas(d), o, kind) + TM.measure_of(kind, X) + (candidates(X, 64, 2),))
    return out


def far_candidates(X, th, M, seed):
    """candidates at least a tenth of a length scale from every design point (in every metric the lengths define)"""
    ln = np.exp(th[2:])
    Xq = candidates(X, 8 * M, seed)
    dist = np.sqrt((((Xq[:, None, :] - X[None, :, :]) / ln) ** 2).sum(axis=2)).min(axis=1)
    Xq = Xq[dist >= 0.1][:M]
    assert len(Xq) == M
    return Xq


def refit_cases():
    out = []
    for N, d, o in REFIT_CASES:
        X, y = TP.data(N, d)
        th = TP.thetas(d)
        out.append((f"refit-N{N}-d{d}-o{o}", X, y, th, o, uniform(d)) + R.boxes(X)["design"] + (far_candidates(X, th, 3, 3),))
    return out


# ---------------------------------------------------------------------------------------------------- the CPU figures
def _measure_one(case):
    name, X, y, th, o, kind, lo, hi, Xq = case
    m = TP.model_of(th)
    a, b, v, _ = D.fit_ab(X, o, m["A"], m["s"], NUGGET, Xq)
    val, scale, _ = D.gain(R.NP, X, m, lo, hi, kind, Xq, a, b, v)
    mp, _, _ = D.gain(R.MP(), X, m, lo, hi, kind, Xq, a, b, v)
    a2, b2, _ = D.chol_ab(X, o, m["A"], m["s"], NUGGET, Xq)
    sa, sb = D.ab_scales(X, o, m["A"], m["s"], Xq, SP.fit_state(X, np.zeros(len(X)), o, m["A"], m["s"], NUGGET)[5])
    return name, D.scaled_errors(val, mp, scale), max(float(np.max(np.abs(a - a2) / sa)), float(np.max(np.abs(b - b2) / sb)))


def refit_gap_numpy(case):
    name, X, y, th, o, kind, lo, hi, Xq = case
    m = TP.model_of(th)
    a, b, v, _ = D.fit_ab(X, o, m["A"], m["s"], NUGGET, Xq)
    val, scale, _ = D.gain(R.NP, X, m, lo, hi, kind, Xq, a, b, v)
    diff, dscale = D.refit(X, m, o, NUGGET, lo, hi, kind, Xq)
    return float(np.max(np.abs(val["gain"] - diff) / (dscale + scale["gain"])))


def measure():
    """the figures NP_VS_MP, REFIT_NP and AB_NP are set from (CPU, minutes)"""
    import multiprocessing as mpc
    import sys
    cases = sorted(all_cases(), key=lambda c: -c[1].size * len(c[1]))
    if "--only" in sys.argv:
        cases = [c for c in cases if c[0].startswith(tuple(sys.argv[sys.argv.index("--only") + 1].split(",")))]
    worst, worst_ab = ("", 0.0), ("", 0.0)
    with mpc.Pool(min(8, mpc.cpu_count())) as pool:
        for name, e, eab in pool.imap_unordered(_measure_one, cases):
            print(f"{name}: {e:.3e}  a, b routes {eab:.3e}", flush=True)
            if e > worst[1]:
                worst = (name, e)
            if eab > worst_ab[1]:
                worst_ab = (name, eab)
    print(f"largest scaled error of numpy against mpmath over {len(cases)} cases: {worst[1]:.3e} ({worst[0]})")
    print(f"largest discrepancy of the two routes to a and b in numpy: {worst_ab[1]:.3e} ({worst_ab[0]})")
    r = 0.0
    for case in refit_cases():
        g = refit_gap_numpy(case)
        print(f"{case[0]}: refit gap {g:.3e}")
        r = max(r, g)
    print(f"largest refit gap in numpy: {r:.3e}")


# ---------------------------------------------------------------------------------------------------- helpers
def fit(ctx, order, X, y, th, kind=None, model_kind=1):
    m = TP.fit(ctx, order, X, y, th, model_kind)
    ctx.sens_set_measure(kind)                    # (set_model has reset it)
    return m


def run_case(ctx, case, check_ab=True):
    """the case through the host entry against the reference on the device's own a, b and var -> (got, scale, model)"""
    name, X, y, th, o, kind, lo, hi, Xq = case
    m = fit(ctx, o, X, y, th, kind)
    M = len(Xq)
    got = ctx.design_gain(lo, hi, Xq)
    a, b = ctx.design_state(M)
    for k in ("gain", "num", "var"):
        assert np.all(np.isfinite(got[k])), (name, k)
    ref, scale, _ = D.gain(R.NP, X, m, lo, hi, kind, Xq, a, b, got["var"])
    e = D.scaled_errors(got, ref, scale)
    print(f"{name} M {M}: scaled error {e:.2e} (bar {TOL:.1e})")
    assert e < TOL, (name, e)
    if check_ab:
        cinv = ctx.cinverse()
        a_np, b_np, v_np, _ = D.fit_ab(X, o, m["A"], m["s"], NUGGET, Xq, cinv=cinv)
        sa, sb = D.ab_scales(X, o, m["A"], m["s"], Xq, cinv)
        eab = max(float(np.max(np.abs(a - a_np) / sa)), float(np.max(np.abs(b - b_np) / sb)))
        print(f"{name}: a, b against numpy on the device's C^-1 {eab:.2e} (bar {AB_TOL:.1e})")
        assert eab < AB_TOL, (name, eab)
    return got, scale, m


def properties(ctx, case, got, scale):
    """0 <= gain <= s_all of gpemu_sens_post; var is the prediction's variance where the k-vector clamp holds nothing back"""
    name, X, y, th, o, kind, lo, hi, Xq = case
    assert np.all(got["gain"] >= -TOL * scale["gain"]), name
    post = ctx.sens_post(lo, hi)
    P, G, Q = ctx.sens_post_state()
    _, pscale = SM.post(kind, R.NP, X, TP.model_of(th), P, G, Q, lo, hi)
    assert np.all(got["gain"] <= post["s_all"] + TP.TOL * pscale["s_all"] + TOL * scale["gain"]), (name, got["gain"].max(), post["s_all"])
    A, s = np.exp(th[0]), np.exp(-2.0 * th[2:])
    k = A * SP.kmatrix(Xq, X, s)
    unclamped = k.min(axis=1) >= 1e-9
    if unclamped.any():
        _, pv = ctx.predict(Xq)
        assert np.allclose(got["var"][unclamped], pv[unclamped], rtol=RTOL, atol=0), name


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("gain", "num", "var"))


def case_of(N, d, o, M, kind_name=None, seed=5):
    X, y = TP.data(N, d)
    kind = uniform(d) if kind_name is None else TM.kinds(kind_name, d)
    box = R.boxes(X)["design"] if kind_name is None else TM.measure_of(kind, X)
    return (f"N{N}-d{d}-o{o}-M{M}", X, y, TP.thetas(d), o, kind) + box + (candidates(X, M, seed),)


@pytest.fixture(scope="module")
def second_ctx():
    ctx = abi.Context(0)
    yield ctx
    ctx.close()


# ---------------------------------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize("N", NS)
def test_shapes(gpu_ctx, N):
    """one design tile, a ragged second one, four tile columns; one candidate, a ragged tile row, four tile rows; d = 8, 16 < d"""
    for case in all_cases():
        if case[0].startswith(f"N{N}-"):
            got, scale, _ = run_case(gpu_ctx, case)
            properties(gpu_ctx, case, got, scale)


@pytest.mark.parametrize("box", ["narrow", "disjoint"])
def test_boxes(gpu_ctx, box):
    for case in all_cases():
        if case[0].startswith(box):
            got, scale, _ = run_case(gpu_ctx, case)
            properties(gpu_ctx, case, got, scale)


@pytest.mark.parametrize("name", ["gauss", "mixed"])
def test_measures(gpu_ctx, name):
    for case in all_cases():
        if case[0].startswith(name):
            got, scale, _ = run_case(gpu_ctx, case)
            properties(gpu_ctx, case, got, scale)


@pytest.mark.parametrize("i", range(len(REFIT_CASES)))
def test_refit_on_the_device(gpu_ctx, second_ctx, i):
    """gain against s_all of this context minus s_all of a second context on the design with the candidate appended, same thetas"""
    case = refit_cases()[i]
    name, X, y, th, o, kind, lo, hi, Xq = case
    got, scale, m = run_case(gpu_ctx, case, check_ab=False)
    post = gpu_ctx.sens_post(lo, hi)
    _, ps = SP.post(R.NP, X, m, *gpu_ctx.sens_post_state(), lo, hi)
    for q, x in enumerate(Xq):
        X2 = np.vstack([X, x[None, :]])
        fit(second_ctx, o, X2, np.append(y, 0.5), th, kind)
        post2 = second_ctx.sens_post(lo, hi)
        _, ps2 = SP.post(R.NP, X2, m, *second_ctx.sens_post_state(), lo, hi)
        gap = abs(got["gain"][q] - (post["s_all"] - post2["s_all"])) / (ps["s_all"] + ps2["s_all"] + scale["gain"][q])
        print(f"{name} candidate {q}: gain {got['gain'][q]:.6e}, refit {post['s_all'] - post2['s_all']:.6e}, gap {gap:.2e} (bar {REFIT_TOL:.1e})")
        assert gap < REFIT_TOL, (name, q, gap)


def test_a_design_point_gains_least(gpu_ctx):
    """a run repeated on a design point (it only averages the nugget down) gains less than any other candidate of the case.  The
    case is a sparse design, 65 points in 8 dimensions: off the design the posterior variance is far above the nugget (the numpy
    reference gives 1.5e-5 for the design point and 2.1e-4 or more for the others).  On 130 points in 3 dimensions the
    emulator is that sure everywhere, and a candidate in a corner of the box can gain less than a repeat in its middle."""
    name, X, y, th, o, kind, lo, hi, Xq = case_of(65, 8, 1, 64)
    Xq = np.vstack([far_candidates(X, th, 64, 5), X[17][None, :]])
    fit(gpu_ctx, o, X, y, th, kind)
    got = gpu_ctx.design_gain(lo, hi, Xq)
    assert np.all(got["gain"][-1] < got["gain"][:-1]) and got["gain"][-1] >= 0.0


# ---------------------------------------------------------------------------------------------------- 2. bits
def test_block_boundary(gpu_ctx):
    """16 385 candidates: two blocks; the last candidate, alone in the second, has the bits of that point evaluated alone"""
    name, X, y, th, o, kind, lo, hi, Xq = case_of(64, 2, 1, 16385)
    fit(gpu_ctx, o, X, y, th, kind)
    got = gpu_ctx.design_gain(lo, hi, Xq)
    a, b = gpu_ctx.design_state(1)
    alone = gpu_ctx.design_gain(lo, hi, Xq[16384:])
    assert all(np.array_equal(got[k][16384:], alone[k]) for k in got)
    first = gpu_ctx.design_gain(lo, hi, Xq[:64])
    assert all(np.array_equal(got[k][:64], first[k]) for k in got)
    ref, scale, _ = D.gain(R.NP, X, TP.model_of(th), lo, hi, kind, Xq[16384:], a, b, alone["var"])
    assert D.scaled_errors(alone, ref, scale) < TOL
    assert np.all(np.isfinite(got["gain"])) and np.all(got["var"] > 0)


def test_same_bits(gpu_ctx):
    """two calls; the host and the _dev entry; after a change of the box and back, which rebuilds K"""
    name, X, y, th, o, kind, lo, hi, Xq = case_of(130, 8, 1, 65)
    fit(gpu_ctx, o, X, y, th, kind)
    M, d = Xq.shape
    first = gpu_ctx.design_gain(lo, hi, Xq)
    assert same(first, gpu_ctx.design_gain(lo, hi, Xq))
    xq_dev, out_dev = gpu_ctx.dev_alloc(Xq.nbytes), gpu_ctx.dev_alloc(3 * M * 8)
    try:
        gpu_ctx.upload(xq_dev, Xq)
        gpu_ctx.design_gain_dev(lo, hi, M, xq_dev, out_dev, C.c_void_p(out_dev.value + M * 8), C.c_void_p(out_dev.value + 2 * M * 8))
        o3 = gpu_ctx.download(out_dev, (3, M))
        assert same(first, dict(gain=o3[0], num=o3[1], var=o3[2]))
        gpu_ctx.design_gain_dev(lo, hi, M, xq_dev, out_dev)                       # num and var may be left out
        assert np.array_equal(gpu_ctx.download(out_dev, (M,)), first["gain"])
    finally:
        gpu_ctx.dev_free(xq_dev)
        gpu_ctx.dev_free(out_dev)
    nlo, nhi = R.boxes(X)["narrow"]
    other = gpu_ctx.design_gain(nlo, nhi, Xq)
    assert not np.array_equal(other["gain"], first["gain"]) and np.array_equal(other["var"], first["var"])
    assert same(first, gpu_ctx.design_gain(lo, hi, Xq))
    gpu_ctx.sens_set_measure(TM.kinds("mixed", d))                                # the kinds change what K holds too
    mixed = gpu_ctx.design_gain(lo, hi, Xq)
    assert not np.array_equal(mixed["gain"], first["gain"])
    gpu_ctx.sens_set_measure(None)
    assert same(first, gpu_ctx.design_gain(lo, hi, Xq))
    gpu_ctx.sens_release()                                                        # frees K: the next call builds it again
    with pytest.raises(abi.GpemuError) as ei:
        gpu_ctx.design_state(M)
    assert ei.value.code == abi.ERR_STATE
    assert same(first, gpu_ctx.design_gain(lo, hi, Xq))


def test_a_new_setup_rebuilds_what_is_kept(gpu_ctx):
    """other thetas on the same design: nothing of the last set-up's K survives"""
    name, X, y, th, o, kind, lo, hi, Xq = case_of(65, 2, 1, 8)
    fit(gpu_ctx, o, X, y, th, kind)
    first = gpu_ctx.design_gain(lo, hi, Xq)
    th2 = th.copy()
    th2[2:] += 0.2
    fit(gpu_ctx, o, X, y, th2, kind)
    run_case(gpu_ctx, (name, X, y, th2, o, kind, lo, hi, Xq))
    fit(gpu_ctx, o, X, y, th, kind)
    assert same(first, gpu_ctx.design_gain(lo, hi, Xq))


def test_setup_by_batch_same_bits(gpu_ctx):
    """contexts set up by gpemu_predict_setup_batch, component 0 and a later one, against a context set up alone"""
    name, X, y, th, o, kind, lo, hi, Xq = case_of(130, 3, 1, 65)
    ys = [y, 0.5 * y + X[:, 0], y * y]
    ctxs = [abi.Context(0) for _ in ys]
    try:
        for c, yc in zip(ctxs, ys):
            c.set_model(1, o, X, yc)
        _, _, status, rc = abi.predict_setup_batch(ctxs, np.tile(th, (len(ys), 1)))
        assert rc == abi.OK and np.all(status == abi.OK)
        fit(gpu_ctx, o, X, y, th, kind)
        alone = gpu_ctx.design_gain(lo, hi, Xq)                                   # (the gain does not depend on the training values)
        for c in (ctxs[0], ctxs[2]):
            assert same(alone, c.design_gain(lo, hi, Xq))
    finally:
        for c in ctxs:
            c.close()


# ---------------------------------------------------------------------------------------------------- 3. neighbours
def test_a_pending_batch_stays_collectable(gpu_ctx):
    name, X, y, th, o, kind, lo, hi, Xq = case_of(130, 3, 1, 65)
    fit(gpu_ctx, o, X, y, th, kind)
    mean, var = gpu_ctx.predict(Xq)
    gpu_ctx.predict_enqueue(Xq)
    got = gpu_ctx.design_gain(lo, hi, Xq[:7])
    m2, v2 = gpu_ctx.predict_collect()
    assert np.array_equal(mean, m2) and np.array_equal(var, v2)
    assert same(got, gpu_ctx.design_gain(lo, hi, Xq[:7]))


def test_neighbours_keep_their_bits(gpu_ctx):
    """gpemu_sens_post and gpemu_predict_var_grad return the bits they returned before the call"""
    name, X, y, th, o, kind, lo, hi, Xq = case_of(130, 3, 2, 65)
    fit(gpu_ctx, o, X, y, th, kind)
    post, vg = gpu_ctx.sens_post(lo, hi), gpu_ctx.predict_var_grad(Xq)
    gpu_ctx.design_gain(lo, hi, Xq)
    post2, vg2 = gpu_ctx.sens_post(lo, hi), gpu_ctx.predict_var_grad(Xq)
    assert TP.same_bits(post, post2)
    assert all(np.array_equal(p, q) for p, q in zip(vg, vg2))


# ---------------------------------------------------------------------------------------------------- 4. errors
def test_errors(gpu_ctx, second_ctx):
    name, X, y, th, o, kind, lo, hi, Xq = case_of(65, 2, 1, 5)
    L, p, M = gpu_ctx.L, abi._p, len(Xq)
    lo, hi, Xq = (np.ascontiguousarray(v, dtype=np.float64) for v in (lo, hi, Xq))
    out = np.empty(M)
    fit(gpu_ctx, o, X, y, th, kind)
    h = gpu_ctx.h
    # NULL pointers and npoints < 1: whatever the state
    second_ctx.set_model(1, o, X, y)                                              # a model, no set-up
    for ctx_h in (h, second_ctx.h):
        assert L.gpemu_design_gain(ctx_h, None, p(hi), M, p(Xq), p(out), None, None) == abi.ERR_ARG
        assert L.gpemu_design_gain(ctx_h, p(lo), None, M, p(Xq), p(out), None, None) == abi.ERR_ARG
        assert L.gpemu_design_gain(ctx_h, p(lo), p(hi), M, None, p(out), None, None) == abi.ERR_ARG
        assert L.gpemu_design_gain(ctx_h, p(lo), p(hi), M, p(Xq), None, None, None) == abi.ERR_ARG
        assert L.gpemu_design_gain(ctx_h, p(lo), p(hi), 0, p(Xq), p(out), None, None) == abi.ERR_ARG
        assert L.gpemu_design_gain_dev(ctx_h, p(lo), p(hi), M, None, None, None, None) == abi.ERR_ARG
    assert L.gpemu_design_gain(None, p(lo), p(hi), M, p(Xq), p(out), None, None) == abi.ERR_ARG
    # no prediction set-up
    assert L.gpemu_design_gain(second_ctx.h, p(lo), p(hi), M, p(Xq), p(out), None, None) == abi.ERR_STATE
    assert L.gpemu_design_gain_dev(second_ctx.h, p(lo), p(hi), M, C.c_void_p(8), C.c_void_p(8), None, None) == abi.ERR_STATE
    a, b = np.empty((M, 65)), np.empty((M, 3))
    assert L.gpemu_test_design_state(second_ctx.h, M, p(a), p(b)) == abi.ERR_STATE
    # a Matern model
    second_ctx.set_model(3, o, X, y)
    _, rc = second_ctx.predict_setup(synth.default_thetas(3, 2))
    assert rc == abi.OK
    assert L.gpemu_design_gain(second_ctx.h, p(lo), p(hi), M, p(Xq), p(out), None, None) == abi.ERR_ARG
    # a bad box, a Gaussian coordinate without a spread
    bad = hi.copy()
    bad[1] = lo[1]
    assert L.gpemu_design_gain(h, p(lo), p(bad), M, p(Xq), p(out), None, None) == abi.ERR_ARG
    bad[1] = np.inf
    assert L.gpemu_design_gain(h, p(lo), p(bad), M, p(Xq), p(out), None, None) == abi.ERR_ARG
    gpu_ctx.sens_set_measure([0, 1])
    for sd in (0.0, -1.0, np.nan):
        bad = hi.copy()
        bad[1] = sd
        assert L.gpemu_design_gain(h, p(lo), p(bad), M, p(Xq), p(out), None, None) == abi.ERR_ARG
    gpu_ctx.sens_set_measure(None)
    # and the entry works after all that; the state of another block size is refused
    got = gpu_ctx.design_gain(lo, hi, Xq)
    assert np.all(np.isfinite(got["gain"]))
    assert L.gpemu_test_design_state(h, M + 1, p(np.empty((M + 1, 65))), p(np.empty((M + 1, 3)))) == abi.ERR_STATE
    assert L.gpemu_test_design_state(h, M, None, p(b)) == abi.ERR_ARG
