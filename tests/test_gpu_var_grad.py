"""Mean, variance and the variance's gradient with respect to the query point (gpemu_predict_var_grad[_dev|_enqueue|_collect],
include/gpemu.h) against tests/vargradref.py: C^-1 k, W, Q from LAPACK, the clamp mask from the oracle's
k-vector, the weights in numpy -- never the code under test.

Bars: max_j |grad_j - ref_j| <= 1e-8 max(kappa, max_j |ref_j|) per query; |mean - ref| <= 1e-8 max(1, |ref|);
|var - ref| <= 1e-8 kappa (a far query, whose variance grows with |h|: 1e-8 max(kappa, |ref|), as test_gpu_predict_paths.py).
This gradient goes through C^-1 k, so every comparison first has vargradref.reference assert that the float64 reference
itself agrees with its extended-precision repeat to 1e-10 in the same measures (and meanref's A N 2^-52 <= 1e-10 for the
mean).  Every test prints its largest errors (pytest -s).

model(): the inputs of test_gpu_mean_grad.py::model, its raised nugget for pow-exp at N = 513 (e^-3, which the mean's
precondition needs) included.  The reference's own error on every input below, measured on the CPU before any device ran
(gradient / variance against the extended-precision repeat, then A N 2^-52; all three must be <= 1e-10):
  ragged sizes, d = 3                  up to 1.4e-14 / 3.2e-15 / 4.3e-11
  kinds x orders, N = 300, d = 8       up to 3.2e-14 / 2.0e-15 / 1.2e-11
  d = 1, 15, 16, 17, N = 200           up to 8.0e-15 / 1.1e-15 / 2.5e-11
  pow-exp d = 31 order 2; d = 64       6.3e-14 / 1.4e-14 / 4.4e-14;  1.4e-20 / 4.4e-16 / 2.4e-14
  Matern log mode; both forms          9.1e-15 / 1.3e-15 / 1.9e-11;  2.0e-14 / 1.4e-15 / 4.2e-11
  partly clamped; far queries, d = 16  1.6e-15 / 4.3e-16 / 6.9e-14;  6.0e-14 / 1.5e-11 / 3.1e-13
  new set-ups; entries; errors; block  up to 1.3e-14 / 1.3e-15 / 3.5e-11
so no case needed a nugget of its own beyond that table.  (A second training vector cos(2 y) + 1.5 for the new-set-up tests
gave A N 2^-52 = 2.1e-10; they use 0.5 y + 1: 9.7e-12.)

Measured on an MI355X, largest error per group, gradient / mean / variance (bars 1e-8): ragged N x M 2.5e-14 / 7.5e-14 /
3.0e-15; kinds x orders at d = 8 3.8e-14 / 1.7e-13 / 4.0e-15; d in {1, 15, 16, 17} 1.9e-14 / 4.5e-14 / 1.3e-15; d = 31 order 2
7.2e-14 / 4.1e-13 / 1.3e-14; d = 64 4.4e-15 / 8.5e-16 / 1.7e-15; Matern log mode 1.3e-14 / 4.8e-14 / 2.4e-15; Gram form 3.1e-14,
short length scales 3.5e-13, GPEMU_KVEC_GRAM=0 2.8e-14; partly clamped (77 - 82 % zero) 1.4e-14; d = 16 with far queries
6.7e-14 / 4.1e-14 / 4.5e-11, the far queries against 2 h^T Q dh 6.7e-14; new set-ups 1.6e-14; entries 2.5e-14; M = 16 385
1.4e-14."""
import numpy as np
import pytest

import vargradref
from madaiemulator_amd import abi, synth
from test_gpu_mean_grad import NUGGET, clamp_inputs, model  # noqa: F401  (NUGGET: the table model() applies)
from test_gpu_predict_mean import setup, special_queries

RTOL = vargradref.RTOL
pytestmark = pytest.mark.gpu


def check(what, got, ref, sel=slice(None), far=()):
    """got = (mean or None, var or None, grad); ref: vargradref's dict; sel: the rows of ref that got holds"""
    m, v, g = got
    gref, mref, vref, vs = ref["grad"][sel], ref["mean"][sel], ref["var"][sel], ref["vscale"][sel]
    assert g.shape == gref.shape and np.all(np.isfinite(g)), what
    err = vargradref.error(g, gref, ref["kappa"])
    emean = evar = 0.0
    if m is not None:
        assert np.all(np.isfinite(m))
        emean = float(np.max(np.abs(m - mref) / np.maximum(1.0, np.abs(mref))))
    if v is not None:
        assert np.all(np.isfinite(v))
        evar = float(np.max(np.abs(v - vref) / vs))
    print(f"{what}: grad {err:.3e} of max(kappa, |ref|_inf), mean {emean:.3e}, var {evar:.3e} of kappa  (bars {RTOL:.1e})")
    assert err <= RTOL and emean <= RTOL and evar <= RTOL, (what, err, emean, evar)
    return err


# ------------------------------------------------------------------ 1. ragged N and M
RAGGED = [(kind, N) for kind in (1, 3) for N in (63, 64, 65, 129, 513)]


def ragged_inputs(kind, N):
    d, order = 3, 1
    X, y, th = model(kind, order, N, d)
    return kind, order, X, y, th, special_queries(X, 200, d, 17)


@pytest.mark.parametrize("kind,N", RAGGED)
def test_ragged_sizes(gpu_ctx, kind, N):
    """N around the 64-point block, one slice (N <= 256) and three (513, the last one short); M from one query to more than
    three 64-query tiles, each M a call of its own; queries on, 5e-11 from and 2e-10 from a training point among them."""
    kind, order, X, y, th, Xq = ragged_inputs(kind, N)
    ref = vargradref.reference(kind, order, X, y, th, Xq)
    setup(gpu_ctx, kind, order, X, y, th)
    for M in (1, 17, 64, 65, 200):
        check(f"kind {kind} N {N} M {M}", gpu_ctx.predict_var_grad(Xq[:M]), ref, slice(0, M))


# ------------------------------------------------------------------ 2. kinds, orders, dimensions
KINDS_ORDERS = ([(k, o, 300, 8) for k in (1, 2, 3) for o in (0, 1, 2, 3)] + [(k, 1, 200, dd) for k in (1, 2, 3) for dd in (1, 15, 16, 17)] +
                [(1, 2, 330, 31), (1, 0, 200, 64)])


def kinds_inputs(kind, order, N, d):
    X, y, th = model(kind, order, N, d)
    return kind, order, X, y, th, special_queries(X, 70, d, 5)


@pytest.mark.parametrize("kind,order,N,d", KINDS_ORDERS)
def test_kinds_and_orders(gpu_ctx, kind, order, N, d):
    """every covariance function x regression order at d = 8; d = 1 and d = 15, 16, 17 (the edge of the first 16-column
    block of [1 | x']); pow-exp at d = 31 order 2 (63 basis functions: every W^T column of the second product in use) and at
    d = 64 (five column blocks)."""
    kind, order, X, y, th, Xq = kinds_inputs(kind, order, N, d)
    ref = vargradref.reference(kind, order, X, y, th, Xq)
    setup(gpu_ctx, kind, order, X, y, th)
    check(f"kind {kind} order {order} N {N} d {d}", gpu_ctx.predict_var_grad(Xq), ref)


def log_mode_inputs(kind):
    N, d, order = 300, 4, 1
    X, y, _ = model(kind, order, N, d)
    return kind, order, X, y, np.array([np.exp(0.3), np.exp(-3.0), np.log(0.8)]), special_queries(X, 70, d, 9)


@pytest.mark.parametrize("kind", [2, 3])
def test_matern_log_mode(kind):
    """GPEMU_MODE_MATERN_LOG: amplitude and nugget on the log scale; the reference runs the literal kernel at their
    exponentials; the two modes return the same bits"""
    kind, order, X, y, th_raw, Xq = log_mode_inputs(kind)
    th_log = np.array([0.3, -3.0, np.log(0.8)])
    ref = vargradref.reference(kind, order, X, y, th_raw, Xq)
    a, b = abi.Context(0), abi.Context(0)
    try:
        a.set_mode(abi.MODE_MATERN_LOG)
        setup(a, kind, order, X, y, th_log)
        setup(b, kind, order, X, y, th_raw)
        ga, gb = a.predict_var_grad(Xq), b.predict_var_grad(Xq)
    finally:
        a.close()
        b.close()
    check(f"kind {kind} log mode", ga, ref)
    check(f"kind {kind} literal mode", gb, ref)
    for u, w in zip(ga, gb):
        assert np.array_equal(u, w)


# ------------------------------------------------------------------ 3. Gram form, difference form, the switch
def forms_inputs(kind):
    N, d, order = 330, 3, 1
    X, y, th = model(kind, order, N, d)
    th_short = th.copy()
    th_short[2:] = np.log(0.1)
    return kind, order, X, y, th, th_short, special_queries(X, 130, d, 23)


@pytest.mark.parametrize("kind", [1, 2, 3])
def test_both_forms(monkeypatch, gpu_ctx, kind):
    """the inputs of test_gpu_mean_grad.py::test_both_forms: long length scales (Gram form), length scales so short that
    make_cov_params refuses the Gram form (differences), the long ones again with GPEMU_KVEC_GRAM=0."""
    kind, order, X, y, th, th_short, Xq = forms_inputs(kind)
    d = X.shape[1]
    half = 0.5 * (X.max(axis=0) - X.min(axis=0))

    def norm2(t):
        w = np.sqrt(0.5) / np.exp(t[2:]) if kind == 1 else np.full(d, 1.0 / np.exp(t[2]))
        return float(np.sum((w * half) ** 2))

    assert norm2(th) <= 16.0 < norm2(th_short)
    ref_long = vargradref.reference(kind, order, X, y, th, Xq)
    ref_short = vargradref.reference(kind, order, X, y, th_short, Xq)
    setup(gpu_ctx, kind, order, X, y, th)
    g_gram = gpu_ctx.predict_var_grad(Xq)
    check(f"kind {kind} Gram form", g_gram, ref_long)
    setup(gpu_ctx, kind, order, X, y, th_short)
    check(f"kind {kind} short length scales", gpu_ctx.predict_var_grad(Xq), ref_short)
    monkeypatch.setenv("GPEMU_KVEC_GRAM", "0")            # copied into the context when it is created
    c = abi.Context(0)
    try:
        setup(c, kind, order, X, y, th)
        g_diff = c.predict_var_grad(Xq)
    finally:
        c.close()
    check(f"kind {kind} switch off", g_diff, ref_long)
    assert not np.array_equal(g_diff[2], g_gram[2]), "the switch did not change the form"


# ------------------------------------------------------------------ 4. the clamp
@pytest.mark.parametrize("kind", [1, 2, 3])
def test_clamped_part(gpu_ctx, kind):
    """the inputs of test_gpu_mean_grad.py::test_clamped_part: 10 .. 90 % of every k-vector under the clamp, no value within
    1 +- 1e-6 of the threshold."""
    X, y, th, Xq, order = clamp_inputs(kind)
    ref = vargradref.reference(kind, order, X, y, th, Xq)
    zero = float(np.mean(ref["K"] == 0.0))
    print(f"kind {kind}: {100 * zero:.1f} % of the k values are clamped")
    assert 0.1 <= zero <= 0.9
    setup(gpu_ctx, kind, order, X, y, th)
    check(f"kind {kind} partly clamped", gpu_ctx.predict_var_grad(Xq), ref)


# ------------------------------------------------------------------ 5. far queries
FAR = [8, 9]


def far_inputs(kind):
    N, d, M, order = 200, 16, 70, 2
    X, y = synth.design(N, d, 31 + N)
    th = synth.default_thetas(kind, d)
    Xq = synth.queries(M, d, 6)
    Xq[3] = X[5]
    Xq[5] = X[7] + 5e-11
    Xq[6] = X[9] + 3.0
    Xq[8] = 30.0
    Xq[9] = 1.0e4
    Xq[M - 1] = X[0]
    return kind, order, X, y, th, Xq


@pytest.mark.parametrize("kind", [1, 2, 3])
@pytest.mark.parametrize("gram", [1, 0])
def test_far_queries_give_the_regression_gradient(monkeypatch, kind, gram):
    """the d = 16 inputs of test_gpu_mean_grad.py's far-query test: coordinates of 30 (and 1e4) put every k under the clamp;
    r = h there and the gradient is 2 h^T Q dh/dx_j, worked out here in numpy from LAPACK's Q without any k or weight.
    The bar is the gradient's own (Q carries the rounding of C^-1 H like everything else)."""
    import scipy.linalg as sl
    from oracle import oracle as O
    kind, order, X, y, th, Xq = far_inputs(kind)
    d = X.shape[1]
    ref = vargradref.reference(kind, order, X, y, th, Xq, far=FAR)
    assert np.all(ref["K"][FAR] == 0.0)
    H = O.hmatrix(order, X)
    Q = np.linalg.inv(H.T @ sl.cho_solve(sl.cho_factor(O.cov_matrix(kind, X, th), lower=True), H))
    hq = O.hmatrix(order, Xq[FAR]) @ Q.T
    want = 2.0 * vargradref.dbasis_rows(order, Xq[FAR], hq)
    assert vargradref.error(ref["grad"][FAR], want, ref["kappa"]) <= 1e-12
    monkeypatch.setenv("GPEMU_KVEC_GRAM", str(gram))
    c = abi.Context(0)
    try:
        setup(c, kind, order, X, y, th)
        got = c.predict_var_grad(Xq)
    finally:
        c.close()
    check(f"kind {kind} gram {gram} d=16", got, ref, far=FAR)
    err = vargradref.error(got[2][FAR], want, ref["kappa"])
    print(f"kind {kind} gram {gram}: far queries, |grad - 2 h^T Q dh| / |.|_inf = {err:.3e}")
    assert err <= RTOL


# ------------------------------------------------------------------ 6. the transposed copy follows the prediction state
def stale_inputs():
    kind, order, N, d = 3, 1, 200, 3
    X, y, th = model(kind, order, N, d)
    th2 = th.copy()
    th2[0], th2[2] = 1.7, th[2] + 0.3
    return kind, order, X, y, th, th2, 0.5 * y + 1.0, special_queries(X, 70, d, 41)


def test_new_setup_rebuilds_the_transposed_copy():
    """set up at theta_1, call, set up at theta_2, call: the second answer is theta_2's (a stale transposed copy of L^-1 would
    give theta_1's a); the same with a new training vector and a new set-up."""
    kind, order, X, y, th1, th2, y2, Xq = stale_inputs()
    ref1 = vargradref.reference(kind, order, X, y, th1, Xq)
    ref2 = vargradref.reference(kind, order, X, y, th2, Xq)
    ref3 = vargradref.reference(kind, order, X, y2, th2, Xq)
    assert vargradref.error(ref1["grad"], ref2["grad"], ref2["kappa"]) > 1e-3     # the two states are told apart
    c = abi.Context(0)
    try:
        setup(c, kind, order, X, y, th1)
        check("theta_1", c.predict_var_grad(Xq), ref1)
        _, rc = c.predict_setup(th2)
        assert rc == abi.OK
        check("theta_2 after theta_1", c.predict_var_grad(Xq), ref2)
        c.set_training(y2)
        with pytest.raises(abi.GpemuError) as ei:        # the prediction state belonged to the old training vector
            c.predict_var_grad(Xq)
        assert ei.value.code == abi.ERR_STATE
        _, rc = c.predict_setup(th2)
        assert rc == abi.OK
        check("new training vector", c.predict_var_grad(Xq), ref3)
    finally:
        c.close()


def test_setup_by_batch_rebuilds_the_transposed_copy():
    """two contexts through gpemu_predict_setup_batch, a call on each, a second batched set-up at other thetas, a call on
    each: the second context's answers are those of its new state, and the bits of a context set up alone"""
    kind, order, X, y, th1, th2, y2, Xq = stale_inputs()
    ys = [y, y2]
    ctxs = [abi.Context(0) for _ in range(2)]
    try:
        for c, yc in zip(ctxs, ys):
            c.set_model(kind, order, X, yc)
        for ths in ([th1, th2], [th2, th1]):
            _, _, status, rc = abi.predict_setup_batch(ctxs, np.array(ths))
            assert rc == abi.OK and not status.any()
            for c, yc, tc in zip(ctxs, ys, ths):
                got = c.predict_var_grad(Xq)
                check("component of a batched set-up", got, vargradref.reference(kind, order, X, yc, tc, Xq))
                alone = abi.Context(0)
                try:
                    setup(alone, kind, order, X, yc, tc)
                    want = alone.predict_var_grad(Xq)
                finally:
                    alone.close()
                for u, w in zip(got, want):
                    assert np.array_equal(u, w)
    finally:
        for c in ctxs:
            c.close()


# ------------------------------------------------------------------ 7. entries, shared buffers, state and arguments
def entries_inputs():
    kind, order, N, d = 3, 1, 513, 3
    X, y, th = model(kind, order, N, d)
    return kind, order, X, y, th, special_queries(X, 200, d, 77)


def test_same_bits_everywhere(gpu_ctx):
    """two calls, the device-pointer entry (with and without mean / variance), the two halves, NULL outputs; and the batch
    buffers it shares: gpemu_predict_batch and gpemu_predict_mean_grad return the bits they returned before"""
    kind, order, X, y, th, Xq = entries_inputs()
    d, M = X.shape[1], Xq.shape[0]
    ref = vargradref.reference(kind, order, X, y, th, Xq)
    setup(gpu_ctx, kind, order, X, y, th)
    pm0, pv0 = gpu_ctx.predict(Xq)
    gm0, gg0 = gpu_ctx.predict_mean_grad(Xq)
    m1, v1, g1 = gpu_ctx.predict_var_grad(Xq)
    m2, v2, g2 = gpu_ctx.predict_var_grad(Xq)
    check("two calls", (m1, v1, g1), ref)
    assert np.array_equal(m1, m2) and np.array_equal(v1, v2) and np.array_equal(g1, g2)
    pm1, pv1 = gpu_ctx.predict(Xq)
    gm1, gg1 = gpu_ctx.predict_mean_grad(Xq)
    assert np.array_equal(pm0, pm1) and np.array_equal(pv0, pv1) and np.array_equal(gm0, gm1) and np.array_equal(gg0, gg1)
    # to rounding, not bit for bit, the mean and variance of gpemu_predict_batch
    assert np.max(np.abs(m1 - pm0) / np.maximum(1.0, np.abs(pm0))) <= RTOL and np.max(np.abs(v1 - pv0)) <= RTOL * ref["kappa"]
    buf = gpu_ctx.dev_alloc(M * (2 * d + 2) * 8)
    try:
        gpu_ctx.upload(buf, Xq)
        mean_dev, var_dev, grad_dev = buf.value + M * d * 8, buf.value + M * (d + 1) * 8, buf.value + M * (d + 2) * 8
        gpu_ctx.predict_var_grad_dev(M, buf, mean_dev, var_dev, grad_dev)
        gpu_ctx.sync()
        md, vd, gd = gpu_ctx.download(mean_dev, (M,)), gpu_ctx.download(var_dev, (M,)), gpu_ctx.download(grad_dev, (M, d))
        assert np.array_equal(md, m1) and np.array_equal(vd, v1) and np.array_equal(gd, g1)
        gpu_ctx.upload(grad_dev, np.zeros((M, d)))
        gpu_ctx.predict_var_grad_dev(M, buf, None, None, grad_dev)
        gpu_ctx.sync()
        assert np.array_equal(gpu_ctx.download(grad_dev, (M, d)), g1)
        assert np.array_equal(gpu_ctx.download(mean_dev, (M,)), m1)        # untouched
    finally:
        gpu_ctx.dev_free(buf)
    gpu_ctx.predict_var_grad_enqueue(Xq)
    me, ve, ge = gpu_ctx.predict_var_grad_collect()
    assert np.array_equal(me, m1) and np.array_equal(ve, v1) and np.array_equal(ge, g1)
    none_m, none_v, gn = gpu_ctx.predict_var_grad(Xq, want_mean=False, want_var=False)
    assert none_m is None and none_v is None and np.array_equal(gn, g1)
    _, vo, go = gpu_ctx.predict_var_grad(Xq, want_mean=False)
    assert np.array_equal(vo, v1) and np.array_equal(go, g1)
    gpu_ctx.prof_begin(abi.PROF_VAR_GRAD)
    gpu_ctx.predict_var_grad(Xq)
    p = gpu_ctx.prof_end()
    assert p["n"] == 2 and p["ms"] > 0


def test_state_and_errors():
    kind, order, N, d = 1, 1, 150, 3
    X, y, th = model(kind, order, N, d)
    Xq = special_queries(X, 40, d, 2)
    c = abi.Context(0)
    try:
        c.set_model(kind, order, X, y)
        for call in (c.predict_var_grad, c.predict_var_grad_enqueue):       # before predict_setup
            with pytest.raises(abi.GpemuError) as ei:
                call(Xq)
            assert ei.value.code == abi.ERR_STATE
        setup(c, kind, order, X, y, th)
        m0, v0, g0 = c.predict_var_grad(Xq)
        check("state test", (m0, v0, g0), vargradref.reference(kind, order, X, y, th, Xq))
        out, vout, gout = np.empty(40), np.empty(40), np.empty((40, d))
        dp, L = abi._p, c.L
        assert L.gpemu_predict_var_grad(c.h, 40, None, dp(out), dp(vout), dp(gout)) == abi.ERR_ARG
        assert L.gpemu_predict_var_grad(c.h, 40, dp(Xq), dp(out), dp(vout), None) == abi.ERR_ARG
        assert L.gpemu_predict_var_grad(c.h, 0, dp(Xq), dp(out), dp(vout), dp(gout)) == abi.ERR_ARG
        assert L.gpemu_predict_var_grad(c.h, -3, dp(Xq), dp(out), dp(vout), dp(gout)) == abi.ERR_ARG
        assert L.gpemu_predict_var_grad_enqueue(c.h, 0, dp(Xq)) == abi.ERR_ARG
        assert L.gpemu_predict_var_grad_enqueue(c.h, 40, None) == abi.ERR_ARG
        assert L.gpemu_predict_var_grad_collect(c.h, 40, dp(out), dp(vout), None) == abi.ERR_ARG
        assert L.gpemu_predict_var_grad_dev(c.h, 40, None, None, None, None) == abi.ERR_ARG
        assert L.gpemu_predict_var_grad_dev(c.h, 40, 8, None, None, None) == abi.ERR_ARG
        assert L.gpemu_predict_var_grad_dev(c.h, 0, 8, 8, 8, 8) == abi.ERR_ARG
        assert L.gpemu_predict_var_grad_collect(c.h, 40, dp(out), dp(vout), dp(gout)) == abi.ERR_STATE     # nothing enqueued
        assert L.gpemu_predict_var_grad(c.h, 40, dp(Xq), None, None, dp(gout)) == abi.OK                    # NULL mean and var
        assert np.array_equal(gout, g0)
        # a variance-gradient batch is collected by its own collect only, and stays enqueued until then
        c.predict_var_grad_enqueue(Xq)
        for other in (c.predict_collect, c.predict_mean_collect, c.predict_mean_grad_collect):
            with pytest.raises(abi.GpemuError) as ei:
                other()
            assert ei.value.code == abi.ERR_STATE
        for other in (c.predict_enqueue, c.predict_mean_enqueue, c.predict_mean_grad_enqueue, c.predict_var_grad_enqueue):
            with pytest.raises(abi.GpemuError) as ei:    # one batch of any kind at a time
                other(Xq)
            assert ei.value.code == abi.ERR_STATE
        m1, v1, g1 = c.predict_var_grad_collect()
        assert np.array_equal(m1, m0) and np.array_equal(v1, v0) and np.array_equal(g1, g0)
        # ... and the other way round, with the three other kinds
        for enq, col in ((c.predict_enqueue, c.predict_collect), (c.predict_mean_enqueue, c.predict_mean_collect),
                         (c.predict_mean_grad_enqueue, c.predict_mean_grad_collect)):
            enq(Xq)
            want = col()
            enq(Xq)
            with pytest.raises(abi.GpemuError) as ei:
                c.predict_var_grad_collect()
            assert ei.value.code == abi.ERR_STATE
            got = col()
            for u, w in zip(got if isinstance(got, tuple) else (got,), want if isinstance(want, tuple) else (want,)):
                assert np.array_equal(u, w)
        c.set_training(y + 1.0)                          # the prediction state belongs to the old training vector
        with pytest.raises(abi.GpemuError) as ei:
            c.predict_var_grad(Xq)
        assert ei.value.code == abi.ERR_STATE
    finally:
        c.close()


# ------------------------------------------------------------------ 8. one internal block and a bit
def block_inputs():
    kind, order, N, d = 3, 1, 129, 3
    X, y, th = model(kind, order, N, d)
    M = 16385
    Xq = synth.queries(M, d, 12)
    sel = np.unique(np.concatenate([np.arange(0, M, 97), [16382, 16383, 16384]]))
    return kind, order, X, y, th, Xq, sel


def test_block_edge():
    """M = 16 385 crosses the 16 384-query block and the second block holds one query: every 97th query and both sides of
    the edge against the reference."""
    kind, order, X, y, th, Xq, sel = block_inputs()
    ref = vargradref.reference(kind, order, X, y, th, Xq[sel])
    c = abi.Context(0)
    try:
        setup(c, kind, order, X, y, th)
        m, v, g = c.predict_var_grad(Xq)
        assert np.all(np.isfinite(g)) and np.all(np.isfinite(m)) and np.all(np.isfinite(v))
        check("16 385 queries, every 97th and the block edge", (m[sel], v[sel], g[sel]), ref)
    finally:
        c.close()
