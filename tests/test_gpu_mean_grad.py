"""The gradient of the posterior mean with respect to the query point (gpemu_predict_mean_grad[_dev|_enqueue|_collect],
include/gpemu.h) against tests/meangradref.py: beta and gamma from LAPACK, the clamp mask from the oracle's
k-vector, the weights in numpy -- never the code under test.

Bar: max_j |grad_j - ref_j| <= 1e-8 max(1, max_j |ref_j|) per query, and the 1e-8 mean bar of test_gpu_predict_mean.py for
the returned mean.  meangradref.reference first asserts on the inputs that B N 2^-52 <= 1e-10 (B: its docstring) and that
meanref's A N 2^-52 <= 1e-10, so that rounding in whatever order the sums run stays two orders below the bar.  Every test
prints its largest error (pytest -s).

model(): the inputs of test_gpu_predict_mean.py::small_model.  Measured with meangradref alone, before any device ran,
B N 2^-52 is 5e-14 .. 9e-11 on them except for pow-exp at N = 513 (1.25e-10 at the default nugget e^-4); there the nugget is
raised to e^-3, which gives 5.7e-11 (NUGGET below)."""
import numpy as np
import pytest

import meangradref
import meanref
from madaiemulator_amd import abi, synth
from oracle import oracle as O
from test_gpu_predict_mean import free_hbm, setup, small_model, special_queries

RTOL = meangradref.RTOL
pytestmark = pytest.mark.gpu
NUGGET = {(1, 513): -3.0}


def model(kind, order, N, d):
    X, y, th = small_model(kind, order, N, d)
    if (kind, N) in NUGGET:
        th[1] = NUGGET[(kind, N)]
    return X, y, th


def check(what, got, ref):
    """got = (mean or None, grad), ref = (grad, mean, ...) of meangradref"""
    m, g = got
    gref, mref = ref[0], ref[1]
    assert g.shape == gref.shape and np.all(np.isfinite(g)), what
    err = meangradref.error(g, gref)
    emean = 0.0
    if m is not None:
        assert np.all(np.isfinite(m))
        emean = float(np.max(np.abs(m - mref) / np.maximum(1.0, np.abs(mref))))
    print(f"{what}: max_j |grad - ref| / max(1, |ref|_inf) = {err:.3e}, mean {emean:.3e}  (bar {RTOL:.1e})")
    assert err <= RTOL and emean <= RTOL, (what, err, emean)
    return err


# ------------------------------------------------------------------ 1. ragged N and M
@pytest.mark.parametrize("N", [63, 64, 65, 129, 513])
@pytest.mark.parametrize("kind", [1, 3])
def test_ragged_sizes(gpu_ctx, kind, N):
    """N around the 64-point block, one slice (N <= 256) and three (513, the last one short); M from one query to more than
    three 64-query tiles, each M a call of its own; queries on, 5e-11 from and 2e-10 from a training point among them"""
    d, order = 3, 1
    X, y, th = model(kind, order, N, d)
    Xq = special_queries(X, 200, d, 17)
    ref = meangradref.reference(kind, order, X, y, th, Xq)
    setup(gpu_ctx, kind, order, X, y, th)
    for M in (1, 17, 64, 65, 200):
        check(f"kind {kind} N {N} M {M}", gpu_ctx.predict_mean_grad(Xq[:M]), (ref[0][:M], ref[1][:M]))


# ------------------------------------------------------------------ 2. kinds, orders, dimensions
@pytest.mark.parametrize("kind,order,N,d", [(k, o, 300, 8) for k in (1, 2, 3) for o in (0, 1, 2, 3)] +
                         [(k, 1, 200, dd) for k in (1, 2, 3) for dd in (1, 15, 16, 17)] + [(1, 2, 330, 31), (1, 0, 200, 64)])
def test_kinds_and_orders(gpu_ctx, kind, order, N, d):
    """every covariance function x regression order at d = 8; d = 1 and d = 15, 16, 17 (the edge of the first 16-column
    block of [1 | x']); pow-exp at d = 31 order 2 (63 basis functions, the library's limit) and at d = 64 (five blocks)"""
    X, y, th = model(kind, order, N, d)
    Xq = special_queries(X, 70, d, 5)
    ref = meangradref.reference(kind, order, X, y, th, Xq)
    setup(gpu_ctx, kind, order, X, y, th)
    check(f"kind {kind} order {order} N {N} d {d}", gpu_ctx.predict_mean_grad(Xq), ref)


@pytest.mark.parametrize("kind", [2, 3])
def test_matern_log_mode(kind):
    """GPEMU_MODE_MATERN_LOG: amplitude and nugget on the log scale; the reference runs the literal kernel at their exponentials"""
    N, d, order = 300, 4, 1
    X, y, _ = model(kind, order, N, d)
    th_log = np.array([0.3, -3.0, np.log(0.8)])
    th_raw = np.array([np.exp(0.3), np.exp(-3.0), np.log(0.8)])
    Xq = special_queries(X, 70, d, 9)
    ref = meangradref.reference(kind, order, X, y, th_raw, Xq)
    a, b = abi.Context(0), abi.Context(0)
    try:
        a.set_mode(abi.MODE_MATERN_LOG)
        setup(a, kind, order, X, y, th_log)
        setup(b, kind, order, X, y, th_raw)
        ga, gb = a.predict_mean_grad(Xq), b.predict_mean_grad(Xq)
    finally:
        a.close()
        b.close()
    check(f"kind {kind} log mode", ga, ref)
    check(f"kind {kind} literal mode", gb, ref)
    assert np.array_equal(ga[1], gb[1]) and np.array_equal(ga[0], gb[0])


# ------------------------------------------------------------------ 3. Gram form, difference form, the switch
@pytest.mark.parametrize("kind", [1, 2, 3])
def test_both_forms(monkeypatch, gpu_ctx, kind):
    """the inputs of test_gpu_predict_mean.py::test_both_forms: long length scales (Gram form), length scales so short that
    make_cov_params refuses the Gram form (differences), the long ones again with GPEMU_KVEC_GRAM=0"""
    N, d, order = 330, 3, 1
    X, y, th = model(kind, order, N, d)
    Xq = special_queries(X, 130, d, 23)
    half = 0.5 * (X.max(axis=0) - X.min(axis=0))

    def norm2(t):
        w = np.sqrt(0.5) / np.exp(t[2:]) if kind == 1 else np.full(d, 1.0 / np.exp(t[2]))
        return float(np.sum((w * half) ** 2))

    th_short = th.copy()
    th_short[2:] = np.log(0.1)
    assert norm2(th) <= 16.0 < norm2(th_short)
    ref_long = meangradref.reference(kind, order, X, y, th, Xq)
    ref_short = meangradref.reference(kind, order, X, y, th_short, Xq)
    setup(gpu_ctx, kind, order, X, y, th)
    g_gram = gpu_ctx.predict_mean_grad(Xq)
    check(f"kind {kind} Gram form", g_gram, ref_long)
    setup(gpu_ctx, kind, order, X, y, th_short)
    check(f"kind {kind} short length scales", gpu_ctx.predict_mean_grad(Xq), ref_short)
    monkeypatch.setenv("GPEMU_KVEC_GRAM", "0")            # copied into the context when it is created
    c = abi.Context(0)
    try:
        setup(c, kind, order, X, y, th)
        g_diff = c.predict_mean_grad(Xq)
        # the independence property in the difference form
        alone = c.predict_mean_grad(Xq[50:51])
        Z = Xq.copy()
        Z[129] = Xq[50]
        again = c.predict_mean_grad(Z)
    finally:
        c.close()
    check(f"kind {kind} switch off", g_diff, ref_long)
    assert not np.array_equal(g_diff[1], g_gram[1]), "the switch did not change the form"
    assert np.array_equal(again[1][129], alone[1][0]) and np.array_equal(alone[1][0], g_diff[1][50])
    assert again[0][129] == alone[0][0] == g_diff[0][50]


# ------------------------------------------------------------------ 4. the clamp
def k_unclamped(kind, th, X, x):
    """k values of one query without nugget and clamp, in numpy"""
    D = x - X
    if kind == 1:
        return meangradref.weights(kind, th, D)
    c = meangradref.ROOT3 if kind == 2 else meangradref.ROOT5
    s = np.sqrt(np.sum(D * D, axis=1)) / np.exp(th[2])
    return th[0] * (1.0 + c * s + ((5.0 / 3.0) * s * s if kind == 3 else 0.0)) * np.exp(-c * s)


def clamp_inputs(kind):
    """length scales short enough that part of every k-vector is under the clamp (pow-exp r = 0.06: k < 1e-10 beyond
    |D| = 0.41; Matern rho = 0.03 / 0.035: beyond about 0.45), queries drawn (CPU, fixed seeds) until no value lies within a
    factor 1 +- 1e-6 of 1e-10: the mask then cannot flip by rounding"""
    N, d, order, M = 300, 3, 1, 70
    X, y, th = model(kind, order, N, d)
    th[2:] = np.log({1: 0.06, 2: 0.03, 3: 0.035}[kind])
    for seed in range(101, 120):
        Xq = synth.queries(M, d, seed)
        k = np.vstack([k_unclamped(kind, th, X, x) for x in Xq])
        if np.all(np.abs(k / 1e-10 - 1.0) > 1e-6):
            return X, y, th, Xq, order
    raise AssertionError("no query set keeps clear of the clamp threshold")


@pytest.mark.parametrize("kind", [1, 2, 3])
def test_clamped_part(gpu_ctx, kind):
    X, y, th, Xq, order = clamp_inputs(kind)
    ref = meangradref.reference(kind, order, X, y, th, Xq)
    K = ref[3]
    zero = float(np.mean(K == 0.0))
    print(f"kind {kind}: {100 * zero:.1f} % of the k values are clamped")
    assert 0.1 <= zero <= 0.9
    live = K[K != 0.0]
    assert np.all(np.abs(live / 1e-10 - 1.0) > 1e-6)
    setup(gpu_ctx, kind, order, X, y, th)
    check(f"kind {kind} partly clamped", gpu_ctx.predict_mean_grad(Xq), ref)


# ------------------------------------------------------------------ 5. far queries
@pytest.mark.parametrize("kind", [1, 2, 3])
@pytest.mark.parametrize("gram", [1, 0])
def test_far_queries_give_the_regression_gradient(monkeypatch, kind, gram):
    """the d = 16 inputs of test_gpu_predict_mean.py::test_far_queries_give_the_regression_mean: coordinates of 30 (and 1e4)
    put every k under the clamp; the gradient there is finite and equals sum_a beta_a dh_a/dx_j -- with the beta the set-up
    returned, as that test explains -- to 1e-13"""
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
    ref = meangradref.reference(kind, order, X, y, th, Xq)
    far = [8, 9]
    assert np.all(ref[3][far] == 0.0)
    monkeypatch.setenv("GPEMU_KVEC_GRAM", str(gram))
    c = abi.Context(0)
    try:
        c.set_model(kind, order, X, y)
        beta, rc = c.predict_setup(th)
        assert rc == abi.OK
        got = c.predict_mean_grad(Xq)
    finally:
        c.close()
    check(f"kind {kind} gram {gram} d=16", got, ref)
    assert np.all(np.isfinite(got[1][far]))
    want = np.vstack([meangradref.dbasis(order, Xq[q], beta) for q in far])
    err = float(np.max(np.abs(got[1][far] - want) / np.max(np.abs(want), axis=1, keepdims=True)))
    print(f"kind {kind} gram {gram}: far queries, |grad - sum beta dh| / |.|_inf = {err:.3e}")
    assert err <= 1e-13


# ------------------------------------------------------------------ 6. determinism and independence
def test_same_bits_everywhere(gpu_ctx):
    kind, order, N, d = 3, 1, 513, 3
    X, y, th = model(kind, order, N, d)
    Xq = special_queries(X, 200, d, 77)
    ref = meangradref.reference(kind, order, X, y, th, Xq)
    setup(gpu_ctx, kind, order, X, y, th)
    m1, g1 = gpu_ctx.predict_mean_grad(Xq)
    m2, g2 = gpu_ctx.predict_mean_grad(Xq)
    check("two calls", (m1, g1), ref)
    assert np.array_equal(m1, m2) and np.array_equal(g1, g2)
    # one query alone, as row 0 and as row 137 of a 200-query call (another tile, wave and lane; a far query next to it)
    x = Xq[50]
    ma, ga = gpu_ctx.predict_mean_grad(x[None, :])
    for row in (0, 137):
        Z = Xq.copy()
        Z[row] = x
        Z[(row + 1) % 200] = 40.0
        mz, gz = gpu_ctx.predict_mean_grad(Z)
        assert np.array_equal(gz[row], ga[0]) and np.array_equal(ga[0], g1[50])
        assert mz[row] == ma[0] == m1[50]
    # device-pointer entry and the two halves
    buf = gpu_ctx.dev_alloc(200 * (2 * d + 1) * 8)
    try:
        gpu_ctx.upload(buf, Xq)
        mean_dev, grad_dev = buf.value + 200 * d * 8, buf.value + 200 * (d + 1) * 8
        gpu_ctx.predict_mean_grad_dev(200, buf, mean_dev, grad_dev)
        gpu_ctx.sync()
        md, gd = gpu_ctx.download(mean_dev, (200,)), gpu_ctx.download(grad_dev, (200, d))
    finally:
        gpu_ctx.dev_free(buf)
    assert np.array_equal(md, m1) and np.array_equal(gd, g1)
    gpu_ctx.predict_mean_grad_enqueue(Xq)
    me, ge = gpu_ctx.predict_mean_grad_collect()
    assert np.array_equal(me, m1) and np.array_equal(ge, g1)
    # mean = NULL is accepted and changes nothing in the gradient
    none, gn = gpu_ctx.predict_mean_grad(Xq, want_mean=False)
    assert none is None and np.array_equal(gn, g1)
    gpu_ctx.prof_begin(abi.PROF_MEAN_GRAD)
    gpu_ctx.predict_mean_grad(Xq)
    p = gpu_ctx.prof_end()
    assert p["n"] == 2 and p["ms"] > 0 and p["bytes"] == 8.0 * 200 * (2 * d + 1)


def test_setup_by_batch_same_bits():
    """components through gpemu_predict_setup_batch return the bits of a context set up alone"""
    kind, order, N, d = 1, 1, 321, 3
    X, y, th = small_model(kind, order, N, d, big_nugget=True)
    ys = [y, np.cos(3.0 * y) + 0.5]
    ths = [th, th + 0.05]
    Xq = special_queries(X, 100, d, 3)
    ctxs = [abi.Context(0) for _ in range(2)]
    try:
        for c, yc in zip(ctxs, ys):
            c.set_model(kind, order, X, yc)
        _, _, status, rc = abi.predict_setup_batch(ctxs, np.array(ths))
        assert rc == abi.OK and not status.any()
        for c, yc, tc in zip(ctxs, ys, ths):
            alone = abi.Context(0)
            try:
                setup(alone, kind, order, X, yc, tc)
                ma, ga = alone.predict_mean_grad(Xq)
            finally:
                alone.close()
            ref = meangradref.reference(kind, order, X, yc, tc, Xq)
            mb, gb = c.predict_mean_grad(Xq)
            check("component of a batched set-up", (mb, gb), ref)
            assert np.array_equal(ma, mb) and np.array_equal(ga, gb)
    finally:
        for c in ctxs:
            c.close()


# ------------------------------------------------------------------ 7. state and arguments
def test_state_and_errors():
    kind, order, N, d = 1, 1, 150, 3
    X, y, th = model(kind, order, N, d)
    Xq = special_queries(X, 40, d, 2)
    c = abi.Context(0)
    try:
        c.set_model(kind, order, X, y)
        with pytest.raises(abi.GpemuError) as ei:        # before predict_setup
            c.predict_mean_grad(Xq)
        assert ei.value.code == abi.ERR_STATE
        with pytest.raises(abi.GpemuError) as ei:
            c.predict_mean_grad_enqueue(Xq)
        assert ei.value.code == abi.ERR_STATE
        setup(c, kind, order, X, y, th)
        mv0, vv0 = c.predict(Xq)
        mo0 = c.predict_mean(Xq)
        m0, g0 = c.predict_mean_grad(Xq)
        assert np.array_equal(c.predict_mean(Xq), mo0)   # the mean-only sweep returns the bits it returned before
        check("state test", (m0, g0), meangradref.reference(kind, order, X, y, th, Xq))
        out, gout = np.empty(40), np.empty((40, d))
        dp = abi._p
        L = c.L
        assert L.gpemu_predict_mean_grad(c.h, 40, None, dp(out), dp(gout)) == abi.ERR_ARG
        assert L.gpemu_predict_mean_grad(c.h, 40, dp(Xq), dp(out), None) == abi.ERR_ARG
        assert L.gpemu_predict_mean_grad(c.h, 0, dp(Xq), dp(out), dp(gout)) == abi.ERR_ARG
        assert L.gpemu_predict_mean_grad_enqueue(c.h, 0, dp(Xq)) == abi.ERR_ARG
        assert L.gpemu_predict_mean_grad_enqueue(c.h, 40, None) == abi.ERR_ARG
        assert L.gpemu_predict_mean_grad_collect(c.h, 40, dp(out), None) == abi.ERR_ARG
        assert L.gpemu_predict_mean_grad_dev(c.h, 40, None, None, None) == abi.ERR_ARG
        assert L.gpemu_predict_mean_grad_dev(c.h, 40, 8, None, None) == abi.ERR_ARG
        assert L.gpemu_predict_mean_grad_dev(c.h, 0, 8, 8, 8) == abi.ERR_ARG
        assert L.gpemu_predict_mean_grad_collect(c.h, 40, dp(out), dp(gout)) == abi.ERR_STATE      # nothing enqueued
        # a gradient batch is collected by its own collect only, and stays enqueued until then
        c.predict_mean_grad_enqueue(Xq)
        for other in (c.predict_collect, c.predict_mean_collect):
            with pytest.raises(abi.GpemuError) as ei:
                other()
            assert ei.value.code == abi.ERR_STATE
        for other in (c.predict_enqueue, c.predict_mean_enqueue, c.predict_mean_grad_enqueue):   # one batch of any kind at a time
            with pytest.raises(abi.GpemuError) as ei:
                other(Xq)
            assert ei.value.code == abi.ERR_STATE
        m1, g1 = c.predict_mean_grad_collect()
        assert np.array_equal(m1, m0) and np.array_equal(g1, g0)
        # ... and the other way round, with both other kinds
        c.predict_enqueue(Xq)
        with pytest.raises(abi.GpemuError) as ei:
            c.predict_mean_grad_collect()
        assert ei.value.code == abi.ERR_STATE
        mv1, vv1 = c.predict_collect()
        assert np.array_equal(mv1, mv0) and np.array_equal(vv1, vv0)
        c.predict_mean_enqueue(Xq)
        with pytest.raises(abi.GpemuError) as ei:
            c.predict_mean_grad_collect()
        assert ei.value.code == abi.ERR_STATE
        assert np.array_equal(c.predict_mean_collect(), mo0)
        c.set_training(y + 1.0)                          # the prediction state belongs to the old training vector
        with pytest.raises(abi.GpemuError) as ei:
            c.predict_mean_grad(Xq)
        assert ei.value.code == abi.ERR_STATE
    finally:
        c.close()


# ------------------------------------------------------------------ 8. one internal block and a bit, no batch buffers
def test_block_edge_and_no_big_buffers():
    """M = 16 385 crosses the 16 384-query block: every 97th query and both sides of the edge against the reference; free
    HBM drops by less than ONE of the two batch buffers of gpemu_predict_batch (16 384 x Np doubles) would take at N = 4096,
    checked the way test_gpu_predict_mean.py::test_no_big_buffers checks it (nugget e^2 as there, for the conditioning)"""
    kind, order, N, d = 1, 0, 4096, 8
    X, y = synth.design(N, d, 20261003 + 1)
    th = synth.default_thetas(kind, d)
    th[1] = 2.0
    M = 16385
    Xq = synth.queries(M, d, 12)
    c = abi.Context(0)
    try:
        c.set_model(kind, order, X, y)
        free0 = free_hbm(c)
        _, rc = c.predict_setup(th)
        assert rc == abi.OK
        free1 = free_hbm(c)
        m, g = c.predict_mean_grad(Xq)
        free2 = free_hbm(c)
        print(f"free HBM: before set-up {free0}, after {free1}, after the sweep {free2}")
        assert free0 - free2 < 16384 * 4096 * 8
        assert free1 - free2 < 64 << 20                  # staging and 16 slices x 16 384 x 17 partial sums (36 MB)
        sel = np.unique(np.concatenate([np.arange(0, M, 97), [16382, 16383, 16384]]))
        ref = meangradref.reference(kind, order, X, y, th, Xq[sel])
        check("16 385 queries, every 97th and the block edge", (m[sel], g[sel]), ref)
    finally:
        c.close()
