"""The mean-only prediction sweep (gpemu_predict_mean[_dev|_enqueue|_collect], include/gpemu.h): the fused k-vector . gamma
kernel against an independent reference -- tests/meanref.py: h^T beta + k^T gamma from the oracle's covariance values (clamp
included) and LAPACK solves; never the code under test.

Bar: |mean - ref| <= RTOL * max(1, |ref|) per query, RTOL = 1e-8 (the project's prediction bar).  Every comparison first
asserts on its inputs that A * N * 2^-52 <= 1e-10 with A = sum_i |k_i gamma_i| / max(1, |mean|) (meanref.reference), so that
rounding in whatever order the N products are added stays two orders below the bar."""
import os

import numpy as np
import pytest

import meanref
from madaiemulator_amd import abi, synth
from oracle import oracle as O

RTOL = meanref.RTOL
pytestmark = pytest.mark.gpu


def small_model(kind, order, N, d, big_nugget=False):
    """the inputs of test_gpu_loo.py::small_model.  big_nugget: where the default hyper-parameters miss the precondition
    A N 2^-52 <= 1e-10 (measured with meanref alone, before any device ran: N = 1100 gives 3.6e-10 / 1.5e-10 for pow-exp /
    Matern 5/2, the second and third training vectors of the batched set-up 4.7e-10 / 3.1e-10) the nugget is raised from
    e^-4 to e^-2 (pow-exp) and from 0.01 to 0.03 (Matern), which brings them to 8.4e-11 / 6.4e-11 / 7.3e-11 / 5.8e-11"""
    X, y = synth.design(N, d, 900 + N)
    th = synth.default_thetas(kind, d)
    if big_nugget:
        th[1] = -2.0 if kind == 1 else 0.03
    return X, y + 1.0, th


def setup(ctx, kind, order, X, y, th):
    ctx.set_model(kind, order, X, y)
    _, rc = ctx.predict_setup(th)
    assert rc == abi.OK


def check(what, m, mref):
    assert m.shape == mref.shape and np.all(np.isfinite(m)), what
    err = float(np.max(np.abs(m - mref) / np.maximum(1.0, np.abs(mref))))
    print(f"{what}: max |mean - ref| / max(1,|ref|) = {err:.3e}  (bar {RTOL:.1e})")
    assert err <= RTOL, (what, err)
    return err


def special_queries(X, M, d, seed):
    """M queries in the design's box; some equal to training points, one 5e-11 and one 2e-10 from one"""
    Xq = synth.queries(M, d, seed)
    if M >= 8:
        N = X.shape[0]
        Xq[1] = X[5 % N]
        Xq[2] = X[N - 1]
        Xq[3] = X[7 % N] + 5e-11
        Xq[4] = X[9 % N] + 2e-10
        Xq[M - 1] = X[0]
    return Xq


# ------------------------------------------------------------------ 1. ragged N and M
@pytest.mark.parametrize("N", [63, 64, 65, 127, 129, 513, 1100])
@pytest.mark.parametrize("kind", [1, 3])
def test_ragged_sizes(gpu_ctx, kind, N):
    """N around the 64-point block, one slice (N <= 256) and several (513: 3, 1100: 5, the last one short); M from one query
    to more than three 64-query tiles, each M a call of its own"""
    d, order = 3, 1
    X, y, th = small_model(kind, order, N, d, big_nugget=(N == 1100))
    Xq = special_queries(X, 200, d, 17)
    mref, _, _ = meanref.reference(kind, order, X, y, th, Xq)
    setup(gpu_ctx, kind, order, X, y, th)
    for M in (1, 3, 17, 64, 65, 200):
        check(f"kind {kind} N {N} M {M}", gpu_ctx.predict_mean(Xq[:M]), mref[:M])


# ------------------------------------------------------------------ 2. kinds, orders, dimensions, the Matern log mode
@pytest.mark.parametrize("kind,order,N,d", [(k, o, 300, 8) for k in (1, 2, 3) for o in (0, 1, 2, 3)] +
                         [(1, 3, 310, 16), (1, 2, 330, 31), (1, 1, 200, 1), (2, 1, 200, 1), (3, 1, 200, 1)])
def test_kinds_and_orders(gpu_ctx, kind, order, N, d):
    """every covariance function x regression order at d = 8; pow-exp at d = 16 order 3 (49 basis functions) and d = 31
    order 2 (63, the library's limit); d = 1"""
    X, y, th = small_model(kind, order, N, d)
    Xq = special_queries(X, 70, d, 5)
    mref, _, _ = meanref.reference(kind, order, X, y, th, Xq)
    setup(gpu_ctx, kind, order, X, y, th)
    check(f"kind {kind} order {order} N {N} d {d}", gpu_ctx.predict_mean(Xq), mref)


@pytest.mark.parametrize("kind", [2, 3])
def test_matern_log_mode(kind):
    """GPEMU_MODE_MATERN_LOG: amplitude and nugget on the log scale; the reference runs the literal kernel at their exponentials"""
    N, d, order = 300, 4, 1
    X, y, _ = small_model(kind, order, N, d)
    th_log = np.array([0.3, -3.0, np.log(0.8)])
    th_raw = np.array([np.exp(0.3), np.exp(-3.0), np.log(0.8)])
    Xq = special_queries(X, 70, d, 9)
    mref, _, _ = meanref.reference(kind, order, X, y, th_raw, Xq)
    a, b = abi.Context(0), abi.Context(0)
    try:
        a.set_mode(abi.MODE_MATERN_LOG)
        setup(a, kind, order, X, y, th_log)
        setup(b, kind, order, X, y, th_raw)
        ma, mb = a.predict_mean(Xq), b.predict_mean(Xq)
    finally:
        a.close()
        b.close()
    check(f"kind {kind} log mode", ma, mref)
    check(f"kind {kind} literal mode", mb, mref)
    assert np.array_equal(ma, mb)                       # the same CovParams reach the kernel


# ------------------------------------------------------------------ 3. Gram form, difference form, the switch
@pytest.mark.parametrize("kind", [1, 2, 3])
def test_both_forms(monkeypatch, gpu_ctx, kind):
    """long length scales (Gram form: distances from the matrix unit), length scales so short that
    sum_k (w_k halfrange_k)^2 > 16 (make_cov_params then refuses the Gram form: differences), and the long ones again in a
    context created with GPEMU_KVEC_GRAM=0 (differences by the switch) -- each against the same kind of reference"""
    N, d, order = 330, 3, 1
    X, y, th = small_model(kind, order, N, d)
    Xq = special_queries(X, 130, d, 23)
    half = 0.5 * (X.max(axis=0) - X.min(axis=0))

    def norm2(t):
        w = np.sqrt(0.5) / np.exp(t[2:]) if kind == 1 else np.full(d, 1.0 / np.exp(t[2]))
        return float(np.sum((w * half) ** 2))

    th_short = th.copy()
    th_short[2:] = np.log(0.1)
    assert norm2(th) <= 16.0 < norm2(th_short)
    ref_long, _, _ = meanref.reference(kind, order, X, y, th, Xq)
    ref_short, _, _ = meanref.reference(kind, order, X, y, th_short, Xq)
    setup(gpu_ctx, kind, order, X, y, th)
    m_gram = gpu_ctx.predict_mean(Xq)
    check(f"kind {kind} Gram form", m_gram, ref_long)
    setup(gpu_ctx, kind, order, X, y, th_short)
    check(f"kind {kind} short length scales", gpu_ctx.predict_mean(Xq), ref_short)
    monkeypatch.setenv("GPEMU_KVEC_GRAM", "0")            # copied into the context when it is created
    c = abi.Context(0)
    try:
        setup(c, kind, order, X, y, th)
        m_diff = c.predict_mean(Xq)
    finally:
        c.close()
    check(f"kind {kind} switch off", m_diff, ref_long)
    assert not np.array_equal(m_diff, m_gram), "the switch did not change the form"


# ------------------------------------------------------------------ 4. clamp, nugget rule, far queries
@pytest.mark.parametrize("kind", [1, 2, 3])
@pytest.mark.parametrize("gram", [1, 0])
def test_far_queries_give_the_regression_mean(monkeypatch, kind, gram):
    """the d = 16 inputs of test_gpu_parity.py::test_kvectors_gram_form: queries at training points and 5e-11 / 2e-10 from
    one (the nugget rule applies to pow-exp's 1e-10 threshold, not to the Matern kernels' 1e-16), queries so far away that
    every k is below the clamp -- coordinates of 30 at d = 16 once overflowed the table exp: the mean there is finite and
    equals h^T beta"""
    N, d, M, order = 200, 16, 70, 1
    X, y = synth.design(N, d, 31 + N)
    th = synth.default_thetas(kind, d)
    Xq = synth.queries(M, d, 6)
    Xq[3] = X[5]
    Xq[4] = X[N - 1]
    Xq[5] = X[7] + 5e-11
    Xq[10] = X[11] + 2e-10
    Xq[6] = X[9] + 3.0
    Xq[7] = -20.0
    Xq[8] = 30.0
    Xq[9] = 1.0e4
    Xq[M - 1] = X[0]
    Xq[40:44] = 1.0 + 0.5 * synth.queries(4, d, 8)
    mref, _, _ = meanref.reference(kind, order, X, y, th, Xq)
    far = [8, 9] + ([7] if kind == 1 else [])
    K = np.vstack([O.kvector(kind, X, Xq[q], th) for q in far])
    assert np.all(K == 0.0)                              # every covariance below the clamp: the reference's mean is h^T beta
    monkeypatch.setenv("GPEMU_KVEC_GRAM", str(gram))
    c = abi.Context(0)
    try:
        c.set_model(kind, order, X, y)
        beta, rc = c.predict_setup(th)
        assert rc == abi.OK
        m = c.predict_mean(Xq)
    finally:
        c.close()
    check(f"kind {kind} gram {gram} d=16", m, mref)      # the independent reference, its own beta included
    assert np.all(np.isfinite(m[far]))
    # "equals h^T beta to 1e-14": with the beta the set-up returned and the oracle's h.  Two CPU routes to beta (LAPACK solves,
    # the oracle's estimateBeta) already differ by 1.2e-14 (Matern 3/2) / 1.6e-14 (5/2) in h^T beta at these queries -- beta's
    # conditioning, nothing the sweep computes -- so 1e-14 can only be asked of the sum itself.  Its rounding in any order is
    # at most (nreg + 1) 2^-53 sum|h_a beta_a| / |h^T beta| <= 4.8e-15 here (asserted), so any k . gamma left over shows.
    H = O.hmatrix(order, Xq[far])
    hb = H @ beta
    assert np.max((H.shape[1] + 1) * 2.0 ** -53 * (np.abs(H * beta).sum(axis=1) / np.abs(hb))) <= 5e-15
    err = float(np.max(np.abs(m[far] - hb) / np.abs(hb)))
    print(f"kind {kind} gram {gram}: far queries, |mean - h^T beta| / |h^T beta| = {err:.3e}")
    assert err <= 1e-14


# ------------------------------------------------------------------ 5. against the existing path
@pytest.mark.parametrize("kind,N,d,order", [(1, 513, 3, 1), (3, 1100, 8, 2)])
def test_against_predict_batch(gpu_ctx, kind, N, d, order):
    """a cross-check (the judge is the independent reference): gpemu_predict_batch's mean on the same context and queries"""
    X, y, th = small_model(kind, order, N, d)
    Xq = special_queries(X, 300, d, 41)
    mref, _, _ = meanref.reference(kind, order, X, y, th, Xq)
    setup(gpu_ctx, kind, order, X, y, th)
    m = gpu_ctx.predict_mean(Xq)
    mb, _ = gpu_ctx.predict(Xq)
    check(f"kind {kind} N {N} reference", m, mref)
    check(f"kind {kind} N {N} gpemu_predict_batch", m, mb)


# ------------------------------------------------------------------ 6. committed fixtures (BASELINE sizes)
@pytest.mark.parametrize("name", ["golden_n4096.npz", "golden_n8192_c3.npz"])
def test_oracle_fixtures(gpu_ctx, name):
    """the 64 oracle emulate_point means committed for BASELINE configs[1] (N=4096, pow-exp) and configs[2] (N=8192,
    Matern 5/2, order 1); the design is regenerated from the fixture's seeds (test_gpu_parity.py does the same).
    The fixtures' hyper-parameters are part of the committed numbers and cannot be made better conditioned: A N 2^-52 is
    1.9e-9 (N = 4096) and 2.3e-9 (N = 8192) on them, measured with meanref alone -- above the 1e-10 the other tests hold
    their inputs to, still four times under the bar.  Asserted here: the worst-case rounding bound A N 2^-52 stays below
    RTOL / 4, and the LAPACK route reproduces the oracle's stored means to 1e-10 (measured: 2.8e-12 / 2.2e-12)."""
    f = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name))
    kind, order, N, d, seed, qseed = (int(v) for v in f["meta"][:6])
    th = f["thetas"]
    X, y = synth.design(N, d, seed)
    setup(gpu_ctx, kind, order, X, y, th)
    Xq = synth.queries(64, d, qseed)
    beta, gamma = meanref.trained(kind, order, X, y, th)
    mref, _, A = meanref.predict(kind, order, X, th, beta, gamma, Xq)
    print(f"{name}: A N eps = {A.max() * N * meanref.EPS:.3e}, LAPACK vs fixture {meanref.error(mref, f['mean']):.3e}")
    assert A.max() * N * meanref.EPS <= RTOL / 4
    assert meanref.error(mref, f["mean"]) < 1e-10        # LAPACK route and the oracle's stored numbers agree
    check(name, gpu_ctx.predict_mean(Xq), f["mean"])


# ------------------------------------------------------------------ 7. determinism and independence
def test_same_bits_everywhere(gpu_ctx):
    kind, order, N, d = 3, 1, 1100, 3
    X, y, th = small_model(kind, order, N, d, big_nugget=True)
    Xq = special_queries(X, 200, d, 77)
    mref, _, _ = meanref.reference(kind, order, X, y, th, Xq)
    setup(gpu_ctx, kind, order, X, y, th)
    m1 = gpu_ctx.predict_mean(Xq)
    m2 = gpu_ctx.predict_mean(Xq)
    check("two calls", m1, mref)
    assert np.array_equal(m1, m2)
    # one query alone, as row 0 and as row 137 of a 200-query call (another tile, wave and lane; a far query next to it)
    x = Xq[50]
    alone = gpu_ctx.predict_mean(x[None, :])
    for row in (0, 137):
        Z = Xq.copy()
        Z[row] = x
        Z[(row + 1) % 200] = 40.0
        assert gpu_ctx.predict_mean(Z)[row] == alone[0] == m1[50]
    # device-pointer entry and the two halves
    buf = gpu_ctx.dev_alloc(200 * (d + 1) * 8)
    try:
        gpu_ctx.upload(buf, Xq)
        gpu_ctx.predict_mean_dev(200, buf, buf.value + 200 * d * 8)
        gpu_ctx.sync()
        md = gpu_ctx.download(buf.value + 200 * d * 8, (200,))
    finally:
        gpu_ctx.dev_free(buf)
    assert np.array_equal(md, m1)
    gpu_ctx.predict_mean_enqueue(Xq)
    assert np.array_equal(gpu_ctx.predict_mean_collect(), m1)
    gpu_ctx.prof_begin(abi.PROF_MEAN)
    gpu_ctx.predict_mean(Xq)
    p = gpu_ctx.prof_end()
    assert p["n"] == 2 and p["ms"] > 0 and p["bytes"] == 8.0 * 200 * (d + 1)


def test_difference_form_same_bits(monkeypatch):
    """the independence property in the difference form (context created with the Gram switch off)"""
    kind, order, N, d = 1, 1, 513, 3
    X, y, th = small_model(kind, order, N, d)
    Xq = special_queries(X, 200, d, 78)
    monkeypatch.setenv("GPEMU_KVEC_GRAM", "0")
    c = abi.Context(0)
    try:
        setup(c, kind, order, X, y, th)
        m1 = c.predict_mean(Xq)
        assert np.array_equal(m1, c.predict_mean(Xq))
        alone = c.predict_mean(Xq[50:51])
        Z = Xq.copy()
        Z[137] = Xq[50]
        assert c.predict_mean(Z)[137] == alone[0] == m1[50]
    finally:
        c.close()


def test_setup_by_batch_same_bits():
    """components through gpemu_predict_setup_batch (the non-lead ones own no factorisation workspace and no batch buffers)
    return the bits of a context set up alone"""
    kind, order, N, d = 1, 1, 321, 3
    X, y, th = small_model(kind, order, N, d, big_nugget=True)
    ys = [y, np.cos(3.0 * y) + 0.5, y * y - 0.3 * X[:, 0]]
    ths = [th, th + 0.05, th - 0.03]
    Xq = special_queries(X, 100, d, 3)
    ctxs = [abi.Context(0) for _ in range(3)]
    try:
        for c, yc in zip(ctxs, ys):
            c.set_model(kind, order, X, yc)
        _, _, status, rc = abi.predict_setup_batch(ctxs, np.array(ths))
        assert rc == abi.OK and not status.any()
        for c, yc, tc in zip(ctxs, ys, ths):
            alone = abi.Context(0)
            try:
                setup(alone, kind, order, X, yc, tc)
                ma = alone.predict_mean(Xq)
            finally:
                alone.close()
            mref, _, _ = meanref.reference(kind, order, X, yc, tc, Xq)
            mb = c.predict_mean(Xq)
            check("component of a batched set-up", mb, mref)
            assert np.array_equal(ma, mb)
    finally:
        for c in ctxs:
            c.close()


# ------------------------------------------------------------------ 8. state and errors
def test_state_and_errors():
    kind, order, N, d = 1, 1, 150, 3
    X, y, th = small_model(kind, order, N, d)
    Xq = special_queries(X, 40, d, 2)
    c = abi.Context(0)
    try:
        c.set_model(kind, order, X, y)
        with pytest.raises(abi.GpemuError) as ei:        # before predict_setup
            c.predict_mean(Xq)
        assert ei.value.code == abi.ERR_STATE
        with pytest.raises(abi.GpemuError) as ei:
            c.predict_mean_enqueue(Xq)
        assert ei.value.code == abi.ERR_STATE
        setup(c, kind, order, X, y, th)
        mv0, vv0 = c.predict(Xq)
        m0 = c.predict_mean(Xq)
        out = np.empty(40)
        dp = abi._p
        assert c.L.gpemu_predict_mean(c.h, 40, None, dp(out)) == abi.ERR_ARG
        assert c.L.gpemu_predict_mean(c.h, 40, dp(Xq), None) == abi.ERR_ARG
        assert c.L.gpemu_predict_mean(c.h, 0, dp(Xq), dp(out)) == abi.ERR_ARG
        assert c.L.gpemu_predict_mean_enqueue(c.h, 0, dp(Xq)) == abi.ERR_ARG
        assert c.L.gpemu_predict_mean_enqueue(c.h, 40, None) == abi.ERR_ARG
        assert c.L.gpemu_predict_mean_collect(c.h, 40, None) == abi.ERR_ARG
        assert c.L.gpemu_predict_mean_dev(c.h, 40, None, None) == abi.ERR_ARG
        assert c.L.gpemu_predict_mean_dev(c.h, 0, 8, 8) == abi.ERR_ARG
        assert c.L.gpemu_predict_mean_collect(c.h, 40, dp(out)) == abi.ERR_STATE      # nothing enqueued
        # a mean batch is collected by the mean collect only, and it stays enqueued until then
        c.predict_mean_enqueue(Xq)
        with pytest.raises(abi.GpemuError) as ei:
            c.predict_collect()
        assert ei.value.code == abi.ERR_STATE
        with pytest.raises(abi.GpemuError) as ei:        # one batch of either kind at a time
            c.predict_enqueue(Xq)
        assert ei.value.code == abi.ERR_STATE
        assert np.array_equal(c.predict_mean_collect(), m0)
        # ... and the other way round
        c.predict_enqueue(Xq)
        with pytest.raises(abi.GpemuError) as ei:
            c.predict_mean_collect()
        assert ei.value.code == abi.ERR_STATE
        mv1, vv1 = c.predict_collect()
        assert np.array_equal(mv1, mv0) and np.array_equal(vv1, vv0)
        # after mean-only calls the mean+variance path returns the bits it returned before
        mv2, vv2 = c.predict(Xq)
        assert np.array_equal(mv2, mv0) and np.array_equal(vv2, vv0)
        mref, _, _ = meanref.reference(kind, order, X, y, th, Xq)
        check("state test", m0, mref)
        c.set_training(y + 1.0)                          # the prediction state belongs to the old training vector
        with pytest.raises(abi.GpemuError) as ei:
            c.predict_mean(Xq)
        assert ei.value.code == abi.ERR_STATE
    finally:
        c.close()


# ------------------------------------------------------------------ 9. no batch buffers
def free_hbm(c):
    import ctypes as C
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert c.L.gpemu_device_memory(0, C.byref(free), C.byref(total)) == abi.OK
    return free.value


def test_no_big_buffers():
    """set-up + a 16 384-query mean sweep at N = 4096: free HBM drops by less than ONE of the two batch buffers of
    gpemu_predict_batch (16 384 x Np doubles each) would take"""
    kind, order, N, d = 1, 0, 4096, 8
    X, y = synth.design(N, d, 20261003 + 1)
    th = synth.default_thetas(kind, d)
    th[1] = 2.0                 # the default nugget e^-4 gives A N 2^-52 = 1.9e-9 at this size, e^0 1.8e-10, e^2 4.4e-11
    M = 16384
    Xq = synth.queries(M, d, 12)
    c = abi.Context(0)
    try:
        c.set_model(kind, order, X, y)
        free0 = free_hbm(c)
        _, rc = c.predict_setup(th)
        assert rc == abi.OK
        free1 = free_hbm(c)
        m = c.predict_mean(Xq)
        free2 = free_hbm(c)
        print(f"free HBM: before set-up {free0}, after {free1}, after the sweep {free2}")
        assert free0 - free2 < M * 4096 * 8
        assert free1 - free2 < 64 << 20                  # the sweep itself: staging and 16 slices of partial sums
        sel = np.arange(0, M, 257)
        mref, _, _ = meanref.reference(kind, order, X, y, th, Xq[sel])
        check("16 384 queries, every 257th", m[sel], mref)
    finally:
        c.close()
