"""The joint posterior covariance between the query points of a call (gpemu_predict_cov[_dev], include/gpemu.h, DESIGN.md
4.11) against tests/predcovref.py: C^-1 k, W, Q from LAPACK, c(x*_p, x*_q) and the clamped k-vectors from the oracle --
never the code under test.

Bars: |Sigma_pq - ref_pq| <= 1e-8 max(vscale_p, vscale_q), vscale = kappa (a listed far query: max(kappa, |var|)), and
|mean - ref| <= 1e-8 max(1, |ref|): the variance's and the mean's bars of tests/test_gpu_var_grad.py.  Every comparison first
has predcovref.reference assert that the float64 reference agrees with its extended-precision repeat to 1e-10 in the same
measure (and meanref's A N 2^-52 <= 1e-10 for the mean).  Every call is also checked for cov == cov.T bit for bit and, up to
M = 200, for eigvalsh(cov)[0] >= -M 1e-8 kappa (Weyl's bound for element errors within the bar).  Every test prints its
largest errors (pytest -s).

Inputs: the models, queries and helpers of tests/test_gpu_var_grad.py.  The reference's own error on them, measured on the
CPU before any device ran (covariance against the extended-precision repeat; bar 1e-10; tests/test_predcovref.py): 2.0e-16 ..
2.8e-15 on the near-query families, 2.1e-14 at d = 31 order 2, 8.3e-14 .. 2.3e-13 with the far queries.

The symmetric product takes gemm()'s own tile choice: 128 x 128 tiles from 2 * 1024 tiles of the lower triangle on (one
matrix per launch: twice GPEMU_GEMM_BIG_TILES, choose_gemm_cfg), i.e. from 64 tile rows, M >= 63 * 128 + 1 = 8065, which is
also past the 512 tiles from which the tile table is used.  BIG_M names it.

Measured on an MI355X, largest error per group, covariance / mean (bars 1e-8): ragged N x M 3.7e-15 / 7.5e-14; kinds x orders
and dimensions (d = 31 order 2 and d = 64 included) 2.2e-14 / 4.1e-13; Matern log mode 2.6e-15 / 4.8e-14; Gram form 3.9e-15,
short length scales 2.4e-15, GPEMU_KVEC_GRAM=0 4.2e-15; partly clamped (77 - 82 % zero) 2.6e-15; nugget rule between queries
2.6e-15, the copy's row within 3.4e-18 kappa of its original's; far queries 1.7e-13 / 1.0e-14, their block against
c + h^T Q h 1.1e-14; structure, entries, batched and new set-ups 3.2e-15 / 6.6e-14, diagonal against gpemu_predict_batch's
variance 4.9e-16 kappa; M = 8065 on 128 x 128 tiles 3.8e-15 / 2.1e-14; state test 1.6e-15.  Smallest eigenvalue / scale between
-2.0e-15 and 0.65 (bound -M 1e-8)."""
import ctypes as C

import numpy as np
import pytest

import predcovref
from madaiemulator_amd import abi, synth
from test_gpu_mean_grad import clamp_inputs, k_unclamped, model
from test_gpu_predict_mean import setup, special_queries
from test_gpu_var_grad import (KINDS_ORDERS, RAGGED, entries_inputs, far_inputs, forms_inputs, kinds_inputs, log_mode_inputs,
                               ragged_inputs, stale_inputs)

RTOL = predcovref.RTOL
BIG_M = 8065
pytestmark = pytest.mark.gpu


def check(what, got, ref, sel=slice(None), eig=True):
    """got = (mean or None, cov); ref: predcovref's dict; sel: the leading rows of ref that got holds"""
    m, S = got
    Sref, mref, vs = ref["cov"][sel, sel], ref["mean"][sel], ref["vscale"][sel]
    M = Sref.shape[0]
    assert S.shape == (M, M) and np.all(np.isfinite(S)), what
    assert np.array_equal(S, S.T), (what, "not symmetric bit for bit")
    err = predcovref.error(S, Sref, vs)
    emean = 0.0
    if m is not None:
        assert np.all(np.isfinite(m))
        emean = float(np.max(np.abs(m - mref) / np.maximum(1.0, np.abs(mref))))
    lam = float("nan")
    if eig and M <= 200:
        lam = float(np.linalg.eigvalsh(S)[0]) / float(vs.max())
        assert lam >= -M * RTOL, (what, "smallest eigenvalue / scale", lam)
    print(f"{what}: cov {err:.3e} of max(vscale_p, vscale_q), mean {emean:.3e}  (bars {RTOL:.1e}); smallest eigenvalue / scale {lam:.2e}")
    assert err <= RTOL and emean <= RTOL, (what, err, emean)
    return err


# ------------------------------------------------------------------ 1. ragged N and M
@pytest.mark.parametrize("kind,N", RAGGED)
def test_ragged_sizes(gpu_ctx, kind, N):
    """N around the 64-point block; M = 1, 2, less than, exactly, one more than a 64 x 64 tile of Sigma and 200 (ten lower
    tiles, the last tile row and column 8 wide), each M a call of its own against the leading block of ONE reference;
    queries on, 5e-11 from and 2e-10 from a training point among them."""
    kind, order, X, y, th, Xq = ragged_inputs(kind, N)
    ref = predcovref.reference(kind, order, X, y, th, Xq)
    setup(gpu_ctx, kind, order, X, y, th)
    for M in (1, 2, 17, 64, 65, 200):
        check(f"kind {kind} N {N} M {M}", gpu_ctx.predict_cov(Xq[:M]), ref, slice(0, M))


# ------------------------------------------------------------------ 2. kinds, orders, dimensions
@pytest.mark.parametrize("kind,order,N,d", KINDS_ORDERS)
def test_kinds_and_orders(gpu_ctx, kind, order, N, d):
    """every covariance function x regression order at d = 8 (M = 70: two tile rows); d = 1 and 15, 16, 17; pow-exp at d = 31
    order 2 (63 basis functions: every column of r and Q r in use, the regression staging at its LDS maximum) and at d = 64"""
    kind, order, X, y, th, Xq = kinds_inputs(kind, order, N, d)
    ref = predcovref.reference(kind, order, X, y, th, Xq)
    setup(gpu_ctx, kind, order, X, y, th)
    check(f"kind {kind} order {order} N {N} d {d}", gpu_ctx.predict_cov(Xq), ref)


# ------------------------------------------------------------------ 3. Matern log mode
@pytest.mark.parametrize("kind", [2, 3])
def test_matern_log_mode(kind):
    """GPEMU_MODE_MATERN_LOG: amplitude and nugget on the log scale, in the k-vectors AND in the prior between queries; the
    reference runs the literal kernel at their exponentials; the two modes return the same bits"""
    kind, order, X, y, th_raw, Xq = log_mode_inputs(kind)
    th_log = np.array([0.3, -3.0, np.log(0.8)])
    ref = predcovref.reference(kind, order, X, y, th_raw, Xq)
    a, b = abi.Context(0), abi.Context(0)
    try:
        a.set_mode(abi.MODE_MATERN_LOG)
        setup(a, kind, order, X, y, th_log)
        setup(b, kind, order, X, y, th_raw)
        ga, gb = a.predict_cov(Xq), b.predict_cov(Xq)
    finally:
        a.close()
        b.close()
    check(f"kind {kind} log mode", ga, ref)
    check(f"kind {kind} literal mode", gb, ref)
    for u, w in zip(ga, gb):
        assert np.array_equal(u, w)


# ------------------------------------------------------------------ 4. both k-vector forms
@pytest.mark.parametrize("kind", [1, 2, 3])
def test_both_forms(monkeypatch, gpu_ctx, kind):
    """the k-vectors in Gram form, in difference form (length scales the Gram form refuses) and with GPEMU_KVEC_GRAM=0; the
    prior between queries is the difference form throughout"""
    kind, order, X, y, th, th_short, Xq = forms_inputs(kind)
    ref_long = predcovref.reference(kind, order, X, y, th, Xq)
    ref_short = predcovref.reference(kind, order, X, y, th_short, Xq)
    setup(gpu_ctx, kind, order, X, y, th)
    g_gram = gpu_ctx.predict_cov(Xq)
    check(f"kind {kind} Gram form", g_gram, ref_long)
    setup(gpu_ctx, kind, order, X, y, th_short)
    check(f"kind {kind} short length scales", gpu_ctx.predict_cov(Xq), ref_short)
    monkeypatch.setenv("GPEMU_KVEC_GRAM", "0")            # copied into the context when it is created
    c = abi.Context(0)
    try:
        setup(c, kind, order, X, y, th)
        g_diff = c.predict_cov(Xq)
    finally:
        c.close()
    check(f"kind {kind} switch off", g_diff, ref_long)
    assert not np.array_equal(g_diff[1], g_gram[1]), "the switch did not change the form"


# ------------------------------------------------------------------ 5. the clamp, 6. the nugget rule between queries
PAIRS = [(11, 4), (23, 7), (41, 30)]          # a copy; 5e-11 apart; both on one training point


def nugget_inputs(kind):
    """clamp_inputs with three pairs of queries set: 11 a copy of 4; 23 at 5e-11 from 7 (inside the pow-exp box of 1e-10,
    outside Matern's of 1e-16); 30 and 41 both on training point 12.  Still no k value within 1 +- 1e-6 of the clamp."""
    X, y, th, Xq, order = clamp_inputs(kind)
    Xq = Xq.copy()
    Xq[11] = Xq[4]
    Xq[23] = Xq[7] + 5e-11
    Xq[30] = X[12]
    Xq[41] = X[12]
    k = np.vstack([k_unclamped(kind, th, X, x) for x in Xq])
    assert np.all(np.abs(k / 1e-10 - 1.0) > 1e-6)
    return X, y, th, Xq, order


@pytest.mark.parametrize("kind", [1, 2, 3])
def test_clamped_part(gpu_ctx, kind):
    """77 - 82 % of the k values under the clamp while the prior between queries is NOT clamped"""
    X, y, th, Xq, order = clamp_inputs(kind)
    ref = predcovref.reference(kind, order, X, y, th, Xq)
    zero = float(np.mean(ref["K"] == 0.0))
    print(f"kind {kind}: {100 * zero:.1f} % of the k values are clamped")
    assert 0.1 <= zero <= 0.9
    setup(gpu_ctx, kind, order, X, y, th)
    check(f"kind {kind} partly clamped", gpu_ctx.predict_cov(Xq), ref)


@pytest.mark.parametrize("kind", [1, 2, 3])
def test_nugget_rule_between_queries(gpu_ctx, kind):
    """a copied query gives the rows and columns of its original and carries the nugget off the diagonal; 5e-11 apart carries it for
    pow-exp only; two queries on one training point.  A missing nugget or a clamped prior is an error of the order of the
    printed reference values, far above the bar."""
    X, y, th, Xq, order = nugget_inputs(kind)
    ref = predcovref.reference(kind, order, X, y, th, Xq)
    kap = ref["kappa"]
    print(f"kind {kind}: reference off-diagonal elements / kappa at the pairs:", [float(ref["cov"][p, q] / kap) for p, q in PAIRS])
    setup(gpu_ctx, kind, order, X, y, th)
    m, S = gpu_ctx.predict_cov(Xq)
    check(f"kind {kind} nugget rule", (m, S), ref)
    # the copy: the same bits wherever both elements are made by the same expression -- columns up to 4 (both in the lower
    # triangle) and from 11 on (both mirrored from one row of it).  Between them one is r_11 . (Q r_j) and the other the
    # mirror of r_j . (Q r_4): equal to rounding, and both within the bar of one reference value (check above)
    same = np.r_[0:5, 11:S.shape[0]]
    assert np.array_equal(S[11, same], S[4, same]) and np.array_equal(S[same, 11], S[same, 4])
    print(f"kind {kind}: rows of the copy and its original differ by at most {np.max(np.abs(S[11] - S[4])) / kap:.2e} kappa between the two")
    for p, q in PAIRS:
        assert abs(S[p, q] - ref["cov"][p, q]) <= RTOL * kap


# ------------------------------------------------------------------ 7. far queries
FAR = [8, 9, 10]


def far_cov_inputs(kind):
    """far_inputs of the variance-gradient tests at order 1 with three far queries: every coordinate 30, 35 and 40"""
    kind, _, X, y, th, Xq = far_inputs(kind)
    Xq = Xq.copy()
    Xq[8], Xq[9], Xq[10] = 30.0, 35.0, 40.0
    return kind, 1, X, y, th, Xq


@pytest.mark.parametrize("kind", [1, 2, 3])
@pytest.mark.parametrize("gram", [1, 0])
def test_far_queries(monkeypatch, kind, gram):
    """d = 16, N = 200, order 1: coordinates of 30 and more put every k under the clamp, r = h there, and the far block is
    c + h_p^T Q h_q, worked out here from LAPACK's Q without any k; the far rows against near queries with the reference"""
    import scipy.linalg as sl
    from oracle import oracle as O
    kind, order, X, y, th, Xq = far_cov_inputs(kind)
    ref = predcovref.reference(kind, order, X, y, th, Xq, far=FAR)
    assert np.all(ref["K"][FAR] == 0.0)
    H = O.hmatrix(order, X)
    Q = np.linalg.inv(H.T @ sl.cho_solve(sl.cho_factor(O.cov_matrix(kind, X, th), lower=True), H))
    hq = O.hmatrix(order, Xq[FAR])
    want = O.cov_matrix(kind, Xq[FAR], th) + hq @ Q @ hq.T
    vs = ref["vscale"][FAR]
    assert predcovref.error(ref["cov"][np.ix_(FAR, FAR)], want, vs) <= 1e-12
    print(f"kind {kind}: far variances / kappa {ref['var'][FAR] / ref['kappa']}")
    monkeypatch.setenv("GPEMU_KVEC_GRAM", str(gram))
    c = abi.Context(0)
    try:
        setup(c, kind, order, X, y, th)
        got = c.predict_cov(Xq)
    finally:
        c.close()
    check(f"kind {kind} gram {gram} d=16", got, ref)
    err = predcovref.error(got[1][np.ix_(FAR, FAR)], want, vs)
    print(f"kind {kind} gram {gram}: far block against c + h^T Q h: {err:.3e}")
    assert err <= RTOL


# ------------------------------------------------------------------ 8. structure
def test_structure(gpu_ctx):
    """symmetric bit for bit, positive semi-definite to Weyl's bound (both inside check), and the diagonal and the mean are
    gpemu_predict_batch's within the bars"""
    kind, order, X, y, th, Xq = entries_inputs()
    ref = predcovref.reference(kind, order, X, y, th, Xq)
    setup(gpu_ctx, kind, order, X, y, th)
    pm, pv = gpu_ctx.predict(Xq)
    m, S = gpu_ctx.predict_cov(Xq)
    check("structure", (m, S), ref)
    ed = float(np.max(np.abs(np.diag(S) - pv) / ref["vscale"]))
    em = float(np.max(np.abs(m - pm) / np.maximum(1.0, np.abs(pm))))
    print(f"diagonal against gpemu_predict_batch's variance {ed:.3e} of kappa, mean {em:.3e}")
    assert ed <= RTOL and em <= RTOL


# ------------------------------------------------------------------ 9. same bits everywhere
def test_same_bits_everywhere(gpu_ctx):
    """two calls, the device-pointer entry with and without a mean, a NULL mean on the host entry; and the batch buffers it
    shares: predict_batch, predict_mean_grad and predict_var_grad return the bits they returned before"""
    kind, order, X, y, th, Xq = entries_inputs()
    d, M = X.shape[1], Xq.shape[0]
    ref = predcovref.reference(kind, order, X, y, th, Xq)
    setup(gpu_ctx, kind, order, X, y, th)
    before = gpu_ctx.predict(Xq) + gpu_ctx.predict_mean_grad(Xq) + gpu_ctx.predict_var_grad(Xq)
    m1, S1 = gpu_ctx.predict_cov(Xq)
    m2, S2 = gpu_ctx.predict_cov(Xq)
    check("two calls", (m1, S1), ref)
    assert np.array_equal(m1, m2) and np.array_equal(S1, S2)
    after = gpu_ctx.predict(Xq) + gpu_ctx.predict_mean_grad(Xq) + gpu_ctx.predict_var_grad(Xq)
    for u, w in zip(before, after):
        assert np.array_equal(u, w)
    buf = gpu_ctx.dev_alloc((M * (d + 1) + M * M) * 8)
    try:
        gpu_ctx.upload(buf, Xq)
        mean_dev, cov_dev = buf.value + M * d * 8, buf.value + M * (d + 1) * 8
        gpu_ctx.predict_cov_dev(M, buf, mean_dev, cov_dev)
        gpu_ctx.sync()
        assert np.array_equal(gpu_ctx.download(mean_dev, (M,)), m1) and np.array_equal(gpu_ctx.download(cov_dev, (M, M)), S1)
        gpu_ctx.upload(cov_dev, np.zeros((M, M)))
        gpu_ctx.predict_cov_dev(M, buf, None, cov_dev)
        gpu_ctx.sync()
        assert np.array_equal(gpu_ctx.download(cov_dev, (M, M)), S1)
        assert np.array_equal(gpu_ctx.download(mean_dev, (M,)), m1)         # untouched
    finally:
        gpu_ctx.dev_free(buf)
    none_m, Sn = gpu_ctx.predict_cov(Xq, want_mean=False)
    assert none_m is None and np.array_equal(Sn, S1)
    # a shorter call after a longer one: the leading block, same bits (an element depends on its own two queries only)
    _, S70 = gpu_ctx.predict_cov(Xq[:70])
    assert np.array_equal(S70, S1[:70, :70])
    gpu_ctx.prof_begin(abi.PROF_COV)
    gpu_ctx.predict_cov(Xq)
    p = gpu_ctx.prof_end()
    assert p["n"] == 2 and p["ms"] > 0 and p["bytes"] == 8.0 * M * M


def test_setup_by_batch_same_bits():
    """two contexts through gpemu_predict_setup_batch: each returns its own state's Sigma, in the bits of a context set up
    alone"""
    kind, order, X, y, th1, th2, y2, Xq = stale_inputs()
    ys, ths = [y, y2], [th1, th2]
    ctxs = [abi.Context(0) for _ in range(2)]
    try:
        for c, yc in zip(ctxs, ys):
            c.set_model(kind, order, X, yc)
        _, _, status, rc = abi.predict_setup_batch(ctxs, np.array(ths))
        assert rc == abi.OK and not status.any()
        for c, yc, tc in zip(ctxs, ys, ths):
            got = c.predict_cov(Xq)
            check("component of a batched set-up", got, predcovref.reference(kind, order, X, yc, tc, Xq))
            alone = abi.Context(0)
            try:
                setup(alone, kind, order, X, yc, tc)
                want = alone.predict_cov(Xq)
            finally:
                alone.close()
            for u, w in zip(got, want):
                assert np.array_equal(u, w)
    finally:
        for c in ctxs:
            c.close()


# ------------------------------------------------------------------ 10. new set-ups
def test_new_setups():
    """set up at theta_1, call, set up at theta_2, call: the second answer is theta_2's; the same with a new training
    vector (Sigma does not depend on it, the mean does)"""
    kind, order, X, y, th1, th2, y2, Xq = stale_inputs()
    ref1 = predcovref.reference(kind, order, X, y, th1, Xq)
    ref2 = predcovref.reference(kind, order, X, y, th2, Xq)
    ref3 = predcovref.reference(kind, order, X, y2, th2, Xq)
    assert predcovref.error(ref1["cov"], ref2["cov"], ref2["vscale"]) > 1e-3     # the two states are told apart
    assert np.max(np.abs(ref3["mean"] - ref2["mean"])) > 1e-3
    c = abi.Context(0)
    try:
        setup(c, kind, order, X, y, th1)
        check("theta_1", c.predict_cov(Xq), ref1)
        _, rc = c.predict_setup(th2)
        assert rc == abi.OK
        check("theta_2 after theta_1", c.predict_cov(Xq), ref2)
        c.set_training(y2)
        with pytest.raises(abi.GpemuError) as ei:        # the prediction state belonged to the old training vector
            c.predict_cov(Xq)
        assert ei.value.code == abi.ERR_STATE
        _, rc = c.predict_setup(th2)
        assert rc == abi.OK
        check("new training vector", c.predict_cov(Xq), ref3)
    finally:
        c.close()


# ------------------------------------------------------------------ 11. the large-tile path
def big_inputs():
    kind, order, N, d = 3, 1, 64, 3
    X, y, th = model(kind, order, N, d)
    Xq = synth.queries(BIG_M, d, 12)
    Xq[5], Xq[BIG_M - 1], Xq[8000] = X[3], X[0], Xq[77]
    rows = np.unique(np.concatenate([np.arange(0, BIG_M, 97), [5, 77, 8000, BIG_M - 2, BIG_M - 1]]))
    return kind, order, X, y, th, Xq, rows


def test_large_tiles():
    """M = 8065 = 63 * 128 + 1: 2080 lower 128 x 128 tiles, the first M at which gemm()'s own rule gives the symmetric product
    the 128 x 128 kernel and the tile table; the last tile row and column are one element wide.  N = 64 keeps the flops and
    the reference small.  Every element against the float64 reference, whose precondition is checked on every 97th query,
    the special ones and the edge.  A small call beside it stays on 64 x 64 tiles."""
    kind, order, X, y, th, Xq, rows = big_inputs()
    ref = predcovref.reference(kind, order, X, y, th, Xq, rows=rows)
    c = abi.Context(0)
    try:
        setup(c, kind, order, X, y, th)
        c.prof_begin(abi.PROF_GEMM_BIG)
        c.predict_cov(Xq[:200], want_mean=False)
        assert c.prof_end()["n"] == 0
        c.prof_begin(abi.PROF_GEMM_BIG)
        m, S = c.predict_cov(Xq)
        assert c.prof_end()["n"] == 1                    # the symmetric product; the sweep's n = Np + 64 < 256 stays small
    finally:
        c.close()
    check(f"M {BIG_M} on 128 x 128 tiles", (m, S), ref, eig=False)
    assert np.array_equal(S[8000], S[77])


# ------------------------------------------------------------------ 12. state and errors
def free_bytes():
    fr, tot = C.c_size_t(0), C.c_size_t(0)
    assert abi.load().gpemu_device_memory(0, C.byref(fr), C.byref(tot)) == abi.OK
    return fr.value


def test_state_and_errors():
    kind, order, N, d = 1, 1, 150, 3
    X, y, th = model(kind, order, N, d)
    Xq = special_queries(X, 40, d, 2)
    c = abi.Context(0)
    try:
        c.set_model(kind, order, X, y)
        with pytest.raises(abi.GpemuError) as ei:        # before predict_setup
            c.predict_cov(Xq)
        assert ei.value.code == abi.ERR_STATE
        assert c.L.gpemu_predict_cov_dev(c.h, 40, 8, None, 8) == abi.ERR_STATE
        setup(c, kind, order, X, y, th)
        ref = predcovref.reference(kind, order, X, y, th, Xq)
        m0, S0 = c.predict_cov(Xq)
        check("state test", (m0, S0), ref)
        out, cov = np.empty(40), np.empty((40, 40))
        dp, L = abi._p, c.L
        assert L.gpemu_predict_cov(c.h, 40, None, dp(out), dp(cov)) == abi.ERR_ARG
        assert L.gpemu_predict_cov(c.h, 40, dp(Xq), dp(out), None) == abi.ERR_ARG
        assert L.gpemu_predict_cov(c.h, 0, dp(Xq), dp(out), dp(cov)) == abi.ERR_ARG
        assert L.gpemu_predict_cov(c.h, -3, dp(Xq), dp(out), dp(cov)) == abi.ERR_ARG
        assert L.gpemu_predict_cov_dev(c.h, 40, None, None, 8) == abi.ERR_ARG
        assert L.gpemu_predict_cov_dev(c.h, 40, 8, None, None) == abi.ERR_ARG
        assert L.gpemu_predict_cov_dev(c.h, 0, 8, 8, 8) == abi.ERR_ARG
        # one more than the block: refused before anything is allocated (the pointers are never touched)
        c.sync()
        fr0 = free_bytes()
        assert L.gpemu_predict_cov(c.h, 16385, dp(Xq), dp(out), dp(cov)) == abi.ERR_ARG
        assert L.gpemu_predict_cov_dev(c.h, 16385, 8, 8, 8) == abi.ERR_ARG
        assert free_bytes() == fr0
        assert L.gpemu_predict_cov(c.h, 40, dp(Xq), None, dp(cov)) == abi.OK                # NULL mean; usable after the refusals
        assert np.array_equal(cov, S0)
        # the host entry stages through the buffers of a pending batch: refused while one is pending, of any kind, and the
        # batch stays collectable
        for enq, col in ((c.predict_enqueue, c.predict_collect), (c.predict_mean_enqueue, c.predict_mean_collect),
                         (c.predict_mean_grad_enqueue, c.predict_mean_grad_collect), (c.predict_var_grad_enqueue, c.predict_var_grad_collect)):
            enq(Xq)
            want = col()
            enq(Xq)
            with pytest.raises(abi.GpemuError) as ei:
                c.predict_cov(Xq)
            assert ei.value.code == abi.ERR_STATE
            got = col()
            for u, w in zip(got if isinstance(got, tuple) else (got,), want if isinstance(want, tuple) else (want,)):
                assert np.array_equal(u, w)
        m1, S1 = c.predict_cov(Xq)
        assert np.array_equal(m1, m0) and np.array_equal(S1, S0)
        c.set_training(y + 1.0)                          # the prediction state belongs to the old training vector
        with pytest.raises(abi.GpemuError) as ei:
            c.predict_cov(Xq)
        assert ei.value.code == abi.ERR_STATE
    finally:
        c.close()
