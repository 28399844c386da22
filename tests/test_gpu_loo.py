"""Leave-one-out prediction at every training point from the resident prediction state (gpemu_loo, include/gpemu.h).

The device evaluates the closed form  P = C^-1 - W Q W^T,  var_i = 1 / P_ii,  mean_i = y_i - gamma_i / P_ii  with
P_ii = sum_{k >= i} (L^-1)_ki^2 - w_i^T Q w_i.  It is compared with what the formula stands for -- the oracle's own
alloc_emulator_struct on the other N - 1 points and emulate_point at the removed one, for EVERY point at small N -- and,
where N refits are out of reach, with the same closed form through LAPACK's explicit inverse plus refits at fixed indices
(tests/looref.py).  Bars: those of test_gpu_parity.py::test_ragged_sizes_full_path, RTOL = 1e-8: mean error below
RTOL * max(1, max |mean|), variance error below RTOL * kappa.

The oracle's k-vector zeroes covariances below 1e-10 (emulator.c:588-590); the closed form reads the matrix C, which is
not clamped.  Every comparison with oracle refits therefore asserts first that no off-diagonal element of C is below
1e-10, so that the clamp cannot enter."""
import numpy as np
import pytest

import looref
from madaiemulator_amd import abi, synth
from oracle import oracle as O

RTOL = 1e-8              # the north_star parity bar (test_gpu_parity.py)
SEED_C2 = 20261003 + 1   # the design of BASELINE configs[1] (tests/golden/make_golden_n4096.py)
SEED_C3 = 20261003 + 2   # the design of BASELINE configs[2] (tests/golden/make_golden_n8192_c3.py)

pytestmark = pytest.mark.gpu


def small_model(kind, order, N, d):
    """the inputs of test_ragged_sizes_full_path"""
    X, y = synth.design(N, d, 900 + N)
    return X, y + 1.0, synth.default_thetas(kind, d)


def setup(ctx, kind, order, X, y, th):
    ctx.set_model(kind, order, X, y)
    _, rc = ctx.predict_setup(th)
    assert rc == abi.OK


def check(what, m, v, mref, vref, kappa, bar=RTOL):
    em, ev = looref.errors(m, v, mref, vref, kappa)
    print(f"{what}: mean err / max(1,|m|) {em:.3e}  var err / kappa {ev:.3e}  (bar {bar:.1e})")
    assert np.all(np.isfinite(m)) and np.all(np.isfinite(v)) and np.all(v > 0), what
    assert em < bar and ev < bar, (what, em, ev, bar)


# ------------------------------------------------------------------ 1. every point against brute-force refits
@pytest.mark.parametrize("kind,order,N,d", [(1, 1, 150, 3), (3, 1, 150, 3), (2, 0, 120, 2), (1, 2, 130, 4), (1, 3, 100, 2)])
def test_every_point_against_oracle_refits(gpu_ctx, kind, order, N, d):
    X, y, th = small_model(kind, order, N, d)
    assert looref.min_offdiag(O.cov_matrix(kind, X, th)) >= looref.CLAMP
    setup(gpu_ctx, kind, order, X, y, th)
    m, v = gpu_ctx.loo()
    mo, vo = looref.oracle_refits(kind, order, X, y, th, range(N))
    check(f"kind {kind} order {order} N {N} d {d}", m, v, mo, vo, O.cov(kind, X[0], X[0], th))


# ------------------------------------------------------------------ 2. a duplicated design row
def test_duplicated_design_row(gpu_ctx):
    """Row N-1 = row 5, as the fill tests do: the nugget rule (emulator.c:136-150) puts the nugget on the off-diagonal
    element (N-1, 5) too, so rows 5 and N-1 of C are the same numbers and C is exactly singular.  There is then no trained
    emulator to validate: the oracle's set-up fails on the full design (Cholesky pivot <= 0) and on every refit that keeps
    both twins, i.e. every i but 5 and N-1; the closed form needs C^-1, which does not exist.  A comparison of numbers
    "as in case 1" has no reference here.  What holds and is checked: the oracle refuses the design; the device either
    refuses it too (GPEMU_ERR_NOT_PD: whether the last pivot rounds to <= 0 depends on the order of the factorisation's
    sums) and then gives GPEMU_ERR_STATE instead of leave-one-out numbers, or -- a pivot that rounded above zero -- answers
    without an error; and dropping one twin gives a design on which every point meets the bars of case 1."""
    kind, order, N, d = 1, 1, 150, 3
    X, y, th = small_model(kind, order, N, d)
    X = X.copy()
    X[N - 1] = X[5]
    Cm = O.cov_matrix(kind, X, th)
    assert Cm[N - 1, 5] == Cm[5, 5] and np.array_equal(Cm[5], Cm[N - 1])       # the nugget sits off the diagonal
    assert O.Emulator(kind, order, X, y, th).status != 0                        # ... and the reference has no emulator
    gpu_ctx.set_model(kind, order, X, y)
    _, rc = gpu_ctx.predict_setup(th)
    print("duplicated row: predict_setup returned", rc)
    assert rc in (abi.OK, abi.ERR_NOT_PD)
    if rc == abi.ERR_NOT_PD:
        with pytest.raises(abi.GpemuError) as ei:
            gpu_ctx.loo()
        assert ei.value.code == abi.ERR_STATE
    else:
        m, v = gpu_ctx.loo()
        assert m.shape == (N,) and v.shape == (N,)
    # one twin dropped (the last row): an ordinary design again, every point against its refit
    Xk, yk = X[:N - 1], y[:N - 1]
    assert looref.min_offdiag(O.cov_matrix(kind, Xk, th)) >= looref.CLAMP
    setup(gpu_ctx, kind, order, Xk, yk, th)
    m, v = gpu_ctx.loo()
    mo, vo = looref.oracle_refits(kind, order, Xk, yk, th, range(N - 1))
    check("one twin dropped", m, v, mo, vo, O.cov(kind, X[0], X[0], th))


# ------------------------------------------------------------------ 3. ragged N
@pytest.mark.parametrize("N", [63, 64, 65, 127, 129, 513])
@pytest.mark.parametrize("kind", [1, 3])
def test_ragged_sizes(gpu_ctx, kind, N):
    """N around the 64-column padding granule, the 64-row chunks and the 512-column strips of the column-sum kernel"""
    d, order = 3, 1
    X, y, th = small_model(kind, order, N, d)
    Cm = O.cov_matrix(kind, X, th)
    setup(gpu_ctx, kind, order, X, y, th)
    m, v = gpu_ctx.loo()
    mc, vc = looref.closed_form(Cm, O.hmatrix(order, X), y)
    kappa = O.cov(kind, X[0], X[0], th)
    check(f"kind {kind} N {N} closed form", m, v, mc, vc, kappa)
    if N == 513:
        idx = [0, 63, 64, 255, 256, 449, 511, N - 1]
        assert looref.min_offdiag(Cm) >= looref.CLAMP
        mo, vo = looref.oracle_refits(kind, order, X, y, th, idx)
        check(f"kind {kind} N {N} oracle refits", m[idx], v[idx], mo, vo, kappa)


# ------------------------------------------------------------------ 4. BASELINE sizes
@pytest.mark.parametrize("kind,order,N,d,seed", [(1, 0, 4096, 8, SEED_C2), (3, 1, 8192, 8, SEED_C3)])
def test_baseline_sizes(gpu_ctx, kind, order, N, d, seed):
    """BASELINE configs[1] and configs[2]: every point against the closed form through LAPACK's explicit inverse, four
    points against LAPACK refits (Cholesky factor of the other N - 1 points).  The bar is RTOL unless the two CPU routes
    themselves disagree by more than 1e-10 at the four points; then it is 100 x their disagreement.  Measured on the CPU
    before any device ran (leave-one-out section): the routes agree to 3.3e-14 (mean) / 1.1e-15 (variance) at
    N = 4096 and 2.4e-14 / 9.2e-16 at N = 8192, so the bar is RTOL at both sizes."""
    X, y = synth.design(N, d, seed)
    th = synth.default_thetas(kind, d)
    Cm = O.cov_matrix(kind, X, th)
    H = O.hmatrix(order, X)
    kappa = float(Cm[0, 0])
    setup(gpu_ctx, kind, order, X, y, th)
    m, v = gpu_ctx.loo()
    idx = [0, N // 3, (2 * N) // 3 + 1, N - 1]
    ml, vl = looref.lapack_refits(Cm, H, y, idx)
    mc, vc = looref.closed_form(Cm, H, y)
    dis = max(looref.errors(mc[idx], vc[idx], ml, vl, kappa))
    bar = RTOL if dis <= 1e-10 else 100.0 * dis
    print(f"N {N}: CPU routes disagree by {dis:.3e} -> bar {bar:.1e}")
    check(f"N {N} closed form", m, v, mc, vc, kappa, bar)
    check(f"N {N} LAPACK refits", m[idx], v[idx], ml, vl, kappa, bar)


# ------------------------------------------------------------------ 5. set-up by batch
def test_setup_by_batch_same_bits():
    """three components through gpemu_predict_setup_batch (the non-lead ones own their L^-1 rows but no factorisation
    workspace): loo() of each equals, bit for bit, loo() of a fresh context set up alone"""
    kind, order, N, d = 1, 1, 321, 3
    X, y, th = small_model(kind, order, N, d)
    ys = [y, np.cos(3.0 * y) + 0.5, y * y - 0.3 * X[:, 0]]
    ths = [th, th + 0.05, th - 0.03]
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
                ma, va = alone.loo()
            finally:
                alone.close()
            mb, vb = c.loo()
            assert np.array_equal(ma, mb) and np.array_equal(va, vb)
            assert np.all(np.isfinite(mb)) and np.all(vb > 0)
    finally:
        for c in ctxs:
            c.close()


# ------------------------------------------------------------------ 6. same bits twice, device-pointer entry
def test_same_bits_twice_and_device_entry(gpu_ctx):
    kind, order, N, d = 3, 1, 1100, 3
    X, y, th = small_model(kind, order, N, d)
    setup(gpu_ctx, kind, order, X, y, th)
    m1, v1 = gpu_ctx.loo()
    m2, v2 = gpu_ctx.loo()
    assert np.array_equal(m1, m2) and np.array_equal(v1, v2)
    buf = gpu_ctx.dev_alloc(2 * N * 8)
    try:
        gpu_ctx.loo_dev(buf, buf.value + N * 8)
        both = gpu_ctx.download(buf, (2, N))
    finally:
        gpu_ctx.dev_free(buf)
    assert np.array_equal(both[0], m1) and np.array_equal(both[1], v1)
    gpu_ctx.prof_begin(abi.PROF_LOO)
    gpu_ctx.loo()
    p = gpu_ctx.prof_end()
    assert p["n"] == 2 and p["ms"] > 0 and p["bytes"] >= 8.0 * N * (N + 1) / 2


# ------------------------------------------------------------------ 7. errors
def test_errors(gpu_ctx):
    kind, order, N, d = 1, 1, 90, 3
    X, y, th = small_model(kind, order, N, d)
    gpu_ctx.set_model(kind, order, X, y)
    with pytest.raises(abi.GpemuError) as ei:            # before predict_setup
        gpu_ctx.loo()
    assert ei.value.code == abi.ERR_STATE
    setup(gpu_ctx, kind, order, X, y, th)
    gpu_ctx.loo()
    gpu_ctx.set_training(y + 1.0)
    with pytest.raises(abi.GpemuError) as ei:            # the prediction state belongs to the old training vector
        gpu_ctx.loo()
    assert ei.value.code == abi.ERR_STATE
    assert gpu_ctx.L.gpemu_loo(gpu_ctx.h, None, None) == abi.ERR_ARG
    # N = nreg + 1: no degrees of freedom are left with one point removed
    n1 = 1 + order * d + 1
    setup(gpu_ctx, kind, order, X[:n1], y[:n1], th)
    with pytest.raises(abi.GpemuError) as ei:
        gpu_ctx.loo()
    assert ei.value.code == abi.ERR_ARG
    # ... and the context still predicts
    Xq = synth.queries(7, d, 4)
    mq, vq = gpu_ctx.predict(Xq)
    mo, vo, _ = O.Emulator(kind, order, X[:n1], y[:n1], th).emulate(Xq)
    assert np.max(np.abs(mq - mo)) < RTOL * max(1.0, np.abs(mo).max())
    assert np.max(np.abs(vq - vo)) < RTOL * O.cov(kind, X[0], X[0], th)
