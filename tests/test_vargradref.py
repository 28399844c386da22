"""tests/vargradref.py (the reference the device tests of the variance gradient are judged by) against things that do not
share its formulas: central differences of the LAPACK variance, mpmath differentiation of the whole variance for the
Matern kinds, the closed form at far queries; and its extended-precision route against mpmath.  CPU only.

Central differences, h = 1e-5, bar 1e-7 max(kappa, |grad|_inf): the differences' truncation h^2 |var'''| / 6 and their
rounding 2^-52 cond kappa / h together measure 5.3e-11 .. 8.6e-9 on these inputs (largest: order 3 at d = 31, where the
cubic basis makes |grad| and the third derivative largest; Matern 3/2 at d = 1 .. 3: 2.4e-9 .. 5.1e-9); a wrong constant
(3 for 1.732050808^2, a dropped factor 2) shows at 1e-3 and above.  The mpmath differentiation agrees to 1.3e-15, the
longdouble route with mpmath to 3.5e-18."""
import math

import numpy as np
import pytest

import vargradref
from madaiemulator_amd import synth
from oracle import oracle as O


def model(kind, N, d):
    """the inputs of test_gpu_predict_mean.py::small_model"""
    X, y = synth.design(N, d, 900 + N)
    return X, y + 1.0, synth.default_thetas(kind, d)


@pytest.mark.parametrize("d", [1, 3, 8, 16, 31])
@pytest.mark.parametrize("order", [0, 1, 2, 3])
@pytest.mark.parametrize("kind", [1, 2, 3])
def test_against_central_differences(kind, order, d):
    N = 150
    X, y, th = model(kind, N, d)
    Xq = synth.queries(8, d, 5)
    Xq[1] = X[5] + 1e-3                                  # close to a training point, outside the nugget rule's box at +-h
    ref = vargradref.predict(kind, order, X, y, th, Xq)
    h = 1e-5
    fd = np.empty_like(ref["grad"])
    for j in range(d):
        e = np.zeros(d)
        e[j] = h
        fd[:, j] = (vargradref.predict(kind, order, X, y, th, Xq + e)["var"] - vargradref.predict(kind, order, X, y, th, Xq - e)["var"]) / (2.0 * h)
    err = vargradref.error(ref["grad"], fd, ref["kappa"])
    print(f"kind {kind} order {order} d {d}: max |grad - central difference| / max(kappa, |grad|_inf) = {err:.3e}, "
          f"|grad|_inf up to {np.abs(ref['grad']).max():.2f}")
    assert err <= 1e-7


@pytest.mark.parametrize("kind", [2, 3])
def test_matern_against_mpmath_differentiation(kind):
    """var(x*) = kappa - k^T C^-1 k + r^T Q r written out in mpmath (k from the oracle's literal formulas, emulator.c:359,
    452; C's elements as data) and differentiated numerically there; bar 1e-10 max(kappa, |grad|_inf): k in float64 against k
    at 30 digits differs by 2^-53 relative, amplified by cond(C) ~ 1e3 at this nugget"""
    import mpmath as mp
    mp.mp.dps = 30
    N, d, order = 14, 2, 1
    X, y = synth.design(N, d, 77)
    th = np.array([1.3, 0.05, math.log(0.6)])
    Xq = synth.queries(3, d, 8)
    ref = vargradref.predict(kind, order, X, y, th, Xq)
    assert np.all(ref["K"] > 1e-6)                       # nothing near the clamp
    A, nug, rho = mp.mpf(float(th[0])), mp.mpf(float(th[1])), mp.exp(mp.mpf(float(th[2])))
    c = mp.mpf("1.732050808") if kind == 2 else mp.mpf("2.236067978")
    Ci = mp.matrix(O.cov_matrix(kind, X, th).tolist()) ** -1
    H = mp.matrix(O.hmatrix(order, X).tolist())
    W = Ci * H
    Q = (H.T * W) ** -1

    def var(*x):
        k = mp.matrix(N, 1)
        for i in range(N):
            t = mp.sqrt(mp.fsum((x[j] - mp.mpf(float(X[i, j]))) ** 2 for j in range(d))) / rho
            k[i] = A * (1 + c * t + ((mp.mpf(5) / 3) * t * t if kind == 3 else 0)) * mp.exp(-c * t)
        hx = mp.matrix([1] + list(x))
        r = hx - W.T * k
        return (A + nug) - (k.T * Ci * k)[0] + (r.T * Q * r)[0]

    want = np.array([[float(mp.diff(var, tuple(mp.mpf(float(v)) for v in x), tuple(int(i == j) for i in range(d))))
                      for j in range(d)] for x in Xq])
    err = vargradref.error(ref["grad"], want, ref["kappa"])
    print(f"kind {kind}: reference against mpmath differentiation {err:.3e}")
    assert err <= 1e-10


@pytest.mark.parametrize("kind", [1, 3])
def test_longdouble_route_against_mpmath(kind):
    """the written-out longdouble Cholesky and solves against the same computation at 40 digits: 1e-15 of the measures"""
    N, d, order = 40, 3, 2
    X, y, th = model(kind, N, d)
    Xq = synth.queries(4, d, 3)
    Xq[1] = X[3]
    ref = vargradref.predict(kind, order, X, y, th, Xq)
    gl, vl = vargradref.longdouble_route(kind, order, X, y, th, ref["Xq"], ref["K"], ref["G"])
    gm, vm = vargradref.mpmath_route(kind, order, X, y, th, ref["Xq"], ref["K"], ref["G"])
    eg = vargradref.error(gl.astype(np.float64), gm, ref["kappa"])
    ev = float(np.max(np.abs(vl.astype(np.float64) - vm)) / ref["kappa"])
    print(f"kind {kind}: longdouble against mpmath, grad {eg:.3e} var {ev:.3e}; float64 reference {vargradref.reference_errors(kind, order, X, y, th, ref)}")
    assert eg <= 1e-15 and ev <= 1e-15
    assert max(vargradref.reference_errors(kind, order, X, y, th, ref)) <= vargradref.PRECOND


@pytest.mark.parametrize("kind", [1, 2, 3])
def test_far_query_is_the_regression_term(kind):
    """every k under the clamp: r = h and the gradient is 2 h^T Q dh/dx_j"""
    import scipy.linalg as sl
    X, y, th = model(kind, 60, 4)
    order = 3
    x = np.full((1, 4), 30.0)
    ref = vargradref.predict(kind, order, X, y, th, x)
    assert np.all(ref["K"] == 0.0)
    H = O.hmatrix(order, X)
    Q = np.linalg.inv(H.T @ sl.cho_solve(sl.cho_factor(O.cov_matrix(kind, X, th), lower=True), H))
    qh = Q @ O.hmatrix(order, x)[0]
    want = 2.0 * (qh[1:5] + 2.0 * 30.0 * qh[5:9] + 3.0 * 900.0 * qh[9:13])
    assert np.max(np.abs(ref["grad"][0] - want)) <= 1e-13 * np.max(np.abs(want))


def test_error_measure():
    g = np.array([[1.0, 2.0], [0.0, 0.1]])
    r = np.array([[1.0, 4.0], [0.0, 0.0]])
    assert vargradref.error(g, r, 0.5) == max(2.0 / 4.0, 0.1 / 0.5)
