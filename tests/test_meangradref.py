"""tests/meangradref.py (the reference the device tests of the mean gradient are judged by) against three things that do
not share its formulas: central differences of meanref.predict, mpmath differentiation of the oracle's Matern 5/2 formula,
and cases small enough to work out by hand.  CPU only."""
import math

import numpy as np
import pytest

import meangradref
import meanref
from madaiemulator_amd import synth
from oracle import oracle as O


def model(kind, N, d):
    """the inputs of test_gpu_predict_mean.py::small_model"""
    X, y = synth.design(N, d, 900 + N)
    return X, y + 1.0, synth.default_thetas(kind, d)


@pytest.mark.parametrize("kind,order,N,d", [(k, o, 150, 3) for k in (1, 2, 3) for o in (1, 2, 3)] +
                         [(1, 3, 150, 8), (2, 1, 150, 8), (3, 1, 150, 8), (1, 1, 120, 1), (2, 1, 120, 1), (3, 1, 120, 1),
                          (1, 1, 150, 16), (1, 1, 150, 31)])
def test_against_central_differences(kind, order, N, d):
    """bar 1e-7 max(1, |grad|_inf): the differences' own truncation at h = 1e-5 measures about 2e-9 on these inputs, a wrong
    constant (3 for 1.732050808^2, a dropped factor) shows at 1e-6 and above.  Queries on a training point and 5e-11 from one
    included: the nugget rule's add is constant on its box and the D = 0 term contributes nothing"""
    X, y, th = model(kind, N, d)
    Xq = synth.queries(12, d, 5)
    Xq[1] = X[5]
    Xq[2] = X[7] + 5e-11
    beta, gamma = meanref.trained(kind, order, X, y, th)
    grad, mean, _, _ = meangradref.predict(kind, order, X, th, beta, gamma, Xq)
    m0, _, _ = meanref.predict(kind, order, X, th, beta, gamma, Xq)
    assert np.array_equal(mean, m0) or meanref.error(mean, m0) < 1e-14
    h = 1e-5
    fd = np.empty_like(grad)
    for j in range(d):
        e = np.zeros(d)
        e[j] = h
        fd[:, j] = (meanref.predict(kind, order, X, th, beta, gamma, Xq + e)[0] -
                    meanref.predict(kind, order, X, th, beta, gamma, Xq - e)[0]) / (2.0 * h)
    err = meangradref.error(grad, fd)
    print(f"kind {kind} order {order} d {d}: max |grad - central difference| / max(1, |grad|_inf) = {err:.3e}, "
          f"|grad|_inf up to {np.abs(grad).max():.2f}")
    assert err <= 1e-7


def test_matern52_weight_against_mpmath():
    """k(t) = A (1 + c t / rho + (5/3) (t / rho)^2) exp(-c t / rho) (emulator.c:452-470) differentiated by mpmath along the
    distance t: dk/dt = -g t / rho^2, and at t = 0, where that is 0 = 0, the second derivative -g(0) / rho^2"""
    import mpmath as mp
    mp.mp.dps = 40
    A, rho, c = 1.3, 0.7, mp.mpf("2.236067978")

    def k(t):
        return A * (1 + c * t / rho + (mp.mpf(5) / 3) * (t / rho) ** 2) * mp.exp(-c * t / rho)

    th = np.array([A, 0.01, math.log(rho)])
    for t in (1e-3, 0.1, 0.5, 1.0, 5.0):
        g = meangradref.weights(O.MATERN52, th, np.array([[t, 0.0]]))[0]
        want = float(mp.diff(k, mp.mpf(t)))
        assert abs(-g * t * meangradref.scales(O.MATERN52, th, 2)[0] - want) <= 1e-13 * max(1.0, abs(want))
    g0 = meangradref.weights(O.MATERN52, th, np.zeros((1, 2)))[0]
    want = float(mp.diff(k, mp.mpf(0), 2, direction=1, h=mp.mpf(10) ** -12))
    assert abs(-g0 * meangradref.scales(O.MATERN52, th, 2)[0] - want) <= 1e-8 * abs(want)
    # Matern 3/2 the same way: k = A (1 + c t / rho) exp(-c t / rho), dk/dt = -(A exp(-u)) (c^2 / rho^2) t
    c3 = mp.mpf("1.732050808")

    def k3(t):
        return A * (1 + c3 * t / rho) * mp.exp(-c3 * t / rho)

    for t in (1e-3, 0.3, 2.0):
        g = meangradref.weights(O.MATERN32, th, np.array([[t, 0.0]]))[0]
        want = float(mp.diff(k3, mp.mpf(t)))
        assert abs(-g * t * meangradref.scales(O.MATERN32, th, 2)[0] - want) <= 1e-13 * max(1.0, abs(want))


def test_two_points_by_hand():
    """d = 1, N = 2, order 0, pow-exp: C = [[a + n, c], [c, a + n]], beta = (y_0 + y_1) / 2 by symmetry, gamma =
    +-(y_0 - y_1) / (2 (a + n - c)); the gradient is -s sum_i gamma_i g_i D_i with g_i = a exp(-D_i^2 / (2 r^2))"""
    X = np.array([[0.2], [0.7]])
    y = np.array([1.5, -0.5])
    th = np.array([0.1, -3.0, math.log(0.4)])
    a, n, r = math.exp(0.1), math.exp(-3.0), 0.4
    c = a * math.exp(-0.5 * (0.5 / r) ** 2)
    gam = (y[0] - y[1]) / (2.0 * (a + n - c))
    gamma_hand = np.array([gam, -gam])
    beta, gamma = meanref.trained(O.POWEREXP, 0, X, y, th)
    assert abs(beta[0] - 0.5) < 1e-14 and np.max(np.abs(gamma - gamma_hand)) < 1e-13
    for xs in (0.3, 0.5, 0.95):
        D = xs - X[:, 0]
        want = -(1.0 / r ** 2) * sum(gamma_hand[i] * a * math.exp(-0.5 * (D[i] / r) ** 2) * D[i] for i in range(2))
        grad, _, _, _ = meangradref.predict(O.POWEREXP, 0, X, th, beta, gamma, np.array([[xs]]))
        assert abs(grad[0, 0] - want) <= 1e-13 * max(1.0, abs(want))


@pytest.mark.parametrize("kind", [1, 2, 3])
def test_far_query_is_the_regression_gradient(kind):
    """every k under the clamp: the gradient is sum_a beta_a dh_a/dx_j exactly"""
    X, y, th = model(kind, 60, 4)
    order = 3
    beta, gamma = meanref.trained(kind, order, X, y, th)
    x = np.full((1, 4), 30.0)
    grad, _, _, K = meangradref.predict(kind, order, X, th, beta, gamma, x)
    assert np.all(K == 0.0)
    want = beta[1:5] + 2.0 * 30.0 * beta[5:9] + 3.0 * 900.0 * beta[9:13]
    assert np.max(np.abs(grad[0] - want)) <= 1e-15 * np.max(np.abs(want))
