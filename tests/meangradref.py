"""CPU reference for the gradient of the posterior mean with respect to the query point (tests/test_gpu_mean_grad.py,
tests/test_meangradref.py).  Test infrastructure only; no device value enters.

With D_j = x*_j - x_ij every covariance function of the library has  d k(x_i, x*) / d x*_j = -g_i s_j D_j :

  pow-exp      s_j = exp(-2 theta_{2+j})   g_i = A exp(-1/2 sum_k D_k^2 / r_k^2)                 (the k value before the nugget)
  Matern 3/2   s_j = c^2 / rho^2           g_i = A exp(-u)                                       c = 1.732050808, u = c |D| / rho
  Matern 5/2   s_j = 1 / rho^2             g_i = A exp(-u) ((c^2 - 10/3) + (5/3) u)              c = 2.236067978

(the reference's literal roots, emulator.c:359, 452), so that

  d mean / d x*_j = sum_a beta_a dh_a/dx_j (x*)  -  s_j sum_i gamma_i g_i (x*_j - x_ij)

beta and gamma come from meanref.trained (oracle covariance values, LAPACK solves); g_i = 0 wherever the oracle's clamped
k-vector (makeKVector_fnptr, emulator.c:578-593: nugget rule, then < 1e-10 -> 0) is zero: the gradient of the function the
mean sweep evaluates.  The weights are evaluated here in numpy.  Beside the gradient comes the conditioning figure

  B = max_j s_j sum_i |gamma_i g_i| (|x*_j - mid_j| + |x_ij - mid_j|) / max(1, max_j |grad_j|)

(mid: the centre of the design's box): rounding in ANY summation order of the N terms on the centred design stays below
B * N * 2^-52 relative to max(1, |grad|_inf); reference() asserts that this is two orders under the tests' bar."""
import numpy as np

import meanref
from oracle import oracle as O

RTOL = 1e-8                      # the bar of the device tests, per query, relative to max(1, |grad|_inf)
PRECOND = 1e-10                  # B * N * 2^-52 must not exceed this
EPS = 2.0 ** -52
ROOT3, ROOT5 = 1.732050808, 2.236067978


def scales(kind, th, d):
    """s_j"""
    th = np.asarray(th, dtype=np.float64)
    if kind == O.POWEREXP:
        return np.exp(-2.0 * th[2:2 + d])
    rho = np.exp(th[2])
    return np.full(d, (ROOT3 * ROOT3 if kind == O.MATERN32 else 1.0) / (rho * rho))


def weights(kind, th, D):
    """g_i for the rows D_i = x* - x_i, before the clamp"""
    th = np.asarray(th, dtype=np.float64)
    if kind == O.POWEREXP:
        r = np.exp(th[2:2 + D.shape[1]])
        return np.exp(th[0]) * np.exp(-0.5 * np.sum((D / r) ** 2, axis=1))
    rho = np.exp(th[2])
    dist = np.sqrt(np.sum(D * D, axis=1))
    if kind == O.MATERN32:
        return th[0] * np.exp(-ROOT3 * dist / rho)
    u = ROOT5 * dist / rho
    return th[0] * np.exp(-u) * ((ROOT5 * ROOT5 - 10.0 / 3.0) + (5.0 / 3.0) * u)


def dbasis(order, x, beta):
    """sum_a beta_a dh_a/dx_j at x: the basis is 1, x_j, x_j^2, x_j^3 with coefficient 1 + (o - 1) d + j on x_j^o"""
    d = x.size
    g = np.zeros(d)
    for o in range(1, order + 1):
        g += o * x ** (o - 1) * beta[1 + (o - 1) * d:1 + o * d]
    return g


def predict(kind, order, X, th, beta, gamma, Xq):
    """-> (grad[M, d], mean[M], B[M], K[M, N]) at every row of Xq"""
    X = np.ascontiguousarray(X, dtype=np.float64)
    N, d = X.shape
    Xq = np.ascontiguousarray(Xq, dtype=np.float64).reshape(-1, d)
    mid = 0.5 * (X.max(axis=0) + X.min(axis=0))
    s = scales(kind, th, d)
    grad, B = np.empty((Xq.shape[0], d)), np.empty(Xq.shape[0])
    K = np.vstack([O.kvector(kind, X, q, th) for q in Xq])
    for m, x in enumerate(Xq):
        D = x - X
        w = gamma * np.where(K[m] == 0.0, 0.0, weights(kind, th, D))
        grad[m] = dbasis(order, x, beta) - s * (w @ D)
        B[m] = np.max(s * (np.abs(w) @ (np.abs(x - mid) + np.abs(X - mid)))) / max(1.0, np.max(np.abs(grad[m])))
    mean = O.hmatrix(order, Xq) @ beta + (K * gamma).sum(axis=1)
    return grad, mean, B, K


def reference(kind, order, X, y, th, Xq):
    """-> (grad, mean, B, K); asserts the preconditions B * N * 2^-52 <= 1e-10 and meanref's A * N * 2^-52 <= 1e-10"""
    beta, gamma = meanref.trained(kind, order, X, y, th)
    grad, mean, B, K = predict(kind, order, X, th, beta, gamma, Xq)
    worst = float(B.max()) * X.shape[0] * EPS
    assert worst <= PRECOND, ("ill-conditioned test inputs: B N eps =", worst)
    A = np.abs(K * gamma).sum(axis=1) / np.maximum(1.0, np.abs(mean))
    assert float(A.max()) * X.shape[0] * EPS <= PRECOND, ("ill-conditioned test inputs: A N eps =", float(A.max()) * X.shape[0] * EPS)
    return grad, mean, B, K


def error(g, gref):
    """the figure the bar is set on: max over the queries of max_j |g - gref| / max(1, max_j |gref|)"""
    return float(np.max(np.max(np.abs(g - gref), axis=1) / np.maximum(1.0, np.max(np.abs(gref), axis=1))))
