"""CPU reference for the mean-only prediction tests (tests/test_gpu_predict_mean.py).  Test infrastructure only.

  mean(x*) = h(x*)^T beta + sum_i k(x_i, x*) gamma_i ,   gamma = C^-1 (y - H beta)      (emulator.c:672-704)

with C, h and the k-vector (clamp of emulator.c:588-590 included) from the oracle's own element routines and the solves from
LAPACK (cho_factor / cho_solve) -- no device value enters.  Beside the mean it returns the amplification

  A = sum_i |k_i gamma_i| / max(1, |mean|)

per query: rounding in ANY summation order of the N products stays below A * N * 2^-52 relative to max(1, |mean|), which is
what the tests assert to be two orders under their bar before they compare anything."""
import numpy as np
import scipy.linalg as sl

from oracle import oracle as O

RTOL = 1e-8                      # the project's prediction bar (tests/test_gpu_loo.py)
PRECOND = 1e-10                  # A * N * 2^-52 must not exceed this
EPS = 2.0 ** -52


def trained(kind, order, X, y, th):
    """-> (beta, gamma) of the emulator trained on (X, y) at thetas th"""
    Cm = O.cov_matrix(kind, X, th)
    H = O.hmatrix(order, X)
    cf = sl.cho_factor(Cm, lower=True, overwrite_a=True, check_finite=False)
    S = sl.cho_solve(cf, np.column_stack([y, H]), check_finite=False)
    Cy, CH = S[:, 0], S[:, 1:]
    beta = np.linalg.solve(H.T @ CH, H.T @ Cy)
    return beta, Cy - CH @ beta


def predict(kind, order, X, th, beta, gamma, Xq):
    """-> (mean, h^T beta, A) at every row of Xq"""
    Xq = np.ascontiguousarray(Xq, dtype=np.float64).reshape(-1, X.shape[1])
    hb = O.hmatrix(order, Xq) @ beta
    K = np.vstack([O.kvector(kind, X, q, th) for q in Xq])
    terms = K * gamma
    mean = hb + terms.sum(axis=1)
    return mean, hb, np.abs(terms).sum(axis=1) / np.maximum(1.0, np.abs(mean))


def reference(kind, order, X, y, th, Xq):
    """-> (mean, h^T beta, A); asserts the precondition A * N * 2^-52 <= 1e-10 on these inputs"""
    beta, gamma = trained(kind, order, X, y, th)
    mean, hb, A = predict(kind, order, X, th, beta, gamma, Xq)
    worst = float(A.max()) * X.shape[0] * EPS
    assert worst <= PRECOND, ("ill-conditioned test inputs: A N eps =", worst)
    return mean, hb, A


def error(m, mref):
    """the figure the bar is set on: max |m - mref| / max(1, max |mref|)"""
    return float(np.max(np.abs(m - mref)) / max(1.0, np.max(np.abs(mref))))
