"""CPU references for the leave-one-out tests (tests/test_gpu_loo.py, tests/test_host_loo.py).  Test infrastructure only.

Three routes to "remove training point i, set the emulator up on the other N - 1 points at the same thetas, predict at x_i"
(GLS beta re-estimated; variance with the regression term and kappa = cov(x_i, x_i), nugget included:
emulator.c:672-785, emulator_struct.c:124-143):

  oracle_refits    the oracle's own alloc_emulator_struct + emulate_point on the N - 1 points (clamped k-vector)
  lapack_refits    the same from LAPACK: Cholesky factor of C with row and column i removed, solves
  closed_form      no refit: with P = C^-1 - W Q W^T, var_i = 1 / P_ii, mean_i = y_i - (P y)_i / P_ii  (Dubrule 1983);
                   C^-1 explicitly from LAPACK's dpotri -- another route than the device's (sums over L^-1)

The last two read the covariance matrix itself, whose elements are not clamped; the oracle's k-vector zeroes entries
below 1e-10 (emulator.c:588-590).  min_offdiag() is the precondition under which all three must agree."""
import numpy as np
import scipy.linalg as sl

from oracle import oracle as O

CLAMP = 1e-10


def min_offdiag(Cm):
    """smallest off-diagonal element of a covariance matrix (the diagonal is never the smallest of a row)"""
    N = Cm.shape[0]
    return float(np.min(Cm + np.diag(np.full(N, np.inf))))


def oracle_refits(kind, order, X, y, th, idx):
    m, v = np.empty(len(idx)), np.empty(len(idx))
    for n, i in enumerate(idx):
        keep = np.arange(len(y)) != i
        e = O.Emulator(kind, order, X[keep], y[keep], th)
        assert e.status == 0
        mi, vi, st = e.emulate(X[i:i + 1])
        m[n], v[n] = mi[0], vi[0]
    return m, v


def closed_form(Cm, H, y):
    """-> (mean, var) at every training point from the explicit inverse (dpotrf + dpotri)"""
    N = Cm.shape[0]
    c, info = sl.lapack.dpotrf(Cm, lower=1)
    assert info == 0
    Ci, info = sl.lapack.dpotri(c, lower=1)
    assert info == 0
    del c
    dg = np.diag(Ci).copy()
    Ci = np.tril(Ci) + np.tril(Ci, -1).T
    W = Ci @ H                                   # C^-1 H
    Q = np.linalg.inv(H.T @ W)                   # (H^T C^-1 H)^-1
    beta = Q @ (W.T @ y)
    gamma = Ci @ y - W @ beta                    # (P y) = C^-1 (y - H beta)
    pii = dg - np.einsum("ia,ab,ib->i", W, Q, W)
    assert N == len(pii)
    return y - gamma / pii, 1.0 / pii


def lapack_refits(Cm, H, y, idx):
    """-> (mean, var) at the points idx, each from a Cholesky factorisation of the other N - 1 points"""
    m, v = np.empty(len(idx)), np.empty(len(idx))
    for n, i in enumerate(idx):
        keep = np.arange(len(y)) != i
        Ck = Cm[np.ix_(keep, keep)]
        cf = sl.cho_factor(Ck, lower=True, overwrite_a=True, check_finite=False)
        Hk, yk, k, h = H[keep], y[keep], Cm[keep, i], H[i]
        S = sl.cho_solve(cf, np.column_stack([yk, Hk, k]), check_finite=False)
        Cy, CH, Ck_ = S[:, 0], S[:, 1:-1], S[:, -1]
        Q = np.linalg.inv(Hk.T @ CH)
        beta = Q @ (Hk.T @ Cy)
        q = h - Hk.T @ Ck_
        m[n] = h @ beta + k @ (Cy - CH @ beta)
        v[n] = Cm[i, i] - k @ Ck_ + q @ Q @ q
    return m, v


def errors(m, v, mref, vref, kappa):
    """the two figures the bars are set on: max mean error / max(1, max |mean|), max variance error / kappa"""
    return (float(np.max(np.abs(m - mref)) / max(1.0, np.max(np.abs(mref)))), float(np.max(np.abs(v - vref)) / kappa))
