"""CPU reference for the joint posterior covariance between query points (tests/test_gpu_predict_cov.py,
tests/test_host_cov.py, tests/test_predcovref.py).  Test infrastructure only; no device value enters.

  Sigma_pq = c(x*_p, x*_q) - k_p^T C^-1 k_q + r_p^T Q r_q,   r_p = h(x*_p) - W^T k_p,  W = C^-1 H,  Q = (H^T C^-1 H)^-1

c(.,.) between two queries is the oracle's makeCovMatrix on the query rows (not clamped, nugget wherever every coordinate
differs by less than the kernel's box), k_p the oracle's clamped k-vector, C and H the oracle's matrices, the solves LAPACK's
(cho_factor / cho_solve): the pattern of vargradref.float64_route.

Like vargradref.reference, reference() checks itself before it hands anything out: the linear algebra is repeated on numpy's
longdouble (vargradref.chol_ld / solve_ld; mpmath at 40 digits where longdouble is no wider than double) from the SAME
matrix elements, and the two must agree to PRECOND = 1e-10 of the scale the device bar is set on,

  error = max_pq |S_pq - ref_pq| / max(vscale_p, vscale_q),

vscale = kappa, or max(kappa, |var|) for the queries listed as far (vargradref.predict's rule).  The mean beside it carries
meanref's precondition A N 2^-52 <= 1e-10.  saddle_route states the same matrix a third way (tests/test_predcovref.py)."""
import numpy as np
import scipy.linalg as sl

import meanref
import vargradref
from oracle import oracle as O

RTOL = vargradref.RTOL           # the bar of the device tests
PRECOND = vargradref.PRECOND     # float64 reference against the extended-precision one
EPS = vargradref.EPS
LD = vargradref.LD


def kvectors(kind, X, th, Xq):
    return np.vstack([O.kvector(kind, X, q, th) for q in Xq])


def float64_route(kind, order, X, th, Xq, K):
    """-> Sigma (M x M) from LAPACK in float64"""
    Cm = O.cov_matrix(kind, X, th)
    H = O.hmatrix(order, X)
    cf = sl.cho_factor(Cm, lower=True, check_finite=False)
    W = sl.cho_solve(cf, H, check_finite=False)
    Q = np.linalg.inv(H.T @ W)
    CiK = sl.cho_solve(cf, K.T, check_finite=False)               # columns C^-1 k
    R = O.hmatrix(order, Xq) - K @ W
    return O.cov_matrix(kind, Xq, th) - K @ CiK + R @ Q @ R.T


def longdouble_route(kind, order, X, th, Xq, K):
    """the same on numpy's longdouble, Cholesky and solves written out (vargradref)"""
    L = vargradref.chol_ld(O.cov_matrix(kind, X, th))
    H = O.hmatrix(order, X).astype(LD)
    Kl = K.astype(LD)
    S = vargradref.solve_ld(L, np.column_stack([H, Kl.T]))
    W, CiK = S[:, :H.shape[1]], S[:, H.shape[1]:]
    Q = vargradref.inv_spd_ld(H.T @ W)
    R = O.hmatrix(order, Xq).astype(LD) - Kl @ W
    return O.cov_matrix(kind, Xq, th).astype(LD) - Kl @ CiK + R @ Q @ R.T


def mpmath_route(kind, order, X, th, Xq, K, dps=40):
    """the extended route on mpmath (a platform without an extended longdouble) -> float64 array of the values rounded once"""
    import mpmath as mp
    with mp.workdps(dps):
        Ci = mp.matrix(O.cov_matrix(kind, X, th).tolist()) ** -1
        H = mp.matrix(O.hmatrix(order, X).tolist())
        Km = mp.matrix(K.tolist())
        W = Ci * H
        Q = (H.T * W) ** -1
        R = mp.matrix(O.hmatrix(order, Xq).tolist()) - Km * W
        S = mp.matrix(O.cov_matrix(kind, Xq, th).tolist()) - Km * Ci * Km.T + R * Q * R.T
        return np.array([[float(S[i, j]) for j in range(S.cols)] for i in range(S.rows)])


def extended_route(kind, order, X, th, Xq, K):
    return (longdouble_route if vargradref.LD_IS_EXTENDED else mpmath_route)(kind, order, X, th, Xq, K)


def saddle_route(kind, order, X, th, Xq, K, sweeps=6):
    """Sigma = C** - [K H*] [[C, H], [H^T, 0]]^-1 [K H*]^T: the universal-kriging system solved as ONE indefinite system --
    LAPACK's LU in float64 as the approximate inverse, residuals and updates in longdouble (iterative refinement) -- which
    shares neither the Cholesky factor nor W, Q, r with the routes above"""
    N = X.shape[0]
    H = O.hmatrix(order, X)
    nreg = H.shape[1]
    A = np.zeros((N + nreg, N + nreg))
    A[:N, :N] = O.cov_matrix(kind, X, th)
    A[:N, N:] = H
    A[N:, :N] = H.T
    B = np.column_stack([K, O.hmatrix(order, Xq)]).T             # (N + nreg) x M
    lu = sl.lu_factor(A, check_finite=False)
    Al, Bl = A.astype(LD), B.astype(LD)
    Z = np.zeros_like(Bl)
    for _ in range(sweeps):
        res = Bl - Al @ Z
        Z = Z + sl.lu_solve(lu, res.astype(np.float64), check_finite=False).astype(LD)
    return O.cov_matrix(kind, Xq, th).astype(LD) - Bl.T @ Z


def error(S, Sref, vscale):
    """the figure the bars are set on: max_pq |S_pq - ref_pq| / max(vscale_p, vscale_q)"""
    vs = np.asarray(vscale, dtype=np.float64)
    return float(np.max(np.abs(np.asarray(S - Sref, dtype=np.float64)) / np.maximum(vs[:, None], vs[None, :])))


def predict(kind, order, X, y, th, Xq, far=()):
    """-> dict(cov, var, mean, K, kappa, vscale, A, Xq) in float64, unchecked"""
    X = np.ascontiguousarray(X, dtype=np.float64)
    Xq = np.ascontiguousarray(Xq, dtype=np.float64).reshape(-1, X.shape[1])
    K = kvectors(kind, X, th, Xq)
    S = float64_route(kind, order, X, th, Xq, K)
    var = np.diag(S).copy()
    beta, gamma = meanref.trained(kind, order, X, y, th)
    terms = K * gamma
    mean = O.hmatrix(order, Xq) @ beta + terms.sum(axis=1)
    A = np.abs(terms).sum(axis=1) / np.maximum(1.0, np.abs(mean))
    kap = vargradref.kappa(kind, th)
    vscale = np.full(var.size, kap)
    for q in far:
        vscale[q] = max(vscale[q], abs(var[q]))
    return dict(cov=S, var=var, mean=mean, K=K, kappa=kap, vscale=vscale, A=A, Xq=Xq)


def reference_error(kind, order, X, th, ref, rows=None):
    """error of the float64 reference against the extended-precision one in the bar's measure; rows: the queries whose
    sub-block is repeated (every element depends on its own two queries only) -- all of them when None"""
    sel = np.arange(ref["Xq"].shape[0]) if rows is None else np.asarray(rows)
    Sx = extended_route(kind, order, np.ascontiguousarray(X, dtype=np.float64), th, ref["Xq"][sel], ref["K"][sel])
    return error(ref["cov"][np.ix_(sel, sel)], Sx, ref["vscale"][sel])


def reference(kind, order, X, y, th, Xq, far=(), rows=None):
    """predict(), after asserting that the reference is good to PRECOND on these inputs; the measured figures come back as
    'ref_err' = (covariance against the extended-precision route, the mean's A N 2^-52)"""
    ref = predict(kind, order, X, y, th, Xq, far)
    ec = reference_error(kind, order, X, th, ref, rows)
    ea = float(ref["A"].max()) * X.shape[0] * EPS
    assert ec <= PRECOND and ea <= PRECOND, ("ill-conditioned test inputs: reference errors (cov, mean)", ec, ea)
    ref["ref_err"] = (ec, ea)
    return ref
