"""CPU reference for the gradient of the posterior variance with respect to the query point (tests/test_gpu_var_grad.py,
tests/test_vargradref.py).  Test infrastructure only; no device value enters.

  var(x*) = kappa - k^T C^-1 k + r^T Q r,   r = h(x*) - W^T k,  W = C^-1 H,  Q = (H^T C^-1 H)^-1      (emulator.c:720-785)

kappa = cov(x*, x*) is constant, and d k_i / d x*_j = -g_i s_j D_ij with D_ij = x*_j - x_ij and the g_i, s_j of meangradref
(g_i = 0 wherever the oracle's clamped k-vector is zero), so that with a = C^-1 k + W Q r

  d var / d x*_j = 2 s_j sum_i a_i g_i D_ij + 2 sum_a (Q r)_a dh_a/dx_j (x*).

C, H and the k-vectors come from the oracle's element routines, the solves from LAPACK (cho_factor / cho_solve), the
weights from numpy.  beta and gamma (for the mean beside it) from meanref.trained.

This gradient goes through C^-1 k: its rounding grows with cond(C), in the reference as on the device.  reference()
therefore checks the reference before it hands it out: the linear algebra is repeated in extended precision -- a
Cholesky factorisation and the solves written out here on numpy's longdouble (x87 extended, 2^-63; when the platform's
longdouble is no wider than a double: on mpmath at 40 digits) from the SAME matrix elements, k-vectors and weights -- and the
two must agree to PRECOND = 1e-10 of the measure the device bar is set on, two orders below that bar:

  error = max over the queries of  max_j |g_j - ref_j| / max(kappa, max_j |ref_j|)

(kappa: the scale of the variance tests' bar, "1e-8 kappa").  The variance is checked the same way against 1e-10 kappa.
tests/test_vargradref.py checks the longdouble route itself against mpmath on a small case."""
import numpy as np
import scipy.linalg as sl

import meangradref
import meanref
from oracle import oracle as O

RTOL = 1e-8                      # the bar of the device tests
PRECOND = 1e-10                  # float64 reference against the extended-precision one
EPS = 2.0 ** -52
LD = np.longdouble
LD_IS_EXTENDED = np.finfo(LD).eps < 1e-18


def kappa(kind, th):
    """cov(x*, x*), nugget included (emulator_struct.c:135)"""
    th = np.asarray(th, dtype=np.float64)
    return float(np.exp(th[0]) + np.exp(th[1])) if kind == O.POWEREXP else float(th[0] + th[1])


def masked_weights(kind, X, th, Xq, K):
    """G[m, i] = g_i of query m, zero where the clamped k value is zero"""
    return np.vstack([np.where(K[m] == 0.0, 0.0, meangradref.weights(kind, th, x - X)) for m, x in enumerate(Xq)])


def dbasis_rows(order, Xq, C):
    """sum_a C[m, a] dh_a/dx_j at the rows of Xq (meangradref.dbasis with a coefficient vector per query)"""
    return np.vstack([meangradref.dbasis(order, x, c) for x, c in zip(Xq, C)])


def assemble(X, Xq, s, A, G, dh, dtype=np.float64):
    """grad[m, j] = 2 s_j sum_i A[m, i] G[m, i] (x*_mj - x_ij) + 2 dh[m, j] in the arithmetic of dtype"""
    X, Xq, s = X.astype(dtype), Xq.astype(dtype), s.astype(dtype)
    Wt = A.astype(dtype) * G.astype(dtype)
    # sum_i w_i (x*_j - x_ij) term by term, as written: no cancellation between x*_j sum w and sum w x_ij is introduced
    T = np.stack([(Wt[m][:, None] * (Xq[m] - X)).sum(axis=0) for m in range(Xq.shape[0])])
    return 2 * (s * T + dh.astype(dtype))


def float64_route(kind, order, X, y, th, Xq, K, G):
    """-> (grad, var, Qr) from LAPACK in float64"""
    N, d = X.shape
    Cm = O.cov_matrix(kind, X, th)
    H = O.hmatrix(order, X)
    cf = sl.cho_factor(Cm, lower=True, check_finite=False)
    W = sl.cho_solve(cf, H, check_finite=False)
    Q = np.linalg.inv(H.T @ W)
    CiK = sl.cho_solve(cf, K.T, check_finite=False).T              # rows C^-1 k
    R = O.hmatrix(order, Xq) - K @ W
    QR = R @ Q.T
    var = kappa(kind, th) - np.einsum("mi,mi->m", K, CiK) + np.einsum("ma,ma->m", R, QR)
    A = CiK + QR @ W.T
    grad = assemble(X, Xq, meangradref.scales(kind, th, d), A, G, dbasis_rows(order, Xq, QR))
    return grad, var, QR


# ---- the same in extended precision, written out
def chol_ld(A):
    A = A.astype(LD)
    N = A.shape[0]
    L = np.zeros((N, N), dtype=LD)
    for j in range(N):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        assert v[0] > 0
        L[j, j] = np.sqrt(v[0])
        L[j + 1:, j] = v[1:] / L[j, j]
    return L


def solve_ld(L, B):
    """C^-1 B for C = L L^T"""
    B = B.astype(LD).copy()
    N = L.shape[0]
    for i in range(N):
        B[i] = (B[i] - L[i, :i] @ B[:i]) / L[i, i]
    for i in range(N - 1, -1, -1):
        B[i] = (B[i] - L[i + 1:, i] @ B[i + 1:]) / L[i, i]
    return B


def inv_spd_ld(S):
    return solve_ld(chol_ld(S), np.eye(S.shape[0], dtype=LD))


def longdouble_route(kind, order, X, y, th, Xq, K, G):
    N, d = X.shape
    L = chol_ld(O.cov_matrix(kind, X, th))
    H = O.hmatrix(order, X).astype(LD)
    Kl = K.astype(LD)
    S = solve_ld(L, np.column_stack([H, Kl.T]))
    W, CiK = S[:, :H.shape[1]], S[:, H.shape[1]:].T
    Q = inv_spd_ld(H.T @ W)
    R = O.hmatrix(order, Xq).astype(LD) - Kl @ W
    QR = R @ Q.T
    var = LD(kappa(kind, th)) - (Kl * CiK).sum(axis=1) + (R * QR).sum(axis=1)
    A = CiK + QR @ W.T
    Xl = Xq.astype(LD)
    dh = np.zeros((Xq.shape[0], d), dtype=LD)
    for o in range(1, order + 1):
        dh += o * Xl ** (o - 1) * QR[:, 1 + (o - 1) * d:1 + o * d]
    grad = assemble(X, Xq, meangradref.scales(kind, th, d), A, G, dh, LD)
    return grad, var


def mpmath_route(kind, order, X, y, th, Xq, K, G, dps=40):
    """the extended route on mpmath (slow: small cases, or a platform without an extended longdouble) -> float64 arrays of
    the values rounded once"""
    import mpmath as mp
    with mp.workdps(dps):
        N, d = X.shape
        M = Xq.shape[0]
        Cm = mp.matrix(O.cov_matrix(kind, X, th).tolist())
        H = mp.matrix(O.hmatrix(order, X).tolist())
        Kt = mp.matrix(K.T.tolist())
        Ci = Cm ** -1                                                     # (at 40 digits the explicit inverse loses nothing that matters)
        W, CiK = Ci * H, Ci * Kt
        Q = (H.T * W) ** -1
        R = mp.matrix(O.hmatrix(order, Xq).tolist()) - Kt.T * W          # M x nreg
        QR = R * Q.T
        A = CiK.T + QR * W.T                                              # M x N
        s = meangradref.scales(kind, th, d)
        grad, var = np.empty((M, d)), np.empty(M)
        kap = mp.mpf(kappa(kind, th))
        for m in range(M):
            var[m] = float(kap - mp.fsum(Kt[i, m] * CiK[i, m] for i in range(N)) + mp.fsum(R[m, a] * QR[m, a] for a in range(R.cols)))
            for j in range(d):
                t = mp.fsum(A[m, i] * mp.mpf(float(G[m, i])) * (mp.mpf(float(Xq[m, j])) - mp.mpf(float(X[i, j]))) for i in range(N))
                dh = mp.fsum(o * mp.mpf(float(Xq[m, j])) ** (o - 1) * QR[m, 1 + (o - 1) * d + j] for o in range(1, order + 1))
                grad[m, j] = float(2 * (mp.mpf(float(s[j])) * t + dh))
    return grad, var


def error(g, gref, kap):
    """the figure the bars are set on: max over the queries of max_j |g - gref| / max(kappa, max_j |gref|)"""
    g, gref = np.asarray(g), np.asarray(gref)
    return float(np.max(np.max(np.abs(g - gref), axis=1) / np.maximum(kap, np.max(np.abs(gref), axis=1))))


def predict(kind, order, X, y, th, Xq, far=()):
    """-> dict(grad, var, mean, K, G, QR, kappa, vscale, A, Xq) in float64, unchecked.  vscale: the per-query scale of the
    variance bar, kappa -- except for the queries listed in far (every k under the clamp, coordinates of 30 and more), whose
    variance kappa + h^T Q h grows with |h|: max(kappa, |var|) there, as tests/test_gpu_predict_paths.py has it"""
    X = np.ascontiguousarray(X, dtype=np.float64)
    Xq = np.ascontiguousarray(Xq, dtype=np.float64).reshape(-1, X.shape[1])
    K = np.vstack([O.kvector(kind, X, q, th) for q in Xq])
    G = masked_weights(kind, X, th, Xq, K)
    grad, var, QR = float64_route(kind, order, X, y, th, Xq, K, G)
    beta, gamma = meanref.trained(kind, order, X, y, th)
    terms = K * gamma
    mean = O.hmatrix(order, Xq) @ beta + terms.sum(axis=1)
    A = np.abs(terms).sum(axis=1) / np.maximum(1.0, np.abs(mean))
    vscale = np.full(var.size, kappa(kind, th))
    for q in far:
        vscale[q] = max(vscale[q], abs(var[q]))
    return dict(grad=grad, var=var, mean=mean, K=K, G=G, QR=QR, kappa=kappa(kind, th), vscale=vscale, A=A, Xq=Xq)


def reference_errors(kind, order, X, y, th, ref):
    """-> (gradient, variance) error of the float64 reference against the extended-precision one, in the bars' measures"""
    route = longdouble_route if LD_IS_EXTENDED else mpmath_route
    gx, vx = route(kind, order, np.ascontiguousarray(X, dtype=np.float64), y, th, ref["Xq"], ref["K"], ref["G"])
    kap = ref["kappa"]
    eg = float(np.max(np.max(np.abs(ref["grad"] - gx), axis=1) / np.maximum(kap, np.max(np.abs(gx), axis=1))))
    ev = float(np.max(np.abs(ref["var"] - vx) / ref["vscale"]))
    return eg, ev


def reference(kind, order, X, y, th, Xq, far=()):
    """predict(), after asserting that the reference is good to PRECOND on these inputs (gradient and variance against the
    extended-precision route, the mean through meanref's A N 2^-52); the measured figures come back as 'ref_err'"""
    ref = predict(kind, order, X, y, th, Xq, far)
    eg, ev = reference_errors(kind, order, X, y, th, ref)
    ea = float(ref["A"].max()) * X.shape[0] * EPS
    assert eg <= PRECOND and ev <= PRECOND and ea <= PRECOND, ("ill-conditioned test inputs: reference errors (grad, var, mean)", eg, ev, ea)
    ref["ref_err"] = (eg, ev, ea)
    return ref
