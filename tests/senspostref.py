"""CPU references for the emulator-uncertainty terms of the closed-form sensitivity analysis (gpemu_sens_post /
gpemu_sens_main_var, include/gpemu.h).  Test infrastructure only; no device value enters except as an INPUT.

f is the posterior process of a power-exponential emulator, without k-vector clamp and without nugget,

  c*(x, x') = c(x, x') - k^T P k' + h^T Q h' - h^T G^T k' - k^T G h',   P = C^-1 - W Q W^T,  G = W Q,  W = C^-1 H,

and S_u = E_{x_u} Var*[E[f | x_u]] is c* integrated over the box with the coordinates of u shared between x and x'.  The
references take P, G and Q as inputs (the device's own, or `fit_state`'s from numpy) beside the model dict of sensref.py
(A, s; beta and gamma are not needed: the uncertainty does not depend on the training values):

  1. `post` / `band` with the NP backend: the closed forms in numpy fp64, tables from sensref.py,
  2. the same with the MP backend: mpmath at 50 digits,
  3. `quadrature_post` / `quadrature_band`: tensor Gauss-Legendre quadrature of c* itself on all pairs of nodes (d <= 3).

Every value comes with its SCALE |CC_u| + A^2 sum |P_ii'| KK_u + sum |Q_ab Hm_u| + 2 sum |G_ia HK_u|.

`python tests/senspostref.py --measure` prints the largest scaled error of backend 1 against backend 2 over the cases of
tests/test_gpu_sens_post.py, and the discrepancy of the two routes to C^-1 on the CPU; both are written down in that file."""
import numpy as np

import sensref as R

KEYS = ("s_none", "s_all", "s_first", "s_rest")


# ---------------------------------------------------------------------------------------------------- pieces
def _expm1(B, x):
    return B.exp(x) - 1 if isinstance(B, R.MP) else np.expm1(x)


def _erf(B, x):
    return B.derf(x * 0, x)


def uu(B, s, lo, hi):
    """UU_l = (1 / w^2) int int k_l dx dx' = (2 / w^2) [w sqrt(pi / 2 s) erf(a) - (1 - e^{-a^2}) / s],  a = w sqrt(s / 2)"""
    w = hi - lo
    a = w * B.sqrt(s / 2)
    return 2 / (w * w) * (w * B.sqrt(B.pi / (2 * s)) * _erf(B, a) + _expm1(B, -a * a) / s)


def basis_index(d, order):
    """-> [(p, l)] of the regression functions 1 .. nreg - 1 (the constant is function 0)"""
    return [(p, l) for p in range(1, order + 1) for l in range(d)]


def _subsets(d):
    """the 2 d + 2 sets u as boolean lists, in the order none, all, {j}, all but j"""
    return ([[False] * d, [True] * d] + [[l == j for l in range(d)] for j in range(d)]
            + [[l != j for l in range(d)] for j in range(d)])


def _pack(vals, d):
    return dict(s_none=vals[0], s_all=vals[1], s_first=vals[2:2 + d], s_rest=vals[2 + d:])


def _asum(x):
    return abs(x).sum()


def post(B, X, model, P, G, Q, lo, hi):
    """-> (dict(s_none, s_all, s_first [d], s_rest [d]), the same keys with the scales), float arrays"""
    X, lo, hi = B.arr(X), B.arr(lo), B.arr(hi)
    P, G, Q = B.arr(P), B.arr(G), B.arr(Q)
    N, d = X.shape
    nreg = Q.shape[0]
    order = (nreg - 1) // d
    A, s = B.arr(model["A"])[()], B.arr(model["s"])
    M = R.moments(B, lo, hi)
    IJ = R.point_integrals(B, X, s, lo, hi)
    PI, Pex = R.leave_one_out(IJ[0])
    II = R.pair_integrals(B, X, s, s, lo, hi)
    IIall, IIex = R.leave_one_out(II)
    UU = uu(B, s, lo, hi)
    idx = basis_index(d, order)
    Eh = np.array([lo[0] * 0 + 1] + [M[p][l] for p, l in idx], dtype=object if isinstance(B, R.MP) else float)
    vals, scls = [], []
    for inu in _subsets(d):
        cc = A + lo[0] * 0
        KK = IIall * 0 + 1
        for l in range(d):
            if inu[l]:
                KK = KK * II[:, :, l]
            else:
                cc = cc * UU[l]
                KK = KK * IJ[0][:, None, l] * IJ[0][None, :, l]
        Hm = Eh[:, None] * Eh[None, :]
        HK = Eh[:, None] * (A * PI)[None, :]                    # nreg x N
        for a, (p, l) in enumerate(idx, start=1):
            if inu[l]:
                HK[a] = A * IJ[p][:, l] * Pex[:, l]
                for b, (q, m) in enumerate(idx, start=1):
                    if m == l:
                        Hm[a, b] = M[p + q][l]
        kk, hq, hk = A * A * P * KK, Q * Hm, 2 * G * HK.T
        vals.append(cc - kk.sum() + hq.sum() - hk.sum())
        scls.append(abs(cc) + _asum(kk) + _asum(hq) + _asum(hk))
    return ({k: B.tofloat(v) for k, v in _pack(vals, d).items()}, {k: B.tofloat(v) for k, v in _pack(scls, d).items()})


def band(B, X, model, P, G, Q, beta, gamma, lo, hi, grid):
    """grid[j][g] -> (dict(main [d x G], var [d x G], var_e0), scales): var[j][g] = Var*[E[f | x_j = grid[j][g]]]
       = A prod_{l != j} UU_l - T^T P T + hm^T Q hm - 2 hm^T G^T T,  T_i = A k_j(x_ij, x) Pex_j(i)"""
    X, lo, hi, grid = B.arr(X), B.arr(lo), B.arr(hi), B.arr(grid)
    P, G, Q, beta, gamma = B.arr(P), B.arr(G), B.arr(Q), B.arr(beta), B.arr(gamma)
    N, d = X.shape
    nreg = Q.shape[0]
    order = (nreg - 1) // d
    A, s = B.arr(model["A"])[()], B.arr(model["s"])
    M = R.moments(B, lo, hi)
    IJ = R.point_integrals(B, X, s, lo, hi)
    PI, Pex = R.leave_one_out(IJ[0])
    UU = uu(B, s, lo, hi)
    idx = basis_index(d, order)
    one = lo[0] * 0 + 1

    def value(T, hm, cc):
        tp, hq, hg = P * T[:, None] * T[None, :], Q * hm[:, None] * hm[None, :], 2 * G * T[:, None] * hm[None, :]
        return (cc - tp.sum() + hq.sum() - hg.sum(), abs(cc) + _asum(tp) + _asum(hq) + _asum(hg),
                (T * gamma).sum() + (hm * beta).sum(), abs(T * gamma).sum() + abs(hm * beta).sum())

    var, vscl, main, mscl = [], [], [], []
    for j in range(d):
        cc = A * one
        for l in range(d):
            if l != j:
                cc = cc * UU[l]
        for x in grid[j]:
            T = A * B.exp(-s[j] * (x - X[:, j]) ** 2 / 2) * Pex[:, j]
            hm = np.array([one] + [x ** p if l == j else M[p][l] for p, l in idx], dtype=T.dtype)
            v, vs, m, ms = value(T, hm, cc)
            var.append(v); vscl.append(vs); main.append(m); mscl.append(ms)
    cc = A * one
    for l in range(d):
        cc = cc * UU[l]
    T0 = A * PI
    v0, v0s, _, _ = value(T0, np.array([one] + [M[p][l] for p, l in idx], dtype=T0.dtype), cc)
    G_ = grid.shape[1]
    shp = lambda v: B.tofloat(np.array(v, dtype=object)).reshape(d, G_)
    return (dict(main=shp(main), var=shp(var), var_e0=B.tofloat(v0)), dict(main=shp(mscl), var=shp(vscl), var_e0=B.tofloat(v0s)))


# ---------------------------------------------------------------------------------------------------- a fit in numpy
def hmatrix(X, order):
    X = np.asarray(X, float)
    return np.hstack([np.ones((len(X), 1))] + [X ** p for p in range(1, order + 1)])


def kmatrix(Xa, Xb, s):
    D2 = ((np.asarray(Xa, float)[:, None, :] - np.asarray(Xb, float)[None, :, :]) ** 2 * s).sum(axis=2)
    return np.exp(-D2 / 2)


def fit_state(X, y, order, A, s, nugget):
    """-> (P, G, Q, beta, gamma, Cinv, W) of the emulator with C = A K + nugget I, by numpy's inverse"""
    C = A * kmatrix(X, X, s) + nugget * np.eye(len(X))
    H = hmatrix(X, order)
    Cinv = np.linalg.inv(C)
    Cinv = (Cinv + Cinv.T) / 2
    W = Cinv @ H
    Q = np.linalg.inv(H.T @ W)
    Q = (Q + Q.T) / 2
    beta = Q @ (W.T @ y)
    return Cinv - W @ Q @ W.T, W @ Q, Q, beta, Cinv @ (y - H @ beta), Cinv, W


def cstar(X, model, P, G, Q, Xa, Xb):
    """c*(x, x') for the rows of Xa against the rows of Xb, numpy fp64: no clamp, no nugget"""
    order = (Q.shape[0] - 1) // X.shape[1]
    A, s = model["A"], np.asarray(model["s"], float)
    ka, kb = A * kmatrix(Xa, X, s), A * kmatrix(Xb, X, s)
    ha, hb = hmatrix(Xa, order), hmatrix(Xb, order)
    return A * kmatrix(Xa, Xb, s) - ka @ P @ kb.T + ha @ Q @ hb.T - ha @ G.T @ kb.T - ka @ G @ hb.T


def quadrature_post(X, model, P, G, Q, lo, hi, n=12):
    """the dict `post` returns first, by Gauss-Legendre quadrature of c* on ALL pairs of the n^d tensor nodes: no closed form"""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    d = len(lo)
    assert d <= 3
    t, wt = np.polynomial.legendre.leggauss(n)
    nodes = [lo[l] + (t + 1) * (hi[l] - lo[l]) / 2 for l in range(d)]
    mesh = np.stack([g.ravel() for g in np.meshgrid(*nodes, indexing="ij")], axis=1)
    Wt = wt / 2
    cs = cstar(X, model, P, G, Q, mesh, mesh).reshape((n,) * (2 * d))
    vals = []
    for inu in _subsets(d):
        f = cs
        for l in range(d - 1, -1, -1):                          # axes l (of x) and l + (axes of x left) (of x')
            k = f.ndim // 2
            if inu[l]:
                f = np.tensordot(np.diagonal(f, axis1=l, axis2=k + l), Wt, axes=([-1], [0]))
            else:
                f = np.tensordot(np.tensordot(f, Wt, axes=([k + l], [0])), Wt, axes=([l], [0]))
        vals.append(float(f))
    return _pack(np.array(vals), d)


def quadrature_band(X, model, P, G, Q, lo, hi, grid, n=24):
    """var[j][g] by quadrature of c* over the other coordinates of x and x' (d <= 2: the pairs of an n^(d-1) mesh)"""
    lo, hi, grid = np.asarray(lo, float), np.asarray(hi, float), np.asarray(grid, float)
    d = len(lo)
    assert d <= 2
    t, wt = np.polynomial.legendre.leggauss(n)
    out = np.empty(grid.shape)
    for j in range(d):
        for g, x in enumerate(grid[j]):
            if d == 1:
                out[j, g] = cstar(X, model, P, G, Q, np.array([[x]]), np.array([[x]]))[0, 0]
                continue
            o = 1 - j
            pts = np.empty((n, 2))
            pts[:, j] = x
            pts[:, o] = lo[o] + (t + 1) * (hi[o] - lo[o]) / 2
            out[j, g] = (wt / 2) @ cstar(X, model, P, G, Q, pts, pts) @ (wt / 2)
    return out


# ---------------------------------------------------------------------------------------------------- the other route to C^-1
def band_tables(X, model, order, lo, hi, grid):
    """-> (T [d x G x N], hm [d x G x nreg], cc [d]) of the band, numpy fp64"""
    X, lo, hi, grid = (np.asarray(v, float) for v in (X, lo, hi, grid))
    N, d = X.shape
    A, s = model["A"], np.asarray(model["s"], float)
    M = R.moments(R.NP, lo, hi)
    I = R.point_integrals(R.NP, X, s, lo, hi)[0]
    _, Pex = R.leave_one_out(I)
    UU = uu(R.NP, s, lo, hi)
    idx = basis_index(d, order)
    T = np.stack([A * np.exp(-s[j] * (grid[j][:, None] - X[None, :, j]) ** 2 / 2) * Pex[None, :, j] for j in range(d)])
    hm = np.stack([np.stack([np.ones_like(grid[j])] + [grid[j] ** p if l == j else np.full_like(grid[j], M[p][l]) for p, l in idx], axis=1)
                   for j in range(d)])
    return T, hm, np.array([A * np.prod(np.delete(UU, j)) for j in range(d)])


def chol_variance(X, order, A, s, nugget, T, hm, cc):
    """cc - |L^-1 T|^2 + r^T Q r, r = hm - W^T T, for the rows of T (M x N) and hm (M x nreg) from a Cholesky factor of
    C = A K + nugget I: the prediction's route, which never forms C^-1"""
    import scipy.linalg as sl
    C = A * kmatrix(X, X, s) + nugget * np.eye(len(X))
    H = hmatrix(X, order)
    L = np.linalg.cholesky(C)
    W = sl.cho_solve((L, True), H)
    Q = np.linalg.inv(H.T @ W)
    u = sl.solve_triangular(L, T.T, lower=True)
    r = hm - T @ W
    return cc - (u * u).sum(axis=0) + np.einsum("ma,ab,mb->m", r, Q, r)


def gauss_nodes(lo, hi, n=24):
    """-> (nodes, weights of the uniform density) on [lo, hi]"""
    t, wt = np.polynomial.legendre.leggauss(n)
    return lo + (t + 1) * (hi - lo) / 2, wt / 2


def scaled_errors(got, ref, scale, keys=KEYS):
    return R.scaled_errors(got, ref, scale, keys)


if __name__ == "__main__":
    import os
    import sys
    if "--measure" in sys.argv:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        import test_gpu_sens_post
        test_gpu_sens_post.measure()
