"""CPU reference for the expected reduction of the IMSE by one more run (gpemu_design_gain, include/gpemu.h).
Test infrastructure only; no device value enters except as an INPUT.

f is the posterior process of senspostref.py (no k-vector clamp, no nugget inside c).  Conditioning it on a run at x*, observed
with variance v = c*(x*, x*) + nugget, takes c*(x, x*) c*(x', x*) / v off its covariance, so the box average of its variance
(s_all of senspostref.post, the IMSE) drops by

  gain(x*) = num / v,   num = E_x[c*(x, x*)^2],   c*(x, x*) = c(x, x*) - k(x)^T a + h(x)^T b,   a = C^-1 k* + W Q r,  b = Q r.

The reference takes a, b and v as inputs (the device's own, or `fit_ab`'s from numpy) and assembles num as the RAW GRAM FORM

  num = z^T Gamma z,   z = [1, -a, b],   Gamma = E[phi phi^T],   phi(x) = [A k(x, x*), A k(x, x_1) .. A k(x, x_N), h(x)],

with Gamma's blocks from the pair integrals II (`pair`), the per-point integrals and the moments of sensref / sensmeasureref
under the measure `kind` (None: all uniform).  The device expands the same form into six parts and sums them another way:

  num = A^2 II(x*, x*) - 2 A^2 sum a_i w_i + 2 A sum b_al HK*_al + A^2 a^T K a - 2 A sum b_al (a^T HK_al) + b^T Hm b;

the SCALE of num is the sum of the absolute values of these six parts, that of gain the same divided by v.  Beside it the
reference returns the sum of the absolute values of the TERMS inside the parts (keys num_terms, gain_terms) --
  A^2 |II(x*, x*)| + 2 A^2 sum |a_i w_i| + 2 A sum |b_al HK*_al| + A^2 sum |a_i K_ii' a_i'| + 2 A sum |b_al a_i HK_al,i| + sum |b_al Hm b_be|
-- which is what bounds the rounding error of any fp64 evaluation (a holds entries of size 1 / nugget with alternating signs:
a^T K a is far smaller than its terms); tests/test_designref.py takes its own bars from it, the GPU tests use the scale.

Three backends as in senspostref.py: numpy fp64 (R.NP), mpmath at 50 digits (R.MP()), and `quadrature`: tensor Gauss-Legendre /
Gauss-Hermite quadrature of senspostref.cstar(...)^2, which uses no closed form.  `refit` is the identity itself: s_all of the
design minus s_all of the design with x* appended, both by senspostref.post on a numpy fit.

`python tests/designref.py --measure` prints, over exactly the cases of tests/test_gpu_design.py, the largest scaled error of the
numpy backend against mpmath, the largest refit gap and the discrepancy of the two routes to a and b in numpy; the figures it
printed are written down in that file."""
import numpy as np

import sensref as R
import senspostref as SP
import sensmeasureref as SM


def _kind(kind, d):
    return np.zeros(d, dtype=int) if kind is None else np.asarray(kind, dtype=int).ravel()


def _prod(F):
    """product over the last axis (prefix products: no division, exact zeros stay zeros)"""
    return R.leave_one_out(F)[0]


# ---------------------------------------------------------------------------------------------------- pieces
def pair(B, xa, xb, s, lo, hi, kind):
    """II_l of the points xa, xb (arrays that broadcast, last axis d), one context (s = t):
       uniform:  exp(-(s / 2) (a - b)^2 / 2) sqrt(pi / 4 s) / w [erf(sqrt(s) (hi - c)) - erf(sqrt(s) (lo - c))],  c = (a + b) / 2
       Gaussian: (1 + 2 s v)^-1/2 exp(-[s^2 v (a - b)^2 + s (a - mu)^2 + s (b - mu)^2] / (2 (1 + 2 s v)))"""
    kind = _kind(kind, len(s))
    xa, xb = np.broadcast_arrays(xa, xb)
    out = np.empty(xa.shape, dtype=xa.dtype)
    u, g = np.flatnonzero(kind == SM.UNIFORM), np.flatnonzero(kind == SM.GAUSS)
    if len(u):
        a, b, su, l_, h_ = xa[..., u], xb[..., u], s[u], lo[u], hi[u]
        c, al = (a + b) / 2, B.sqrt(su)
        out[..., u] = B.exp(-(su / 2) * (a - b) ** 2 / 2) * (B.sqrt(B.pi / (4 * su)) / (h_ - l_)) * B.derf(al * (l_ - c), al * (h_ - c))
    if len(g):
        a, b, sg, mu, v = xa[..., g], xb[..., g], s[g], lo[g], hi[g] * hi[g]
        D2 = 1 + 2 * sg * v
        out[..., g] = B.exp(-(sg * sg * v * (a - b) ** 2 + sg * (a - mu) ** 2 + sg * (b - mu) ** 2) / (2 * D2)) / B.sqrt(D2)
    return out


def basis_tables(B, X, s, lo, hi, kind, order):
    """-> HK [nreg, n]: E[h_al(x) prod_l k_l(X_il, x_l)] for the rows of X (no amplitude)"""
    d = X.shape[1]
    with SM.measure(_kind(kind, d)):
        IJ = R.point_integrals(B, X, s, lo, hi)
    PI, Pex = R.leave_one_out(IJ[0])
    return np.stack([PI] + [IJ[p][:, l] * Pex[:, l] for p, l in SP.basis_index(d, order)])


def basis_moments(B, lo, hi, kind, order):
    """-> Hm [nreg, nreg] = E[h h^T]"""
    d = len(lo)
    with SM.measure(_kind(kind, d)):
        M = R.moments(B, lo, hi)
    idx = SP.basis_index(d, order)
    Eh = np.array([lo[0] * 0 + 1] + [M[p][l] for p, l in idx], dtype=object if isinstance(B, R.MP) else float)
    Hm = Eh[:, None] * Eh[None, :]
    for a, (p, l) in enumerate(idx, start=1):
        for b, (q, m) in enumerate(idx, start=1):
            if m == l:
                Hm[a, b] = M[p + q][l]
    return Hm


def design_tables(B, X, model, lo, hi, kind, order):
    """what depends on the design alone: (K [N, N], HK [nreg, N], Hm [nreg, nreg]) in the backend's numbers"""
    X, lo, hi, s = B.arr(X), B.arr(lo), B.arr(hi), B.arr(model["s"])
    K = _prod(pair(B, X[:, None, :], X[None, :, :], s, lo, hi, kind))
    return K, basis_tables(B, X, s, lo, hi, kind, order), basis_moments(B, lo, hi, kind, order)


def gain(B, X, model, lo, hi, kind, Xq, a, b, v, tables=None):
    """-> (dict(num [M], gain [M]), the same keys with the scales and num_terms, gain_terms, parts [M, 6]) as float arrays; a [M, N], b [M, nreg], v [M]"""
    order = (np.shape(b)[1] - 1) // np.shape(X)[1]
    K, HK, Hm = tables if tables is not None else design_tables(B, X, model, lo, hi, kind, order)
    X, Xq, lo, hi, s = B.arr(X), B.arr(Xq), B.arr(lo), B.arr(hi), B.arr(model["s"])
    a, b, v, A = B.arr(a), B.arr(b), B.arr(v), B.arr(model["A"])[()]
    w = _prod(pair(B, Xq[:, None, :], X[None, :, :], s, lo, hi, kind))          # [M, N]
    self_ = _prod(pair(B, Xq, Xq, s, lo, hi, kind))                             # [M]
    HKs = basis_tables(B, Xq, s, lo, hi, kind, order)                           # [nreg, M]
    # the Gram matrix of [A k(., x_i), h] and, per candidate, its border for A k(., x*)
    Grr = np.block([[A * A * K, A * HK.T], [A * HK, Hm]])
    G0 = np.concatenate([A * A * w, A * HKs.T], axis=1)
    Z = np.concatenate([-a, b], axis=1)
    num = A * A * self_ + 2 * (G0 * Z).sum(axis=1) + (np.dot(Z, Grr) * Z).sum(axis=1)
    parts = np.stack([A * A * self_, -2 * A * A * (a * w).sum(axis=1), 2 * A * (b * HKs.T).sum(axis=1),
                      A * A * (np.dot(a, K) * a).sum(axis=1), -2 * A * (np.dot(a, HK.T) * b).sum(axis=1), (np.dot(b, Hm) * b).sum(axis=1)],
                     axis=1)
    af, bf, Af = np.abs(B.tofloat(a)), np.abs(B.tofloat(b)), float(A)
    Kf, HKf, Hmf, wf, HKsf = (np.abs(B.tofloat(x)) for x in (K, HK, Hm, w, HKs))
    terms = (Af * Af * np.abs(B.tofloat(self_)) + 2 * Af * Af * (af * wf).sum(axis=1) + 2 * Af * (bf * HKsf.T).sum(axis=1)
             + Af * Af * ((af @ Kf) * af).sum(axis=1) + 2 * Af * ((af @ HKf.T) * bf).sum(axis=1) + ((bf @ Hmf) * bf).sum(axis=1))
    num, parts, v = B.tofloat(num), B.tofloat(parts), B.tofloat(v)
    scale = np.abs(parts).sum(axis=1)
    ok = v > 0
    vs = np.where(ok, v, 1.0)
    g = np.where(ok, num / vs, 0.0)
    return dict(num=num, gain=g), dict(num=scale, gain=scale / vs, num_terms=terms, gain_terms=terms / vs), parts


KEYS = ("num", "gain")


def scaled_errors(got, ref, scale, keys=KEYS):
    return R.scaled_errors(got, ref, scale, keys)


# ---------------------------------------------------------------------------------------------------- a, b, v in numpy
def fit_ab(X, order, A, s, nugget, Xq, cinv=None):
    """-> (a [M, N], b [M, nreg], v [M], (P, G, Q)) with C^-1 by numpy's inverse (or `cinv`, e.g. the device's)"""
    X, Xq = np.asarray(X, float), np.asarray(Xq, float)
    if cinv is None:
        cinv = SP.fit_state(X, np.zeros(len(X)), order, A, s, nugget)[5]
    W = cinv @ SP.hmatrix(X, order)
    Q = np.linalg.inv(SP.hmatrix(X, order).T @ W)
    Q = (Q + Q.T) / 2
    k, h = A * SP.kmatrix(Xq, X, s), SP.hmatrix(Xq, order)
    r = h - k @ W
    b = r @ Q
    a = k @ cinv + b @ W.T
    v = A - np.einsum("mi,ij,mj->m", k, cinv, k) + np.einsum("ma,ma->m", r, b) + nugget
    return a, b, v, (cinv - W @ Q @ W.T, W @ Q, Q)


def ab_scales(X, order, A, s, Xq, cinv):
    """the scales a and b are compared on: sum_j |C^-1_ij k_j| + sum_al |W_i,al b_al| and sum_be |Q_al,be| (|h_be| + sum_i |W_i,be k_i|)"""
    W = cinv @ SP.hmatrix(X, order)
    Q = np.linalg.inv(SP.hmatrix(X, order).T @ W)
    k, h = A * SP.kmatrix(Xq, X, s), SP.hmatrix(Xq, order)
    rs = np.abs(h) + np.abs(k) @ np.abs(W)
    bs = rs @ np.abs(Q)
    return np.abs(k) @ np.abs(cinv) + bs @ np.abs(W).T, bs


def chol_ab(X, order, A, s, nugget, Xq):
    """a, b and v by the prediction's route, which never forms C^-1: u = L^-1 k, a = L^-T u + W b"""
    import scipy.linalg as sl
    X, Xq = np.asarray(X, float), np.asarray(Xq, float)
    C = A * SP.kmatrix(X, X, s) + nugget * np.eye(len(X))
    H = SP.hmatrix(X, order)
    L = np.linalg.cholesky(C)
    W = sl.cho_solve((L, True), H)
    Q = np.linalg.inv(H.T @ W)
    k, h = A * SP.kmatrix(Xq, X, s), SP.hmatrix(Xq, order)
    u = sl.solve_triangular(L, k.T, lower=True)
    r = h - k @ W
    b = r @ Q
    a = sl.solve_triangular(L.T, u, lower=False).T + b @ W.T
    return a, b, A - (u * u).sum(axis=0) + np.einsum("ma,ma->m", r, b) + nugget


# ---------------------------------------------------------------------------------------------------- no closed form
def quadrature(X, model, order, nugget, lo, hi, kind, Xq, n=24):
    """num by tensor quadrature of cstar(x, x*)^2 over the measure (d <= 3), P, G, Q from a numpy fit"""
    X, Xq = np.asarray(X, float), np.asarray(Xq, float)
    d = X.shape[1]
    assert d <= 3
    P, G, Q = SP.fit_state(X, np.zeros(len(X)), order, model["A"], model["s"], nugget)[:3]
    nw = SM.nodes_weights(_kind(kind, d), lo, hi, n)
    mesh = np.stack([g.ravel() for g in np.meshgrid(*[t for t, _ in nw], indexing="ij")], axis=1)
    wt = nw[0][1]
    for _, w in nw[1:]:
        wt = np.multiply.outer(wt, w)
    cs = SP.cstar(X, model, P, G, Q, mesh, Xq)
    return wt.ravel() @ (cs * cs)


def refit(X, model, order, nugget, lo, hi, kind, Xq):
    """-> (s_all - s_all' per candidate, the sum of the two values' scales): the identity itself, N + 1 points refitted per candidate"""
    X, Xq = np.asarray(X, float), np.asarray(Xq, float)
    kind = _kind(kind, X.shape[1])

    def s_all(Z):
        P, G, Q = SP.fit_state(Z, np.zeros(len(Z)), order, model["A"], model["s"], nugget)[:3]
        val, scale = SM.post(kind, R.NP, Z, model, P, G, Q, np.asarray(lo, float), np.asarray(hi, float))
        return float(val["s_all"]), float(scale["s_all"])

    v0, s0 = s_all(X)
    out = [s_all(np.vstack([X, x[None, :]])) for x in Xq]
    return np.array([v0 - v for v, _ in out]), np.array([s0 + s for _, s in out])


if __name__ == "__main__":
    import os
    import sys
    if "--measure" in sys.argv:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        import test_gpu_design
        test_gpu_design.measure()
