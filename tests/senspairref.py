"""CPU references for the second-order sensitivity analysis (gpemu_sens_pairs / gpemu_sens_pairs_post / gpemu_sens_joint,
include/gpemu.h), built on sensref.py and senspostref.py, which it imports and does not change.  Test
infrastructure only; no device value enters except as an INPUT.

For u = {j, k}, j < k, numbered p(j, k) = j (2 d - j - 1) / 2 + (k - j - 1):

  `pair_covariances`  cov_pair[p] = Cov(E[m^a | x_j, x_k], E[m^b | x_j, x_k]): the `assemble(inu, kk)` rule of
                      sensref.covariances with  KK_jk = sum_ii' gamma_i gamma'_i' II_j II_k Pex2_jk(i) Pex2'_jk(i'),
                      Pex2_jk(i) = prod_{l != j,k} I_l(i),
  `pair_post`         s_pair[p] = S_u of senspostref.post,
  `joint_surface`     joint = E[m | x_j, x_k] at given points and the interaction effect inter = joint - main_j - main_k + E0
                      = A sum_i gamma_i [k_j k_k Pex2_jk - k_j Pex_j - k_k Pex_k + prod_l I_l](i) (the polynomial parts cancel),

each with the NP or the MP backend of sensref.py, returning values and SCALES as sensref.covariances does (the sum of the
absolute values of the parts a value is made of), and the counterparts by tensor Gauss-Legendre quadrature, which use no
closed form: `quadrature_pairs` and `quadrature_joint` for d <= 4, `quadrature_pair_post` for d <= 3 (all pairs of nodes).

`python tests/senspairref.py --measure` prints the largest scaled errors of the NP backend against the MP backend over the
cases of tests/test_gpu_sens_pairs.py; the figures it printed are written down in that file."""
import numpy as np

import sensref as R
import senspostref as SP


def pairs(d):
    return [(j, k) for j in range(d) for k in range(j + 1, d)]


def pair_index(j, k, d):
    return j * (2 * d - j - 1) // 2 + (k - j - 1)


def leave_two_out(F):
    """F[..., l] -> G[..., p(j, k)] = prod over l != j, k, by plain products (no division)"""
    d = F.shape[-1]
    out = []
    for j, k in pairs(d):
        run = F[..., 0] * 0 + 1
        for l in range(d):
            if l != j and l != k:
                run = run * F[..., l]
        out.append(run)
    return np.stack(out, axis=-1)


# ---------------------------------------------------------------------------------------------------- closed forms
def pair_covariances(B, X, ma, mb, lo, hi):
    """-> (dict(cov_pair [npairs]), dict(cov_pair: the scales)), float arrays"""
    X, lo, hi = B.arr(X), B.arr(lo), B.arr(hi)
    N, d = X.shape
    M = R.moments(B, lo, hi)
    a, b = R._Side(B, X, ma, lo, hi, M), R._Side(B, X, mb, lo, hi, M)
    EQQ = lo * 0                                                # E[q^a_l q^b_l]
    for p, ca in enumerate(a.c):
        for q, cb in enumerate(b.c):
            EQQ = EQQ + ca * cb * M[p + q + 2]
    Hab, Hba = R._poly_kernel(B, a, b), R._poly_kernel(B, b, a)
    II = R.pair_integrals(B, X, a.s, b.s, lo, hi)               # N x N x d
    Pa, Pb = leave_two_out(a.IJ[0]), leave_two_out(b.IJ[0])     # N x npairs
    gg = a.gamma[:, None] * b.gamma[None, :]
    AA = a.A * b.A
    e00 = a.E0 * b.E0
    val, scl = [], []
    for p, (j, k) in enumerate(pairs(d)):
        kk = AA * (gg * II[:, :, j] * II[:, :, k] * Pa[:, None, p] * Pb[None, :, p]).sum()
        # sensref.covariances' assemble(inu, kk) with u = {j, k}
        ua, ub = a.Eq[j] + a.Eq[k], b.Eq[j] + b.Eq[k]
        ca, cb = a.S - ua, b.S - ub
        pp = ca * cb + ca * ub + cb * ua + ua * ub
        pk = ca * b.F + cb * a.F
        for l in (j, k):
            pp = pp + EQQ[l] - a.Eq[l] * b.Eq[l]
            pk = pk + Hab[l] + Hba[l]
        val.append(pp + pk + kk - e00)
        scl.append(R._abs(pp) + R._abs(pk) + R._abs(kk) + R._abs(e00))
    return dict(cov_pair=B.tofloat(val)), dict(cov_pair=B.tofloat(scl))


def pair_post(B, X, model, P, G, Q, lo, hi):
    """-> (dict(s_pair [npairs]), scales): senspostref.post's S_u for u = {j, k}"""
    X, lo, hi = B.arr(X), B.arr(lo), B.arr(hi)
    P, G, Q = B.arr(P), B.arr(G), B.arr(Q)
    N, d = X.shape
    nreg = Q.shape[0]
    order = (nreg - 1) // d
    A, s = B.arr(model["A"])[()], B.arr(model["s"])
    M = R.moments(B, lo, hi)
    IJ = R.point_integrals(B, X, s, lo, hi)
    PI, Pex = R.leave_one_out(IJ[0])
    Pex2 = leave_two_out(IJ[0])
    II = R.pair_integrals(B, X, s, s, lo, hi)
    UU = SP.uu(B, s, lo, hi)
    idx = SP.basis_index(d, order)
    Eh = np.array([lo[0] * 0 + 1] + [M[p][l] for p, l in idx], dtype=object if isinstance(B, R.MP) else float)
    Hm0 = Eh[:, None] * Eh[None, :]
    HK0 = Eh[:, None] * (A * PI)[None, :]                       # nreg x N
    vals, scls = [], []
    for pn, (j, k) in enumerate(pairs(d)):
        cc = A + lo[0] * 0
        for l in range(d):
            if l != j and l != k:
                cc = cc * UU[l]
        KK = II[:, :, j] * II[:, :, k] * Pex2[:, None, pn] * Pex2[None, :, pn]
        Hm, HK = Hm0.copy(), HK0.copy()
        for l in (j, k):                                        # basis function (p, l) is number 1 + (p - 1) d + l
            for p in range(1, order + 1):
                a = 1 + (p - 1) * d + l
                HK[a] = A * IJ[p][:, l] * Pex[:, l]
                for q in range(1, order + 1):
                    Hm[a, 1 + (q - 1) * d + l] = M[p + q][l]
        kk, hq, hk = A * A * P * KK, Q * Hm, 2 * G * HK.T
        vals.append(cc - kk.sum() + hq.sum() - hk.sum())
        scls.append(abs(cc) + SP._asum(kk) + SP._asum(hq) + SP._asum(hk))
    return dict(s_pair=B.tofloat(vals)), dict(s_pair=B.tofloat(scls))


def joint_surface(B, X, model, lo, hi, j, k, xj, xk):
    """-> (dict(e0, joint [G], inter [G]), scales) at the points (x_j, x_k) = (xj[g], xk[g]), j < k"""
    assert j < k
    X, lo, hi, xj, xk = B.arr(X), B.arr(lo), B.arr(hi), B.arr(xj), B.arr(xk)
    N, d = X.shape
    a = R._Side(B, X, model, lo, hi, R.moments(B, lo, hi))
    Pex2 = leave_two_out(a.IJ[0])[:, pair_index(j, k, d)]
    kj = B.exp(-a.s[j] * (xj[None, :] - X[:, j, None]) ** 2 / 2)        # N x G
    kk = B.exp(-a.s[k] * (xk[None, :] - X[:, k, None]) ** 2 / 2)
    g = a.gamma[:, None]
    t1 = a.A * (g * kj * kk * Pex2[:, None]).sum(axis=0)
    t2 = a.A * (g * kj * a.Pex[:, j, None]).sum(axis=0)
    t3 = a.A * (g * kk * a.Pex[:, k, None]).sum(axis=0)
    q = xj * 0
    for p, cp in enumerate(a.c):
        q = q + cp[j] * xj ** (p + 1) + cp[k] * xk ** (p + 1)
    const = a.S - a.Eq[j] - a.Eq[k]
    inter = a.A * (g * (((kj * kk * Pex2[:, None] - kj * a.Pex[:, j, None]) - kk * a.Pex[:, k, None]) + a.P[:, None])).sum(axis=0)
    val = dict(e0=a.E0, joint=const + q + t1, inter=inter)
    scl = dict(e0=R._abs(a.S) + R._abs(a.F), joint=R._abs(const) + abs(q) + abs(t1), inter=abs(t1) + abs(t2) + abs(t3) + R._abs(a.F))
    return {n: B.tofloat(v) for n, v in val.items()}, {n: B.tofloat(v) for n, v in scl.items()}


# ---------------------------------------------------------------------------------------------------- quadrature
def _mesh(lo, hi, n):
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    d = len(lo)
    t, wt = np.polynomial.legendre.leggauss(n)
    nodes = [lo[l] + (t + 1) * (hi[l] - lo[l]) / 2 for l in range(d)]
    return nodes, np.stack([g.ravel() for g in np.meshgrid(*nodes, indexing="ij")], axis=1), wt / 2


def quadrature_pairs(X, ma, mb, lo, hi, n=20):
    """cov_pair by tensor Gauss-Legendre quadrature of m itself and of its conditional means given (x_j, x_k): d <= 4"""
    d = len(lo)
    assert 2 <= d <= 4
    _, mesh, W = _mesh(lo, hi, n)
    fa = R.mean_function(X, ma, mesh).reshape((n,) * d)
    fb = fa if mb is ma else R.mean_function(X, mb, mesh).reshape((n,) * d)

    def cond(f, keep):
        for l in range(d - 1, -1, -1):
            if l not in keep:
                f = np.tensordot(f, W, axes=([l], [0]))
        return f

    e0a, e0b = float(cond(fa, ())), float(cond(fb, ()))
    return dict(cov_pair=np.array([W @ ((cond(fa, u) - e0a) * (cond(fb, u) - e0b)) @ W for u in pairs(d)]))


def quadrature_joint(X, model, lo, hi, j, k, xj, xk, n=20):
    """dict(e0, joint, inter) by quadrature of m over the other coordinates; inter as joint - main_j - main_k + E0: d <= 4"""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    d = len(lo)
    assert 2 <= d <= 4

    def average(fixed):
        """E[m | x_l = v for (l, v) in fixed]"""
        free = [l for l in range(d) if l not in fixed]
        if not free:
            return float(R.mean_function(X, model, np.array([[fixed[l] for l in range(d)]]))[0])
        _, sub, W = _mesh(lo[free], hi[free], n)
        pts = np.empty((len(sub), d))
        pts[:, free] = sub
        for l, v in fixed.items():
            pts[:, l] = v
        f = R.mean_function(X, model, pts).reshape((n,) * len(free))
        for _ in free:
            f = np.tensordot(f, W, axes=([0], [0]))
        return float(f)

    e0 = average({})
    joint = np.array([average({j: a, k: b}) for a, b in zip(xj, xk)])
    inter = np.array([jt - average({j: a}) - average({k: b}) + e0 for jt, a, b in zip(joint, xj, xk)])
    return dict(e0=np.array(e0), joint=joint, inter=inter)


def quadrature_pair_post(X, model, P, G, Q, lo, hi, n=12):
    """s_pair by Gauss-Legendre quadrature of c* on ALL pairs of the n^d tensor nodes (senspostref.quadrature_post's way): d <= 3"""
    d = len(lo)
    assert 2 <= d <= 3
    _, mesh, Wt = _mesh(lo, hi, n)
    cs = SP.cstar(X, model, P, G, Q, mesh, mesh).reshape((n,) * (2 * d))
    vals = []
    for u in pairs(d):
        f = cs
        for l in range(d - 1, -1, -1):                          # axes l (of x) and l + (axes of x left) (of x')
            h = f.ndim // 2
            if l in u:
                f = np.tensordot(np.diagonal(f, axis1=l, axis2=h + l), Wt, axes=([-1], [0]))
            else:
                f = np.tensordot(np.tensordot(f, Wt, axes=([h + l], [0])), Wt, axes=([l], [0]))
        vals.append(float(f))
    return dict(s_pair=np.array(vals))


def scaled_errors(got, ref, scale, keys):
    return R.scaled_errors(got, ref, scale, keys)


if __name__ == "__main__":
    import os
    import sys
    if "--measure" in sys.argv:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        import test_gpu_sens_pairs
        test_gpu_sens_pairs.measure_np_against_mp()
