"""CPU reference for the gain over a weighted set of target points (gpemu_design_target_*, include/gpemu.h, DESIGN.md 4.23;
tests/test_gpu_design_target.py, tests/test_host_design_target.py, tests/test_designtargetref.py).  Test infrastructure only;
no device value enters unless a function says so.

  c*(x_s, x*) = c(x_s, x*) - k_s^T C^-1 k_* + r_s^T Q r_*,   r = h - W^T k,  W = C^-1 H,  Q = (H^T C^-1 H)^-1
  var(x*)     = c*(x*, x*) + nugget,    num(x*) = sum_s w_s c*(x_s, x*)^2,    gain = num / var  (0 where var <= 0)
  v(x_s)      = c*(x_s, x_s),           target_var = sum_s w_s v(x_s)

The conventions are the entry's, not predcovref's: the k-vectors are not clamped, and c(., .) and k carry no nugget wherever
the two points lie (kernel() below; tests/test_designtargetref.py pins it against the oracle's element off the nugget rule).
C and H are the oracle's matrices, the solves LAPACK's (cho_factor / cho_solve): the pattern of predcovref.float64_route.

Like predcovref.reference, reference() checks itself before it hands anything out: the linear algebra is repeated on numpy's
longdouble (vargradref.chol_ld / solve_ld; mpmath at 40 digits where longdouble is no wider than double) from the same matrix
elements, and the two must agree to PRECOND = 1e-10 of the scales the device bars are set on: kappa for c*, var and v,
kappa sum w for target_var, 2 kappa^2 sum w for num.

sweep() is the part the sweep kernel and the panel product compute, from given u, r and Q r rows (the device's own in the GPU
test): product, prior and reduction in the arithmetic of a dtype, with the scale its error is measured on,
  T_qs = |c| + sum_k |u_qk u_sk| + sum_a |r_qa (Q r)_sa|,   scale_q = sum_s w_s T_qs^2.

`python tests/designtargetref.py --measure` prints every figure a bar of the GPU file is derived from, over exactly its cases."""
import os
import sys

import numpy as np
import scipy.linalg as sl

if __name__ == "__main__":                       # (run as a script: the repository's root is not on the path yet)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import vargradref
from oracle import oracle as O

RTOL = vargradref.RTOL           # the bar of the device tests
PRECOND = vargradref.PRECOND     # float64 reference against the extended-precision one
LD = vargradref.LD
NUGGET = 1e-3

NS = [1, 63, 64, 65, 130]
DS = [1, 3, 8, 17]
ORDERS = [0, 1, 2, 3]
KINDS = [O.POWEREXP, O.MATERN32, O.MATERN52]
MS = [1, 63, 64, 65, 200]
REFIT_CASES = [(65, 2, 1, O.POWEREXP), (130, 3, 2, O.MATERN32), (64, 8, 0, O.MATERN52)]     # N, d, order, kind
QUAD_CASES = [(65, 1, 1, 32), (130, 2, 2, 16), (64, 2, 0, 16)]                               # N, d, order, nodes per coordinate
BIG = 16385


# ---------------------------------------------------------------------------------------------------- the model
def thetas(kind, d):
    """amplitude 1, nugget 1e-3 (C stays well conditioned), lengths that grow with d (test_gpu_sens_post.thetas); the Matern
    kernels take the first of them for every coordinate"""
    ln = [np.log(0.6 * max(1.0, np.sqrt(d / 3.0))) + 0.03 * l for l in range(d)]
    return np.array([0.0, np.log(NUGGET)] + ln) if kind == O.POWEREXP else np.array([1.0, NUGGET, ln[0]])


def amp_nugget(kind, th):
    return (float(np.exp(th[0])), float(np.exp(th[1]))) if kind == O.POWEREXP else (float(th[0]), float(th[1]))


def kappa(kind, th):
    return sum(amp_nugget(kind, th))


def kernel(kind, th, Xa, Xb, dtype=np.float64):
    """the bare kernel value between the rows of Xa and of Xb: no nugget, no clamp (emulator.c:101-152, :344-386, :438-480 with
    their literals for the square roots of 3 and 5)"""
    Xa, Xb, th = np.asarray(Xa).astype(dtype), np.asarray(Xb).astype(dtype), np.asarray(th).astype(dtype)
    D = Xa[:, None, :] - Xb[None, :, :]
    if kind == O.POWEREXP:
        return np.exp(th[0]) * np.exp(-((D / np.exp(th[2:])) ** 2).sum(axis=2) / 2)
    s = np.sqrt((D * D).sum(axis=2)) / np.exp(th[2])
    if kind == O.MATERN32:
        r3 = dtype(1.732050808)
        return th[0] * (1 + r3 * s) * np.exp(-r3 * s)
    r5 = dtype(2.236067978)
    return th[0] * (1 + r5 * s + (dtype(5.0) / dtype(3.0)) * s * s) * np.exp(-r5 * s)


def data(N, d):
    from madaiemulator_amd import synth
    if N == 1:                                   # (synth.design standardises y: one point has no spread)
        return synth.uniform(900 + d, (1, d)), np.array([0.7])
    X, y = synth.design(N, d, 900 + 31 * N + d)
    return X, y + 1.0


def box(X):
    lo, hi = X.min(axis=0), X.max(axis=0)
    if len(X) == 1:
        lo, hi = lo - 0.5, hi + 0.5
    return lo, hi


def points(X, n, seed):
    """n points of the design's range widened by a quarter on either side"""
    lo, hi = box(X)
    w = hi - lo
    return (lo - 0.25 * w) + 1.5 * w * np.random.default_rng(7000 + seed + 7 * len(X) + X.shape[1]).random((n, X.shape[1]))


def far_candidates(X, th, M, seed):
    """candidates at least a tenth of a length scale from every design point (test_gpu_design.far_candidates, either kind of thetas)"""
    ln = np.exp(th[2:])
    Xq = points(X, 8 * M, seed)
    dist = np.sqrt((((Xq[:, None, :] - X[None, :, :]) / ln) ** 2).sum(axis=2)).min(axis=1)
    Xq = Xq[dist >= 0.1][:M]
    assert len(Xq) == M
    return Xq


def targets_and_candidates(X, S, M, seed=0):
    """S targets with weights and M candidates: target 0 and candidate 0 lie on design points, the last candidate on the last
    target, the weights are uneven and one of them is 0 (where there are enough points for that)"""
    N = len(X)
    Xt, Xq = points(X, S, 11 + seed), points(X, M, 23 + seed)
    Xt[0] = X[0]
    Xq[0] = X[min(1, N - 1)]
    if M > 1:
        Xq[-1] = Xt[-1]
    w = 0.5 + np.random.default_rng(5 + S + seed).random(S)
    if S > 2:
        w[1] = 0.0
    return Xt, w / w.sum() * 1.5, Xq              # (a sum other than 1: the weights are used as given)


def shape_cases():
    """(N, d, order, kind, M, S): every N, d and order that fit; the kind, M and S rotate so that every value meets every
    other somewhere (tests/test_designtargetref.py checks that they do).  N = 1 has four cases for the five values of M and of
    S: a fifth one brings the missing 200"""
    out = []
    for iN, N in enumerate(NS):
        for iD, d in enumerate(DS):
            for o in ORDERS:
                if 1 + o * d <= N:
                    out.append((N, d, o, KINDS[(iD + o) % 3], MS[(iN + iD + o) % 5], MS[(iN + 2 * iD + 3 * o + 1) % 5]))
    return out + [(1, 3, 0, O.MATERN52, 200, 200)]


def case(N, d, o, kind, M, S, seed=0):
    X, y = data(N, d)
    Xt, w, Xq = targets_and_candidates(X, S, M, seed)
    return dict(name=f"N{N}-d{d}-o{o}-k{kind}-M{M}-S{S}" + (f"-seed{seed}" if seed else ""), N=N, d=d, order=o, kind=kind, X=X, y=y, th=thetas(kind, d), Xt=Xt, w=w, Xq=Xq)


def all_cases():
    """every case whose numbers tests/test_gpu_design_target.py compares with reference() and sweep()"""
    return [case(*c) for c in shape_cases()]


def big_cases():
    """the block edges: S = 16 385 and M = 16 385 at N = 65, d = 2"""
    return [case(65, 2, 1, O.MATERN52, 5, BIG, 1), case(65, 2, 1, O.POWEREXP, BIG, 7, 2)]


def refit_cases():
    out = []
    for N, d, o, kind in REFIT_CASES:
        c = case(N, d, o, kind, 3, 65, 3)
        c["Xq"] = far_candidates(c["X"], c["th"], 3, 3)
        c["name"] = "refit-" + c["name"]
        out.append(c)
    return out


def gauss_legendre_targets(lo, hi, n):
    """the tensor Gauss-Legendre rule with n nodes per coordinate on the box -> (Xt [n^d, d], weights of the uniform density)"""
    t, wt = np.polynomial.legendre.leggauss(n)
    axes = [lo[l] + (t + 1) * (hi[l] - lo[l]) / 2 for l in range(len(lo))]
    G = np.meshgrid(*axes, indexing="ij")
    Wm = np.meshgrid(*([wt / 2] * len(lo)), indexing="ij")
    return np.column_stack([g.ravel() for g in G]), np.prod([w.ravel() for w in Wm], axis=0)


def quad_cases():
    """power-exponential, d <= 2, the targets a Gauss-Legendre rule of the design's box: (case, lo, hi)"""
    out = []
    for N, d, o, n in QUAD_CASES:
        c = case(N, d, o, O.POWEREXP, 5, 1, 4)
        lo, hi = box(c["X"])
        c["Xt"], c["w"] = gauss_legendre_targets(lo, hi, n)
        c["Xq"] = far_candidates(c["X"], c["th"], 5, 4)
        c["name"] = f"quad-N{N}-d{d}-o{o}-n{n}"
        out.append((c, lo, hi))
    return out


# ---------------------------------------------------------------------------------------------------- the routes
def _assemble(kind, th, Xt, w, Xq, Kt, Kq, CiKt, CiKq, Rt, Rq, Q, dtype):
    amp, nug = amp_nugget(kind, th)
    w = np.asarray(w).astype(dtype)
    cstar = kernel(kind, th, Xq, Xt, dtype) - Kq @ CiKt + Rq @ Q @ Rt.T
    var = dtype(amp) - (Kq * CiKq.T).sum(axis=1) + ((Rq @ Q) * Rq).sum(axis=1) + dtype(nug)
    var_t = dtype(amp) - (Kt * CiKt.T).sum(axis=1) + ((Rt @ Q) * Rt).sum(axis=1)
    num = (w[None, :] * cstar * cstar).sum(axis=1)
    gain = np.where(var > 0, num / np.where(var > 0, var, 1), 0)
    return dict(cstar=cstar, var=var, var_t=var_t, num=num, gain=gain, target_var=(w * var_t).sum())


def float64_route(kind, order, X, th, Xt, w, Xq):
    """LAPACK in float64"""
    Cm, H = O.cov_matrix(kind, X, th), O.hmatrix(order, X)
    cf = sl.cho_factor(Cm, lower=True, check_finite=False)
    W = sl.cho_solve(cf, H, check_finite=False)
    Q = np.linalg.inv(H.T @ W)
    Kt, Kq = kernel(kind, th, Xt, X), kernel(kind, th, Xq, X)
    CiKt, CiKq = sl.cho_solve(cf, Kt.T, check_finite=False), sl.cho_solve(cf, Kq.T, check_finite=False)
    Rt, Rq = O.hmatrix(order, Xt) - Kt @ W, O.hmatrix(order, Xq) - Kq @ W
    return _assemble(kind, th, Xt, w, Xq, Kt, Kq, CiKt, CiKq, Rt, Rq, Q, np.float64)


def longdouble_route(kind, order, X, th, Xt, w, Xq):
    """the same on numpy's longdouble, Cholesky and solves written out (vargradref); the kernel values of the targets and
    candidates are made in longdouble too"""
    L = vargradref.chol_ld(O.cov_matrix(kind, X, th))
    H = O.hmatrix(order, X).astype(LD)
    Kt, Kq = kernel(kind, th, Xt, X, LD), kernel(kind, th, Xq, X, LD)
    nr, S = H.shape[1], len(Xt)
    Z = vargradref.solve_ld(L, np.column_stack([H, Kt.T, Kq.T]))
    W, CiKt, CiKq = Z[:, :nr], Z[:, nr:nr + S], Z[:, nr + S:]
    Q = vargradref.inv_spd_ld(H.T @ W)
    Rt, Rq = O.hmatrix(order, Xt).astype(LD) - Kt @ W, O.hmatrix(order, Xq).astype(LD) - Kq @ W
    return _assemble(kind, th, Xt, w, Xq, Kt, Kq, CiKt, CiKq, Rt, Rq, Q, LD)


def mpmath_route(kind, order, X, th, Xt, w, Xq, dps=40):
    """the extended route on mpmath (a platform without an extended longdouble; small cases) -> float64 arrays rounded once.
    The kernel values enter as float64 here: mpmath keeps the linear algebra exact to 40 digits, which is what PRECOND is about"""
    import mpmath as mp
    with mp.workdps(dps):
        tom = lambda A: mp.matrix(np.asarray(A, dtype=np.float64).tolist())
        tof = lambda A: np.array([[float(A[i, j]) for j in range(A.cols)] for i in range(A.rows)])
        Ci, H = tom(O.cov_matrix(kind, X, th)) ** -1, tom(O.hmatrix(order, X))
        Kt, Kq = tom(kernel(kind, th, Xt, X)), tom(kernel(kind, th, Xq, X))
        W = Ci * H
        Q = (H.T * W) ** -1
        Rt, Rq = tom(O.hmatrix(order, Xt)) - Kt * W, tom(O.hmatrix(order, Xq)) - Kq * W
        amp, nug = amp_nugget(kind, th)
        cstar = tof(tom(kernel(kind, th, Xq, Xt)) - Kq * Ci * Kt.T + Rq * Q * Rt.T)
        vq = tof(-Kq * Ci * Kq.T + Rq * Q * Rq.T).diagonal() + amp + nug
        vt = tof(-Kt * Ci * Kt.T + Rt * Q * Rt.T).diagonal() + amp
    w = np.asarray(w, dtype=np.float64)
    num = (w[None, :] * cstar * cstar).sum(axis=1)
    return dict(cstar=cstar, var=vq, var_t=vt, num=num, gain=np.where(vq > 0, num / np.where(vq > 0, vq, 1), 0), target_var=(w * vt).sum())


def extended_route(kind, order, X, th, Xt, w, Xq):
    return (longdouble_route if vargradref.LD_IS_EXTENDED else mpmath_route)(kind, order, X, th, Xt, w, Xq)


def scales(kind, th, w, var):
    """what each output is compared on: kappa for c*, var and var_t; kappa sum w for target_var; 2 kappa^2 sum w for num (c* on
    the scale kappa, squared and summed); that over var for gain"""
    kap, sw = kappa(kind, th), float(np.sum(w))
    var = np.asarray(var, dtype=np.float64)
    return dict(cstar=kap, var=kap, var_t=kap, target_var=kap * sw, num=2 * kap * kap * sw,
                gain=2 * kap * kap * sw / np.where(var > 0, var, np.inf))


def errors(got, ref, scale, keys=("var", "var_t", "target_var", "num", "gain")):
    """-> {key: max |got - ref| / scale}"""
    return {k: float(np.max(np.abs(np.asarray(got[k] - ref[k], dtype=np.float64)) / scale[k])) for k in keys}


def reference(c, rows=None):
    """the float64 route of a case, after asserting that it is good to PRECOND on these inputs; the measured figures come back
    as 'ref_err'.  rows: the candidates and targets whose part is repeated in extended precision (every element depends on its
    own two points only) -- all of them when None"""
    ref = float64_route(c["kind"], c["order"], c["X"], c["th"], c["Xt"], c["w"], c["Xq"])
    if rows is None:
        sub, ext = ref, extended_route(c["kind"], c["order"], c["X"], c["th"], c["Xt"], c["w"], c["Xq"])
    else:
        qs, ts = rows
        sub = float64_route(c["kind"], c["order"], c["X"], c["th"], c["Xt"][ts], c["w"][ts], c["Xq"][qs])
        ext = extended_route(c["kind"], c["order"], c["X"], c["th"], c["Xt"][ts], c["w"][ts], c["Xq"][qs])
    sc = scales(c["kind"], c["th"], c["w"] if rows is None else c["w"][rows[1]], sub["var"])
    e = errors(sub, ext, sc, ("cstar", "var", "var_t", "target_var", "num", "gain"))
    assert max(e.values()) <= PRECOND, ("ill-conditioned test inputs: reference errors", c["name"], e)
    ref["ref_err"] = e
    ref["scale"] = scales(c["kind"], c["th"], c["w"], ref["var"])
    return ref


def refit_target_var(c, x):
    """target_var of the design with x appended, the same thetas (float64 route)"""
    X2 = np.vstack([c["X"], np.asarray(x)[None, :]])
    return float64_route(c["kind"], c["order"], X2, c["th"], c["Xt"], c["w"], c["Xq"][:1])["target_var"]


def refit_gaps(c, ref=None):
    """|gain - (target_var - target_var')| per candidate over kappa sum w: the identity, N + 1 points refitted in numpy"""
    ref = ref or float64_route(c["kind"], c["order"], c["X"], c["th"], c["Xt"], c["w"], c["Xq"])
    sc = kappa(c["kind"], c["th"]) * float(np.sum(c["w"]))
    return np.array([abs(ref["gain"][q] - (ref["target_var"] - refit_target_var(c, x))) / sc for q, x in enumerate(c["Xq"])])


# ---------------------------------------------------------------------------------------------------- the sweep alone
def sweep(kind, th, Xq, Xt, w, Uq, Ut, Rq, QRt, dtype=LD):
    """num from given rows: P = U_q U_t^T, the prior c + r . (Q r), the weighted sum of squares, in dtype -> (num, scale)"""
    Uq, Ut, Rq, QRt, w = (np.asarray(a).astype(dtype) for a in (Uq, Ut, Rq, QRt, w))
    c = kernel(kind, th, Xq, Xt, dtype)
    cs = (c - Uq @ Ut.T) + Rq @ QRt.T
    T = np.abs(c) + np.abs(Uq) @ np.abs(Ut).T + np.abs(Rq) @ np.abs(QRt).T
    return (w[None, :] * cs * cs).sum(axis=1), np.asarray((w[None, :] * T * T).sum(axis=1), dtype=np.float64)


def rows_numpy(kind, order, X, th, P):
    """u = L^-1 k, r and Q r of the points P from a numpy fit (the device's own stand in for them in the GPU test)"""
    Cm, H = O.cov_matrix(kind, X, th), O.hmatrix(order, X)
    L = np.linalg.cholesky(Cm)
    K = kernel(kind, th, P, X)
    U = sl.solve_triangular(L, K.T, lower=True, check_finite=False).T
    W = sl.cho_solve((L, True), H, check_finite=False)
    Q = np.linalg.inv(H.T @ W)
    R = O.hmatrix(order, P) - K @ W
    return U, R, R @ Q.T


def sweep_error(c):
    """float64 against longdouble on the sweep's computation, on its scale"""
    Uq, Rq, _ = rows_numpy(c["kind"], c["order"], c["X"], c["th"], c["Xq"])
    Ut, _, QRt = rows_numpy(c["kind"], c["order"], c["X"], c["th"], c["Xt"])
    n64, sc = sweep(c["kind"], c["th"], c["Xq"], c["Xt"], c["w"], Uq, Ut, Rq, QRt, np.float64)
    nld, _ = sweep(c["kind"], c["th"], c["Xq"], c["Xt"], c["w"], Uq, Ut, Rq, QRt, LD)
    return float(np.max(np.abs(np.asarray(n64 - nld, dtype=np.float64)) / sc))


# ---------------------------------------------------------------------------------------------------- the closed form
def closed_form(c, lo, hi):
    """designref.gain for a power-exponential case and the uniform measure on the box, a and b from a numpy fit -> dict(num, gain)"""
    import designref as D
    import sensref as R
    th = c["th"]
    m = dict(A=float(np.exp(th[0])), s=np.exp(-2.0 * th[2:]))
    a, b, v, _ = D.fit_ab(c["X"], c["order"], m["A"], m["s"], float(np.exp(th[1])), c["Xq"])
    val, scale, _ = D.gain(R.NP, c["X"], m, lo, hi, None, c["Xq"], a, b, v)
    return dict(num=np.asarray(val["num"], dtype=np.float64), gain=np.asarray(val["gain"], dtype=np.float64), var=np.asarray(v),
                scale={k: np.asarray(scale[k], dtype=np.float64) for k in ("num", "gain")})


def quadrature_error(c, lo, hi):
    """the Gauss-Legendre sum of the float64 route against the closed form's integral, on the closed form's own scale (the sum
    of the absolute values of its six parts, designref.py: the parts cancel to 1e-8 of it, so relative to num itself the two
    float64 routes agree to 1e-8 only, however many nodes the rule has)"""
    ref = float64_route(c["kind"], c["order"], c["X"], c["th"], c["Xt"], c["w"], c["Xq"])
    cf = closed_form(c, lo, hi)
    return max(float(np.max(np.abs(ref[k] - cf[k]) / cf["scale"][k])) for k in ("num", "gain"))


def _measure_one(c):
    ref = reference(c)
    return c["name"], max(ref["ref_err"].values()), sweep_error(c)


def measure():
    import multiprocessing as mpc
    worst, worst_s = ("", 0.0), ("", 0.0)
    cases = all_cases()
    O.lib()                                      # (built once, before the workers start)
    with mpc.Pool(min(8, mpc.cpu_count())) as pool:
        for name, e, es in pool.imap_unordered(_measure_one, cases):
            print(f"{name}: float64 route against the extended one {e:.3e}, sweep float64 against longdouble {es:.3e}", flush=True)
            worst = max(worst, (name, e), key=lambda t: t[1])
            worst_s = max(worst_s, (name, es), key=lambda t: t[1])
    print(f"largest error of the float64 route over {len(cases)} cases: {worst[1]:.3e} ({worst[0]}; PRECOND {PRECOND:.0e})")
    print(f"largest float64-against-longdouble error of the sweep's computation: {worst_s[1]:.3e} ({worst_s[0]})")
    for c in big_cases():
        qs = np.arange(min(5, len(c["Xq"])))
        ts = np.arange(min(200, len(c["Xt"])))
        ref = reference(c, (qs, ts))
        print(f"{c['name']}: float64 route against the extended one on a part {max(ref['ref_err'].values()):.3e}")
    g = 0.0
    for c in refit_cases():
        gaps = refit_gaps(c)
        print(f"{c['name']}: refit gaps {gaps}")
        g = max(g, float(gaps.max()))
    print(f"largest refit gap in numpy: {g:.3e}")
    q = 0.0
    for c, lo, hi in quad_cases():
        e = quadrature_error(c, lo, hi)
        print(f"{c['name']}: quadrature error {e:.3e}")
        q = max(q, e)
    print(f"largest quadrature error: {q:.3e}")


if __name__ == "__main__":
    if "--measure" in sys.argv:
        measure()
