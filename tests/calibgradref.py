"""References for the gradient of the calibration statistics (gpemu_calib_grad), built on calibref's cases:
the DIRECT nt x nt form, never the r-form the library evaluates.  With C = S + A D A^T = L L^T, W = L^-1 [A | z - y]:

    u = -A^T C^-1 (z - y) = -W_A^T w,     tau_c = (A^T C^-1 A)_cc = |column c of W_A|^2
    d chi2 / dx_j   =   2 sum_c u_c dm_c/dx_j  -      sum_c u_c^2 dv_c/dx_j
    d logpdf / dx_j =   - sum_c u_c dm_c/dx_j  +  1/2 sum_c (u_c^2 - tau_c) dv_c/dx_j

(a variance below 0 counts as 0 and its dv_c has weight 0: the derivative of the function the evaluation computes).

  direct64   float64 (numpy / LAPACK): X = C^-1 [A | z - y] through the Cholesky factor, then two steps of iterative
             refinement in float64 with the residual taken against S, A and v themselves, never against the rounded C.  Without
             them the solve's error grows with cond(C) (2e4 at point 902 of r8_nt130: 1.7e-13 against 50 digits there, 30 x
             what the points below show), which u and tau pass on undamped -- chi2, a quadratic form, does not; with them
             direct64 is as good at every point as at the sampled ones and the bars below describe it
  direct_mp  the same at 50 digits (mpmath, forward solves W = L^-1 [A | z - y]: u = -W_A^T w, tau_c = |column c of W_A|^2)
  rform64    the r x r form in numpy on a projection (m_hat, Sigma_z): u = T^-1 (m - m_hat), tau = diag T^-1
  stat_mp    chi2 and logpdf at 50 digits WITHOUT the final rounding, from 50-digit m and v: what a central difference with a
             step of 1e-15 needs (calibref.direct_mp rounds its inputs and outputs to float64; test_calibgradref.py asserts
             that the two agree where both apply)

Gradient inputs per case, seeded: gmean ~ N(0, 1), gvar = var * N(0, 1), component c's M x d row-major block at c * ldg with
ldg = M * d + pad, the padding filled with 1e300; d from {1, 3, 8, 17}, spread over the cases by their index.

Error measure per (q, j): |got - ref| / max(1, sum |terms|), the reference's own sum of the absolute values of the 2 nr
summands: the sum over the components cancels.

BARS, per statistic (gchi2, glogpdf): 8 x MEASURED, the largest error of direct64 against direct_mp over the points
calibref.mp_points takes of every family of calibref.CASES and calibref.SPECIALS (v_huge apart, as in calibref: float64 cannot
factor C at v = 1e30; that family is compared with direct_mp alone), rounded up to one digit.  Measured on the CPU before a
device ran:
    gchi2 5.5e-15   glogpdf 4.4e-15
(test_calibgradref.py recomputes them and asserts that neither exceeds MEASURED).  The r-form in float64 on
gpemu_calib_project's tables (rform64) is within 3.9e-15 and 3.9e-15 of direct_mp on the same points.
"""
import zlib

import numpy as np

import calibref as R

STATS = ("gchi2", "glogpdf")
MEASURED = np.array([6e-15, 5e-15])
BARS = 8.0 * MEASURED
DIMS = (1, 3, 8, 17)
GPAD = 5


def dim_of(name):
    names = [a[0] for a in R.CASES] + ["special_" + k for k in R.SPECIALS]
    return DIMS[names.index(name) % len(DIMS)]


def add_gradients(c, d=None):
    """c (a calibref case) gains d, ldg and gmean, gvar of shape (nr, ldg); returns c"""
    d = dim_of(c["name"]) if d is None else d
    nr, M = c["nr"], c["M"]
    rng = np.random.default_rng(zlib.crc32((c["name"] + "/grad").encode()))
    ldg = M * d + GPAD
    gmean = np.full((nr, ldg), 1e300)                    # the padding must never reach a result
    gvar = np.full((nr, ldg), 1e300)
    gmean[:, :M * d] = rng.standard_normal((nr, M * d))
    gvar[:, :M * d] = np.repeat(c["var"][:, :M], d, axis=1) * rng.standard_normal((nr, M * d))
    c.update(d=d, ldg=ldg, gmean=gmean, gvar=gvar)
    return c


def make(name):
    """the calibref case or special of that name, with its gradient inputs"""
    c = R.make_special(name[8:]) if name.startswith("special_") else R.make_case(*next(a for a in R.CASES if a[0] == name))
    return add_gradients(c)


def all_cases():
    return [add_gradients(c) for c in R.all_cases()]


def _blocks(c):
    nr, M, d = c["nr"], c["M"], c["d"]
    return c["gmean"][:, :M * d].reshape(nr, M, d), c["gvar"][:, :M * d].reshape(nr, M, d)


def _combine(u, tau, live, gm, gv):
    """u, tau, live: (nr,) for one point; gm, gv: (nr, d) -> gchi2, glogpdf, and the two sums of |terms|, each (d,); the sums
    over c in index order from 0.0"""
    d = gm.shape[1]
    gc, gl, sc, sl = np.zeros(d), np.zeros(d), np.zeros(d), np.zeros(d)
    for k in range(len(u)):
        t1 = u[k] * gm[k]
        gc += 2.0 * t1
        sc += np.abs(2.0 * t1)
        gl -= t1
        sl += np.abs(t1)
    for k in range(len(u)):
        if not live[k]:
            continue
        t2, t3 = (u[k] * u[k]) * gv[k], 0.5 * (u[k] * u[k] - tau[k]) * gv[k]
        gc -= t2
        sc += np.abs(t2)
        gl += t3
        sl += np.abs(t3)
    return gc, gl, sc, sl


def direct64(c):
    """-> g[2, M, d] (gchi2, glogpdf) and scale[2, M, d] (the sums of |terms|), float64, direct form; NaN where a point's
    means or variances are not finite or C cannot be factored"""
    import scipy.linalg
    nr, M, d = c["nr"], c["M"], c["d"]
    A, S = c["A"], R._smat(c)
    gm, gv = _blocks(c)
    g = np.full((2, M, d), np.nan)
    scale = np.full((2, M, d), np.nan)
    for q in range(M):
        m, v0 = c["mean"][:, q], c["var"][:, q]
        if not (np.all(np.isfinite(m)) and np.all(np.isfinite(v0))):
            continue
        live = ~(v0 < 0.0)
        v = np.where(live, v0, 0.0)
        try:
            L = np.linalg.cholesky(S + (A * v[None, :]) @ A.T)
        except np.linalg.LinAlgError:
            continue
        B = np.column_stack([A, c["z"] - (c["ybar"] + A @ m)])
        X = scipy.linalg.cho_solve((L, True), B)
        for _ in range(2):                               # refinement against S, A and v themselves (see the module's docstring)
            X = X + scipy.linalg.cho_solve((L, True), B - (S @ X + A @ (v[:, None] * (A.T @ X))))
        u = -(A.T @ X[:, nr])
        tau = np.einsum("tc,tc->c", A, X[:, :nr])
        g[0, q], g[1, q], scale[0, q], scale[1, q] = _combine(u, tau, live, gm[:, q], gv[:, q])
    return g, scale


def rform64(c, proj):
    """the r x r form on a projection (dict with mhat, sigz) -> g[2, M, d]"""
    nr, M, d = c["nr"], c["M"], c["d"]
    gm, gv = _blocks(c)
    g = np.full((2, M, d), np.nan)
    for q in range(M):
        m, v0 = c["mean"][:, q], c["var"][:, q]
        if not (np.all(np.isfinite(m)) and np.all(np.isfinite(v0))):
            continue
        live = ~(v0 < 0.0)
        Ti = np.linalg.inv(proj["sigz"] + np.diag(np.where(live, v0, 0.0)))
        g[0, q], g[1, q], _, _ = _combine(Ti @ (m - proj["mhat"]), np.diag(Ti).copy(), live, gm[:, q], gv[:, q])
    return g


def _mp_tables(c):
    import mpmath as mp
    mp.mp.dps = 50
    f = mp.mpf
    nt = c["nt"]
    A = [[f(float(x)) for x in row] for row in c["A"]]
    S = [[f(float(x)) for x in row] for row in R._smat(c)]
    if c["S"] is None:                                   # the diagonal form squares sd in extended precision, as calibref does
        for t in range(nt):
            S[t][t] = f(float(c["sd"][t])) ** 2
    return A, S, [f(float(x)) for x in c["ybar"]], [f(float(x)) for x in c["z"]]


def _mp_solve(c, tabs, m, v):
    """m, v: nr mpf values (v already >= 0) -> u, tau (lists of mpf), chi2, log|C| by forward solves against the 50-digit factor"""
    import mpmath as mp
    A, S, ybar, z = tabs
    nt, nr = c["nt"], c["nr"]
    f = mp.mpf
    Av = [[A[t][k] * v[k] for k in range(nr)] for t in range(nt)]
    rhs = [A[t] + [z[t] - ybar[t] - mp.fsum(A[t][k] * m[k] for k in range(nr))] for t in range(nt)]
    L = [[f(0)] * nt for _ in range(nt)]
    W = [None] * nt
    logdet = f(0)
    for i in range(nt):
        Li = L[i]
        for jj in range(i + 1):
            Lj = L[jj]
            s = S[i][jj] + mp.fsum(Av[i][k] * A[jj][k] for k in range(nr)) - mp.fsum(Li[k] * Lj[k] for k in range(jj))
            if i == jj:
                Li[i] = mp.sqrt(s)
                logdet += mp.log(s)
            else:
                Li[jj] = s / Lj[jj]
        W[i] = [(rhs[i][col] - mp.fsum(Li[k] * W[k][col] for k in range(i))) / Li[i] for col in range(nr + 1)]
    u = [-mp.fsum(W[t][k] * W[t][nr] for t in range(nt)) for k in range(nr)]
    tau = [mp.fsum(W[t][k] ** 2 for t in range(nt)) for k in range(nr)]
    chi2 = mp.fsum(W[t][nr] ** 2 for t in range(nt))
    return u, tau, chi2, logdet


def stat_mp(c, m, v, tabs=None):
    """chi2 and logpdf as mpf, not rounded, from nr mpf means and variances (a variance below 0 counts as 0)"""
    import mpmath as mp
    mp.mp.dps = 50
    tabs = _mp_tables(c) if tabs is None else tabs
    v = [x if x > 0 else mp.mpf(0) for x in v]
    _, _, chi2, logdet = _mp_solve(c, tabs, m, v)
    return chi2, -(chi2 + logdet + c["nt"] * mp.log(2 * mp.pi)) / 2


def grad_mp(c, m, v, gm, gv, tabs=None):
    """the two gradients as lists of d mpf and their sums of |terms|, from mpf (or float) inputs: m, v (nr), gm, gv (nr x d)"""
    import mpmath as mp
    mp.mp.dps = 50
    f = mp.mpf
    tabs = _mp_tables(c) if tabs is None else tabs
    nr, d = c["nr"], len(gm[0])
    live = [not (x < 0) for x in v]
    u, tau, _, _ = _mp_solve(c, tabs, [f(x) for x in m], [f(x) if x > 0 else f(0) for x in v])
    out = [[], [], [], []]
    for j in range(d):
        t1 = [u[k] * f(gm[k][j]) for k in range(nr)]
        t2 = [(u[k] ** 2 if live[k] else f(0)) * f(gv[k][j]) for k in range(nr)]
        t3 = [(u[k] ** 2 - tau[k] if live[k] else f(0)) * f(gv[k][j]) / 2 for k in range(nr)]
        out[0].append(2 * mp.fsum(t1) - mp.fsum(t2))
        out[1].append(mp.fsum(t3) - mp.fsum(t1))
        out[2].append(2 * mp.fsum(abs(x) for x in t1) + mp.fsum(abs(x) for x in t2))
        out[3].append(mp.fsum(abs(x) for x in t1) + mp.fsum(abs(x) for x in t3))
    return out


def direct_mp(c, points):
    """direct64 at 50 digits for the listed points -> g[2, len(points), d], scale[2, len(points), d], float64 (rounded once)"""
    d = c["d"]
    gm, gv = _blocks(c)
    tabs = _mp_tables(c)
    g = np.full((2, len(points), d), np.nan)
    scale = np.full((2, len(points), d), np.nan)
    for i, q in enumerate(points):
        m, v = c["mean"][:, q], c["var"][:, q]
        if not (np.all(np.isfinite(m)) and np.all(np.isfinite(v))):
            continue
        o = grad_mp(c, [float(x) for x in m], [float(x) for x in v], gm[:, q].tolist(), gv[:, q].tolist(), tabs)
        for s in range(2):
            g[s, i] = [float(x) for x in o[s]]
            scale[s, i] = [float(x) for x in o[2 + s]]
    return g, scale


def err(got, ref, scale):
    """|got - ref| / max(1, scale), elementwise; a NaN on both sides is agreement (0), on one side inf"""
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    with np.errstate(invalid="ignore"):
        e = np.abs(got - ref) / np.maximum(1.0, np.nan_to_num(np.asarray(scale, float), nan=0.0))
    both = np.isnan(got) & np.isnan(ref)
    one = np.isnan(got) ^ np.isnan(ref)
    return np.where(both, 0.0, np.where(one, np.inf, e))
