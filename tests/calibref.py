"""References for the calibration entries (gpemu_calib_*): the DIRECT nt x nt form, never the r-form the
library evaluates.

  direct64   float64: Cholesky of S + A D A^T per point (numpy / LAPACK), the per-output implausibilities with their sums
             over the components in index order from 0.0
  direct_mp  the same at 50 digits (mpmath), for the points asked for
  rform64    the r x r identity written in numpy on top of a projection (m_hat, Sigma_z, constants): the algebra the device
             evaluates, for checking on the CPU that it stays inside the bars before a device runs

Error measure everywhere: |got - ref| / max(1, |ref|) per statistic.

BARS, per statistic (chi2, logpdf, I1, I2, I3): 8 x MEASURED, the largest error of direct64 against direct_mp over the points
mp_points takes of every input family of CASES and SPECIALS below (v_huge apart: float64 cannot factor S + A D A^T at
v = 1e30, that family is compared with direct_mp alone), rounded up to one digit.  Measured on the CPU before a device ran:
    chi2 5.5e-15   logpdf 1.9e-13   I1 9.4e-16   I2 1.8e-15   I3 1.8e-15
(test_calibref.py recomputes them and asserts that none exceeds MEASURED).  logpdf is the loosest because
chi2 + log|S + A D A^T| + nt log 2 pi cancels to O(1) from terms of a few hundred at nt = 65.  The families have
cond(S) <= 4e2 and cond(G) <= 2e3, far inside the 1e8 the entries are specified for.  The r x r identity itself, in float64
on gpemu_calib_project's tables (rform64), is within 3.1e-15 (chi2) and 3.2e-14 (logpdf) of direct_mp on the same points.
"""
import zlib

import numpy as np

STATS = ("chi2", "logpdf", "I1", "I2", "I3")
MEASURED = np.array([6e-15, 2e-13, 1e-15, 2e-15, 2e-15])
BARS = 8.0 * MEASURED
LOG2PI = 1.8378770664093454835606594728112

# (name, nr, nt, M, full S, rel, extra columns of the leading dimension)
CASES = [
    ("r1_nt1", 1, 1, 1, False, False, 0),
    ("r2_nt2_full", 2, 2, 63, True, False, 0),
    ("r3_nt3_rel", 3, 3, 64, False, True, 0),
    ("r4_nt7_full", 4, 7, 65, True, False, 0),
    ("r5_nt7", 5, 7, 257, False, False, 3),
    ("r8_nt64_full_rel", 8, 64, 1000, True, True, 24),
    ("r9_nt65_rel", 9, 65, 257, False, True, 0),
    ("r12_nt64_full", 12, 64, 65, True, False, 0),
    ("r13_nt130_rel", 13, 130, 64, False, True, 0),
    ("r16_nt65_full_rel", 16, 65, 257, True, True, 7),
    ("r16_nt16", 16, 16, 63, False, False, 0),
    ("r8_nt130", 8, 130, 1000, False, False, 0),
]
SPECIALS = ("v_zero", "v_negative", "v_huge", "one_nan", "ties")


def make_case(name, nr, nt, M, full, rel, pad=0, seed=None):
    """A seeded observation set and the components' means and variances at M points.  A = orthonormal columns times decaying
    scales (what pca_evecs_r sqrt(pca_evals_r) looks like), S = diag(sd) Corr diag(sd)."""
    rng = np.random.default_rng(zlib.crc32(name.encode()) if seed is None else seed)
    Q, _ = np.linalg.qr(rng.standard_normal((nt, nr)))
    scales = 2.0 * 10.0 ** (-1.5 * np.arange(nr) / max(nr, 1))
    A = np.ascontiguousarray(Q * scales)
    ybar = rng.uniform(0.5, 3.0, nt)
    sd = rng.uniform(0.05, 0.3, nt)
    S = None
    if full:
        F = rng.standard_normal((nt, 3))
        Cm = 0.6 * np.eye(nt) + 0.4 * (F @ F.T) / 3.0
        dg = np.sqrt(np.diag(Cm))
        Cm = Cm / np.outer(dg, dg)
        S = np.outer(sd, sd) * Cm
        S = 0.5 * (S + S.T)
    m_true = rng.standard_normal(nr)
    z = ybar + A @ m_true + sd * rng.standard_normal(nt)
    ld = M + pad
    mean = np.full((nr, ld), 1e300)                      # the columns beyond M must never be read into a result
    var = np.full((nr, ld), 1e300)
    mean[:, :M] = m_true[:, None] + 0.7 * rng.standard_normal((nr, M))
    var[:, :M] = np.exp(rng.normal(-3.0, 1.5, (nr, M)))
    return dict(name=name, nt=nt, nr=nr, M=M, ybar=ybar, A=A, z=z, S=S, sd=None if full else sd,
                rel=rng.uniform(0.0, 0.1, nt) if rel else None, mean=mean, var=var)


def make_special(kind):
    """the special inputs on one small shape (nr = 5, nt = 7, M = 65, diagonal S, with rel)"""
    c = make_case("special_" + kind, 5, 7, 65, False, True, seed=4242)
    M = c["M"]
    if kind == "v_zero":
        c["var"][:, :M] = 0.0
    elif kind == "v_negative":
        c["var"][:, :M] = -np.abs(c["var"][:, :M]) * 1e-14
    elif kind == "v_huge":
        c["var"][:, :M] = 1e30
    elif kind == "one_nan":
        c["mean"][2, 17] = np.nan
    elif kind == "ties":
        # outputs 2 and 5 are the same output twice and the worst of all: an exact tie, the smaller index wins
        for k in ("ybar", "z", "sd", "rel"):
            c[k][5] = c[k][2]
        c["A"][5] = c["A"][2]
        c["z"][2] = c["z"][5] = c["ybar"][2] + 40.0
    c["name"] = "special_" + kind
    return c


def all_cases():
    return [make_case(*a) for a in CASES] + [make_special(k) for k in SPECIALS]


def _smat(c):
    return c["S"] if c["S"] is not None else np.diag(c["sd"] ** 2)


def _top3(I):
    """I: (M, nt) -> the three largest per row (0 where nt leaves none) and the first index of the largest"""
    M, nt = I.shape
    srt = -np.sort(-I, axis=1)
    top = np.zeros((3, M))
    top[:min(3, nt)] = srt[:, :3].T
    return top, np.argmax(I, axis=1)


def direct64(c):
    """-> stat[5, M], worst[M], in float64 by the direct form; a variance below 0 counts as 0"""
    nt, nr, M = c["nt"], c["nr"], c["M"]
    A, S = c["A"], _smat(c)
    m = c["mean"][:, :M].T                               # M x nr
    v = c["var"][:, :M].T
    v = np.where(v < 0.0, 0.0, v)
    stat = np.full((5, M), np.nan)
    y = np.zeros((M, nt))
    den = np.zeros((M, nt))
    for k in range(nr):                                  # index order from 0.0
        y += A[None, :, k] * m[:, k, None]
        den += (A[None, :, k] * A[None, :, k]) * v[:, k, None]
    y = c["ybar"][None, :] + y
    rel = c["rel"] if c["rel"] is not None else np.zeros(nt)
    den = den + np.diag(S)[None, :] + (rel[None, :] * y) ** 2
    I = np.abs(c["z"][None, :] - y) / np.sqrt(den)
    ok = np.all(np.isfinite(m), axis=1) & np.all(np.isfinite(v), axis=1)
    for q in range(M):
        if not ok[q]:
            continue
        Cq = S + (A * v[q][None, :]) @ A.T
        try:
            L = np.linalg.cholesky(Cq)
        except np.linalg.LinAlgError:
            continue
        w = _forward(L, c["z"] - (c["ybar"] + A @ m[q]))
        chi2 = float(w @ w)
        stat[0, q] = chi2
        stat[1, q] = -0.5 * (chi2 + 2.0 * np.sum(np.log(np.diag(L))) + nt * LOG2PI)
    top, worst = _top3(I)
    stat[2:5] = top
    stat[2:5, ~ok] = np.nan
    worst = np.where(ok, worst, -1).astype(np.int32)
    return stat, worst


def _forward(L, b):
    import scipy.linalg
    return scipy.linalg.solve_triangular(L, b, lower=True)


def direct_mp(c, points):
    """the same at 50 digits for the listed points -> stat[5, len(points)] as float64 (rounded once at the end), worst"""
    import mpmath as mp
    mp.mp.dps = 50
    nt, nr = c["nt"], c["nr"]
    f = mp.mpf
    A = [[f(float(x)) for x in row] for row in c["A"]]
    S = [[f(float(x)) for x in row] for row in _smat(c)]
    if c["S"] is None:                                   # the diagonal form squares sd in extended precision
        for t in range(nt):
            S[t][t] = f(float(c["sd"][t])) ** 2
    ybar = [f(float(x)) for x in c["ybar"]]
    z = [f(float(x)) for x in c["z"]]
    rel = [f(float(x)) for x in (c["rel"] if c["rel"] is not None else np.zeros(nt))]
    out = np.full((5, len(points)), np.nan)
    worst = np.full(len(points), -1, dtype=np.int32)
    for j, q in enumerate(points):
        mq, vq = c["mean"][:, q], c["var"][:, q]
        if not (np.all(np.isfinite(mq)) and np.all(np.isfinite(vq))):
            continue
        m = [f(float(x)) for x in mq]
        v = [f(float(x)) if x > 0 else f(0) for x in vq]
        y = [ybar[t] + mp.fsum(A[t][k] * m[k] for k in range(nr)) for t in range(nt)]
        I = [abs(z[t] - y[t]) / mp.sqrt(mp.fsum(A[t][k] ** 2 * v[k] for k in range(nr)) + S[t][t] + (rel[t] * y[t]) ** 2)
             for t in range(nt)]
        Av = [[A[t][k] * v[k] for k in range(nr)] for t in range(nt)]
        L = [[f(0)] * nt for _ in range(nt)]
        w = [f(0)] * nt
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
            w[i] = (z[i] - y[i] - mp.fsum(Li[k] * w[k] for k in range(i))) / Li[i]
        chi2 = mp.fsum(x * x for x in w)
        out[0, j] = float(chi2)
        out[1, j] = float(-(chi2 + logdet + nt * mp.log(2 * mp.pi)) / 2)
        srt = sorted(I, reverse=True)
        for k in range(3):
            out[2 + k, j] = float(srt[k]) if k < nt else 0.0
        worst[j] = int(max(range(nt), key=lambda t: (I[t], -t)))
    return out, worst


def mp_points(c):
    """the points of a case that the 50-digit repeat takes: fewer where an nt x nt factorisation at 50 digits is slow"""
    k = 8 if c["nt"] <= 16 else (4 if c["nt"] <= 65 else 2)
    pts = list(range(min(k, c["M"])))
    if c["name"] == "special_one_nan":
        pts.append(17)
    return pts


def project_mp(c):
    """m_hat, Sigma_z, c_perp, log|S|, log|G| at 50 digits, by the definitions (S^-1 through its Cholesky factor) -> float64"""
    import mpmath as mp
    mp.mp.dps = 50
    nt, nr = c["nt"], c["nr"]
    A = mp.matrix(c["A"].tolist())
    S = mp.matrix(_smat(c).tolist())
    if c["S"] is None:
        for t in range(nt):
            S[t, t] = mp.mpf(float(c["sd"][t])) ** 2
    r = mp.matrix((c["z"] - 0.0).tolist()) - mp.matrix(c["ybar"].tolist())
    Si = S ** -1
    G = A.T * Si * A
    Gi = G ** -1
    mhat = Gi * (A.T * Si * r)
    e = r - A * mhat
    cperp = (e.T * Si * e)[0]
    tof = lambda Mx: np.array([[float(Mx[i, j]) for j in range(Mx.cols)] for i in range(Mx.rows)])
    return dict(mhat=tof(mhat).ravel(), sigz=tof(Gi), c_perp=float(cperp), logdet_S=float(mp.log(mp.det(S))),
                logdet_G=float(mp.log(mp.det(G))))


def rform64(c, proj):
    """the r x r identity in numpy on a projection (dict with mhat, sigz, c_perp, logdet_S, logdet_G): chi2 and logpdf per
    point -> (2, M)"""
    M, nt = c["M"], c["nt"]
    out = np.full((2, M), np.nan)
    for q in range(M):
        m, v = c["mean"][:, q], c["var"][:, q]
        if not (np.all(np.isfinite(m)) and np.all(np.isfinite(v))):
            continue
        T = proj["sigz"] + np.diag(np.where(v < 0.0, 0.0, v))
        L = np.linalg.cholesky(T)
        y = _forward(L, m - proj["mhat"])
        chi2 = proj["c_perp"] + float(y @ y)
        out[0, q] = chi2
        out[1, q] = -0.5 * (chi2 + proj["logdet_S"] + proj["logdet_G"] + 2.0 * np.sum(np.log(np.diag(L))) + nt * LOG2PI)
    return out


def err(got, ref):
    """|got - ref| / max(1, |ref|), elementwise; a NaN on both sides is agreement (0), on one side inf"""
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    with np.errstate(invalid="ignore"):
        e = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    both = np.isnan(got) & np.isnan(ref)
    one = np.isnan(got) ^ np.isnan(ref)
    return np.where(both, 0.0, np.where(one, np.inf, e))


def worst_comparable(stat_ref, bar_I1=None):
    """the points whose worst output is decided: the top two implausibilities differ by more than the bar"""
    bar = BARS[2] if bar_I1 is None else bar_I1
    with np.errstate(invalid="ignore"):
        gap = np.abs(stat_ref[2] - stat_ref[3]) / np.maximum(1.0, np.abs(stat_ref[2]))
    return gap > bar
