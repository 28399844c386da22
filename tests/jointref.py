"""CPU reference for hold-out validation and joint draws at query points (tests/test_gpu_predict_joint.py,
tests/test_host_joint.py, tests/test_jointref.py).  Test infrastructure only; no device value enters.

  S = Sigma + diag(noise),  S = L L^T,  werr_a = L^-1 (yobs_a - mean),  maha_a = |werr_a|^2,  logdet = 2 sum log L_pp,
  logpdf_a = -1/2 (maha_a + logdet + M log 2 pi),  out_s = mean + L z_s

Sigma and the mean are predcovref.predict's (the oracle's matrix elements, LAPACK's solves), symmetrised by averaging the
two triangles (they differ by rounding); L is LAPACK's dpotrf, the solves its dtrtrs.

Like its siblings, reference() checks itself before it hands anything out: the factor and the forward solves are repeated on
numpy's longdouble (vargradref.chol_ld and a forward substitution written out; mpmath at 40 digits where longdouble is no
wider than double) from the SAME S, and the two must agree to PRECOND = 1e-10 in the measures the device bars are set on:

  werr    max |werr - ref| / max(1, max |ref|)
  maha    |maha - ref| / max(1, ref)
  logdet  |logdet - ref| / M
  out     max |out - ref| / (sqrt(max S_pp) max(1, max |z|))

It also asserts kappa_2(S) <= 1e3 (eigvalsh), predcovref's own precondition on Sigma and the mean, and that logpdf agrees with
scipy.stats.multivariate_normal.logpdf -- which factors S by eigh, shares nothing with the Cholesky route and carries a
relative error of the order of kappa_2 M eps in both of its terms: bar 4 kappa_2 M 2^-52 max(1, |logpdf|).

Every quantity of a call on the first M' of the M queries is the leading part of the call on all of them -- S' is the leading
block of S, L' of L, werr' the leading columns of werr (forward substitution) -- so ONE reference serves every smaller M:
leading()."""
import numpy as np
import scipy.linalg as sl

import predcovref
import vargradref

RTOL = vargradref.RTOL
PRECOND = vargradref.PRECOND
EPS = vargradref.EPS
LD = vargradref.LD
KAPPA2_MAX = 1e3
LOG2PI = float(np.log(2.0 * np.pi))


def fresh_queries(X, M, seed):
    """M queries drawn uniformly in the bounding box of the design: none on a training point, no two alike (the query sets of
    the other prediction tests hold both, and their Sigma is singular)"""
    rng = np.random.default_rng(seed)
    lo, hi = X.min(axis=0), X.max(axis=0)
    return lo + (hi - lo) * rng.random((M, X.shape[1]))


def noise_for(kap, M, seed):
    """observation noise of 5 .. 15 % of kappa per point"""
    return kap * (0.05 + 0.1 * np.random.default_rng(seed).random(M))


def forward_ld(L, B):
    """L^-1 B on longdouble, written out"""
    B = B.astype(LD).copy()
    for i in range(L.shape[0]):
        B[i] = (B[i] - L[i, :i] @ B[:i]) / L[i, i]
    return B


def mpmath_factor(S, D, Z, dps=40):
    """the extended route on mpmath -> (werr, out - mean, logdet) as float64 arrays of values rounded once"""
    import mpmath as mp
    with mp.workdps(dps):
        L = mp.cholesky(mp.matrix(S.tolist()))
        W = (L ** -1) * mp.matrix(D.T.tolist()) if D.shape[0] else None
        O_ = L * mp.matrix(Z.T.tolist()) if Z.shape[0] else None
        M = S.shape[0]
        w = np.array([[float(W[p, a]) for p in range(M)] for a in range(D.shape[0])]).reshape(D.shape)
        o = np.array([[float(O_[p, s]) for p in range(M)] for s in range(Z.shape[0])]).reshape(Z.shape)
        return w, o, float(2 * sum(mp.log(L[p, p]) for p in range(M)))


def extended_factor(S, D, Z):
    """-> (werr, L z rows, logdet) from the extended-precision route"""
    if not vargradref.LD_IS_EXTENDED:
        return mpmath_factor(S, D, Z)
    L = vargradref.chol_ld(S)
    w = forward_ld(L, D.T).T if D.shape[0] else np.zeros(D.shape, dtype=LD)
    o = (L @ Z.T.astype(LD)).T if Z.shape[0] else np.zeros(Z.shape, dtype=LD)
    return w, o, 2 * np.sum(np.log(np.diag(L)))


def errors(got, ref, M, zmax=1.0, smax=1.0):
    """the four measures, got and ref dicts with werr, maha, logdet, out (any may be missing in got: skipped)"""
    e = {}
    if "werr" in got and ref["werr"].size:
        e["werr"] = float(np.max(np.abs(got["werr"] - ref["werr"])) / max(1.0, float(np.max(np.abs(ref["werr"])))))
        e["maha"] = float(np.max(np.abs(got["maha"] - ref["maha"]) / np.maximum(1.0, np.asarray(ref["maha"], dtype=np.float64))))
    if "logdet" in got:
        e["logdet"] = float(abs(got["logdet"] - ref["logdet"]) / M)
    if "out" in got and ref["out"].size:
        e["out"] = float(np.max(np.abs(got["out"] - ref["out"])) / (np.sqrt(smax) * max(1.0, zmax)))
    return e


def predict(kind, order, X, y, th, Xq, noise=None, yobs=None, z=None, cov=None):
    """-> dict(S, L, mean, var, werr, maha, logdet, logpdf, out, z, yobs, kappa, cov) in float64, unchecked.  yobs: nobs x M or
    None; z: ndraw x M or None; cov: predcovref's dict for these queries when the caller has it already"""
    cov = predcovref.predict(kind, order, X, y, th, Xq) if cov is None else cov
    M = cov["cov"].shape[0]
    S = 0.5 * (cov["cov"] + cov["cov"].T)
    if noise is not None:
        S = S + np.diag(np.asarray(noise, dtype=np.float64).reshape(M))
    yobs = np.zeros((0, M)) if yobs is None else np.asarray(yobs, dtype=np.float64).reshape(-1, M)
    z = np.zeros((0, M)) if z is None else np.asarray(z, dtype=np.float64).reshape(-1, M)
    L = sl.cholesky(S, lower=True, check_finite=False)
    D = yobs - cov["mean"]
    werr = sl.solve_triangular(L, D.T, lower=True, check_finite=False).T if D.shape[0] else D.copy()
    maha = np.sum(werr * werr, axis=1)
    logdet = float(2.0 * np.sum(np.log(np.diag(L))))
    return dict(S=S, L=L, mean=cov["mean"], var=np.diag(S).copy(), werr=werr, maha=maha, logdet=logdet,
                logpdf=-0.5 * (maha + logdet + M * LOG2PI), out=cov["mean"] + z @ L.T, z=z, yobs=yobs, kappa=cov["kappa"], cov=cov)


def leading(ref, M):
    """the reference of the call on the first M queries, from the reference of a call on more"""
    L = ref["L"][:M, :M]
    werr = ref["werr"][:, :M]
    maha = np.sum(werr * werr, axis=1)
    logdet = float(2.0 * np.sum(np.log(np.diag(L))))
    z = ref["z"][:, :M]
    return dict(S=ref["S"][:M, :M], L=L, mean=ref["mean"][:M], var=ref["var"][:M], werr=werr, maha=maha, logdet=logdet,
                logpdf=-0.5 * (maha + logdet + M * LOG2PI), out=ref["mean"][:M] + z @ L.T, z=z, yobs=ref["yobs"][:, :M],
                kappa=ref["kappa"])


def observations(ref, nobs, seed, scale=1.3):
    """nobs rows of observations for a reference made without any: draws from N(mean, scale^2 S)"""
    zz = scale * np.random.default_rng(seed).standard_normal((nobs, ref["mean"].size))
    return ref["mean"] + zz @ ref["L"].T


def reference_errors(ref):
    """-> (the four measures of the float64 reference against the extended-precision route, kappa_2(S))"""
    M = ref["S"].shape[0]
    w, o, ld = extended_factor(ref["S"], ref["yobs"] - ref["mean"], ref["z"])
    ext = dict(werr=w, maha=np.sum(w * w, axis=1), logdet=ld, out=ref["mean"] + o)
    zmax = float(np.max(np.abs(ref["z"]))) if ref["z"].size else 1.0
    e = errors(ref, ext, M, zmax, float(ref["var"].max()))
    lam = np.linalg.eigvalsh(ref["S"])
    return e, float(lam[-1] / lam[0])


def reference(kind, order, X, y, th, Xq, noise=None, yobs=None, z=None, nobs=0, seed=0, cov=None):
    """predict(), after asserting that the reference is good on these inputs (module docstring).  yobs None and nobs > 0: the
    observations are drawn by observations().  cov: predcovref.reference's dict for these inputs when the caller has it.
    The measured figures come back as 'ref_err' (dict) and 'kappa2'."""
    import scipy.stats as st
    cov = predcovref.reference(kind, order, X, y, th, Xq) if cov is None else cov
    ref = predict(kind, order, X, y, th, Xq, noise, yobs, z, cov=cov)
    if yobs is None and nobs > 0:
        ref = predict(kind, order, X, y, th, Xq, noise, observations(ref, nobs, seed), z, cov=cov)
    e, k2 = reference_errors(ref)
    assert k2 <= KAPPA2_MAX, ("ill-conditioned test inputs: kappa_2(S)", k2)
    assert all(v <= PRECOND for v in e.values()), ("ill-conditioned test inputs: reference errors", e)
    M = ref["S"].shape[0]
    if ref["yobs"].shape[0]:
        lp = np.atleast_1d(st.multivariate_normal.logpdf(ref["yobs"], mean=ref["mean"], cov=ref["S"]))
        elp = float(np.max(np.abs(lp - ref["logpdf"]) / np.maximum(1.0, np.abs(ref["logpdf"]))))
        assert elp <= 4.0 * k2 * M * EPS, ("logpdf against scipy.stats.multivariate_normal", elp, 4.0 * k2 * M * EPS)
        e["logpdf_scipy"] = elp
    ref["ref_err"], ref["kappa2"] = e, k2
    return ref
