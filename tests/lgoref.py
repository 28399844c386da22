"""CPU references for K-fold / leave-group-out validation (tests/test_gpu_lgo.py, tests/test_host_lgo.py,
tests/test_lgoref.py).  Test infrastructure only; no device value enters.

"Remove the b training points of a group B, set the emulator up on the other N - b points at the same thetas (GLS beta
re-estimated, variance with the regression term, kappa = cov(x, x) with the nugget), predict jointly at x_B":

  lapack_refits   what the sentence says, from LAPACK: Cholesky factor of C without the rows and columns of B, solves,
                  mean_B and Sigma_B = c - K^T C^-1 K + R Q R^T (symmetrised), e = y_B - mean_B
  closed_form     no refit: P = C^-1 - W Q W^T with C^-1 explicitly from dpotri (as looref.closed_form),
                  cov_B = P_BB^-1, mean_B = y_B - cov_B (P y)_B

and from either the quantities the device returns,

  werr_B = U^-1 e    U the UPPER triangular factor of cov_B = U U^T (the Cholesky factor of the reversed matrix, reversed
                     back; U = R^-T for P_BB = R R^T, so werr_B = R^T e = R^-1 (P y)_B)
  maha = |werr_B|^2, logdet = log det cov_B, logpdf = -1/2 (maha + logdet + b log 2 pi), var = diag(cov_B)

The members of a group are taken in ascending design index.  Both routes read the matrix C, which is not clamped (the
oracle's k-vector zeroes entries below 1e-10: looref.min_offdiag is the precondition for a comparison with oracle refits).

reference() checks itself before it hands anything out: the two routes must agree to PRECOND = 1e-10 in the measures the
device bars (RTOL = 1e-8, the project's parity bar) are set on, and kappa_2(Sigma_B) <= 1e3 for every group:

  mean    max err / max(1, max |mean|)          var     max err / kappa
  werr    max err / max(1, max |werr|)          maha    err / max(1, maha)
  logdet  err / b                               logpdf  err / max(1, |logpdf|)"""
import numpy as np
import scipy.linalg as sl

from oracle import oracle as O

RTOL = 1e-8
PRECOND = 1e-10
KAPPA2_MAX = 1e3
LOG2PI = float(np.log(2.0 * np.pi))


def folds(N, K, seed=None):
    """labels of K interleaved folds: point i in fold i mod K, of a seeded permutation of the points when seed is given"""
    lab = np.arange(N, dtype=np.int32) % K
    if seed is None:
        return lab
    out = np.empty(N, dtype=np.int32)
    out[np.random.default_rng(seed).permutation(N)] = lab
    return out


def ragged(N, sizes, seed):
    """labels of groups of the given sizes drawn from a seeded permutation; the points left over get -1"""
    assert sum(sizes) <= N
    perm = np.random.default_rng(seed).permutation(N)
    lab = np.full(N, -1, dtype=np.int32)
    o = 0
    for g, b in enumerate(sizes):
        lab[perm[o:o + b]] = g
        o += b
    return lab


def members(group, ngroups=None):
    """-> the index array of every group, ascending"""
    group = np.asarray(group)
    ngroups = int(group.max()) + 1 if ngroups is None else ngroups
    return [np.flatnonzero(group == g) for g in range(ngroups)]


def upper_factor(S):
    """U upper triangular with positive diagonal and S = U U^T"""
    L = sl.cholesky(S[::-1, ::-1], lower=True, check_finite=False)
    return L[::-1, ::-1]


def _finish(mean, cov, yB):
    b = len(yB)
    U = upper_factor(cov)
    e = yB - mean
    w = sl.solve_triangular(U, e, lower=False, check_finite=False)
    maha = float(w @ w)
    logdet = float(2.0 * np.sum(np.log(np.diag(U))))
    return dict(mean=mean, cov=cov, var=np.diag(cov).copy(), werr=w, maha=maha, logdet=logdet,
                logpdf=-0.5 * (maha + logdet + b * LOG2PI))


def lapack_refits(Cm, H, y, groups):
    """-> one dict(mean, cov, var, werr, maha, logdet, logpdf) per group, each from a Cholesky refit on the other points"""
    N = len(y)
    out = []
    for B in groups:
        keep = np.ones(N, dtype=bool)
        keep[B] = False
        cf = sl.cho_factor(Cm[np.ix_(keep, keep)], lower=True, overwrite_a=True, check_finite=False)
        Hk, yk, K = H[keep], y[keep], Cm[np.ix_(keep, B)]
        S = sl.cho_solve(cf, np.column_stack([yk, Hk, K]), check_finite=False)
        nreg = H.shape[1]
        Cy, CH, CK = S[:, 0], S[:, 1:1 + nreg], S[:, 1 + nreg:]
        Q = np.linalg.inv(Hk.T @ CH)
        beta = Q @ (Hk.T @ Cy)
        R = H[B] - K.T @ CH                                  # r_p = h(x_p) - H^T C^-1 k_p, one row per member
        mean = H[B] @ beta + K.T @ (Cy - CH @ beta)
        Sig = Cm[np.ix_(B, B)] - K.T @ CK + R @ Q @ R.T
        out.append(_finish(mean, 0.5 * (Sig + Sig.T), y[B]))
    return out


def closed_form(Cm, H, y, groups):
    """the same from the explicit inverse of the FULL matrix (dpotrf + dpotri), no refit"""
    c, info = sl.lapack.dpotrf(Cm, lower=1)
    assert info == 0
    Ci, info = sl.lapack.dpotri(c, lower=1)
    assert info == 0
    Ci = np.tril(Ci) + np.tril(Ci, -1).T
    W = Ci @ H
    Q = np.linalg.inv(H.T @ W)
    gamma = Ci @ y - W @ (Q @ (W.T @ y))
    out = []
    for B in groups:
        P = Ci[np.ix_(B, B)] - W[B] @ Q @ W[B].T
        P = 0.5 * (P + P.T)
        cov = sl.cho_solve(sl.cho_factor(P, lower=True, check_finite=False), np.eye(len(B)), check_finite=False)
        cov = 0.5 * (cov + cov.T)
        out.append(_finish(y[B] - cov @ gamma[B], cov, y[B]))
    return out


def errors(got, ref, kappa):
    """the six measures for ONE group, got and ref dicts with mean, var, werr, maha, logdet, logpdf"""
    b = len(ref["mean"])
    return dict(mean=float(np.max(np.abs(got["mean"] - ref["mean"])) / max(1.0, float(np.max(np.abs(ref["mean"]))))),
                var=float(np.max(np.abs(got["var"] - ref["var"])) / kappa),
                werr=float(np.max(np.abs(got["werr"] - ref["werr"])) / max(1.0, float(np.max(np.abs(ref["werr"]))))),
                maha=float(abs(got["maha"] - ref["maha"]) / max(1.0, ref["maha"])),
                logdet=float(abs(got["logdet"] - ref["logdet"]) / b),
                logpdf=float(abs(got["logpdf"] - ref["logpdf"]) / max(1.0, abs(ref["logpdf"]))))


def worst(errs):
    """the largest of each measure over a list of errors() dicts"""
    return {k: max(e[k] for e in errs) for k in errs[0]}


def split(res, groups):
    """a device result (design-order mean, var, werr; per-group maha, logdet, logpdf) -> one dict per group, as the routes give"""
    return [dict(mean=res["mean"][B], var=res["var"][B], werr=res["werr"][B], maha=float(res["maha"][g]),
                 logdet=float(res["logdet"][g]), logpdf=float(res["logpdf"][g])) for g, B in enumerate(groups)]


def join(per_group, groups, N):
    """the inverse of split(): design-order arrays (NaN where no group holds the point) and per-group arrays"""
    out = dict(mean=np.full(N, np.nan), var=np.full(N, np.nan), werr=np.full(N, np.nan))
    for r, B in zip(per_group, groups):
        for k in ("mean", "var", "werr"):
            out[k][B] = r[k]
    for k in ("maha", "logdet", "logpdf"):
        out[k] = np.array([r[k] for r in per_group])
    return out


def reference_from(Cm, H, y, group, ngroups=None):
    """-> dict(per_group (the refits' list), groups, kappa, ref_err (the worst disagreement of the two routes per measure),
    kappa2 (the largest kappa_2(Sigma_B)), and the joined design-order arrays), after asserting that the reference is good"""
    groups = members(group, ngroups)
    assert all(len(B) for B in groups)
    kappa = float(Cm[0, 0])
    refit = lapack_refits(Cm, H, y, groups)
    closed = closed_form(Cm, H, y, groups)
    e = worst([errors(c, r, kappa) for c, r in zip(closed, refit)])
    k2 = 0.0
    for r in refit:
        lam = np.linalg.eigvalsh(r["cov"])
        k2 = max(k2, float(lam[-1] / lam[0]))
    assert k2 <= KAPPA2_MAX, ("ill-conditioned test inputs: kappa_2(Sigma_B)", k2)
    assert all(v <= PRECOND for v in e.values()), ("ill-conditioned test inputs: the two CPU routes disagree", e)
    out = join(refit, groups, len(y))
    out.update(per_group=refit, groups=groups, kappa=kappa, ref_err=e, kappa2=k2)
    return out


def reference(kind, order, X, y, th, group, ngroups=None):
    return reference_from(O.cov_matrix(kind, X, th), O.hmatrix(order, X), y, group, ngroups)
