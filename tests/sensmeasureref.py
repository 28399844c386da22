"""CPU references for the closed-form sensitivity analysis under a per-coordinate input measure (gpemu_sens_set_measure,
include/gpemu.h): coordinate l is uniform on [lo_l, hi_l] (kind 0) or Gaussian N(lo_l, hi_l^2) (kind 1: lo is
the MEAN, hi the STANDARD DEVIATION).  Test infrastructure only; no device value enters except as an INPUT.

The measure enters the analysis in four functions and nowhere else: the moments E x^p, the per-point integrals I, J^1..J^3,
the pair integrals II and the prior double integral UU.  This module holds measure-aware versions of those four, with the NP
and the MP backend of sensref.py, and swaps them into sensref / senspostref / senspairref for the duration of a call: the
assembly code of the three references runs unchanged.  A uniform coordinate is computed by the ORIGINAL function on its
columns, so all-uniform kinds reproduce the three references bit for bit.  For a Gaussian coordinate (mean mu, variance
v = sd^2, lengths s and t, D1 = 1 + s v, D2 = 1 + (s + t) v):

  I      = D1^-1/2 exp(-(s / D1) (a - mu)^2 / 2),   J^1 = I c,  J^2 = I (c^2 + w),  J^3 = I (c^3 + 3 c w),
           c = (s v a + mu) / D1,  w = v / D1         (k_l times the density is a Gaussian of mean c and variance w, mass I)
  II     = D2^-1/2 exp(-[s t v (a - b)^2 + s (a - mu)^2 + t (b - mu)^2] / (2 D2))
  E x^n  : m_0 = 1, m_1 = mu, m_n = mu m_{n-1} + (n - 1) v m_{n-2}
  UU     = (1 + 2 s v)^-1/2

The counterparts that use no closed form are tensor quadratures of m and of c* themselves: Gauss-Hermite nodes on a Gaussian
coordinate, Gauss-Legendre nodes on a uniform one.

`python tests/sensmeasureref.py --measure` prints the largest scaled errors of the NP backend against the MP backend over
exactly the cases of tests/test_gpu_sens_measure.py, for the plug-in quantities and for the S quantities; the figures it
printed are written down in that file."""
import contextlib

import numpy as np

import sensref as R
import senspostref as SP
import senspairref as SQ

UNIFORM, GAUSS = 0, 1

_ORIG = dict(moments=R.moments, point_integrals=R.point_integrals, pair_integrals=R.pair_integrals, uu=SP.uu)


# ---------------------------------------------------------------------------------------------------- the Gaussian forms
def gauss_moments(B, mu, sd, pmax=6):
    v = sd * sd
    M = [mu * 0 + 1, mu]
    for n in range(2, pmax + 1):
        M.append(mu * M[n - 1] + (n - 1) * v * M[n - 2])
    return M[:pmax + 1]


def gauss_point_integrals(B, X, s, mu, sd):
    v = sd * sd
    D1 = 1 + s * v
    I = B.exp(-(s / D1) * (X - mu) ** 2 / 2) / B.sqrt(D1)
    c, w = (s * v * X + mu) / D1, v / D1
    return [I, I * c, I * (c * c + w), I * (c * (c * c + 3 * w))]


def gauss_pair_integrals(B, X, s, t, mu, sd):
    v = sd * sd
    D2 = 1 + (s + t) * v
    xa, xb = X[:, None, :], X[None, :, :]
    return B.exp(-(s * t * v * (xa - xb) ** 2 + s * (xa - mu) ** 2 + t * (xb - mu) ** 2) / (2 * D2)) / B.sqrt(D2)


def gauss_uu(B, s, mu, sd):
    return 1 / B.sqrt(1 + 2 * s * sd * sd)


# ---------------------------------------------------------------------------------------------------- per-coordinate kinds
def _split(kind):
    kind = np.asarray(kind, dtype=int).ravel()
    assert np.all((kind == UNIFORM) | (kind == GAUSS))
    return np.flatnonzero(kind == UNIFORM), np.flatnonzero(kind == GAUSS)


def _scatter(parts):
    """parts: [(columns, array[..., len(columns)])] -> one array[..., d]"""
    d = sum(len(c) for c, _ in parts)
    first = parts[0][1]
    out = np.empty(first.shape[:-1] + (d,), dtype=first.dtype)
    for cols, a in parts:
        out[..., cols] = a
    return out


def _measure_functions(kind):
    u, g = _split(kind)

    def moments(B, lo, hi, pmax=6):
        if not len(g):
            return _ORIG["moments"](B, lo, hi, pmax)
        mu_, mg = (_ORIG["moments"](B, lo[u], hi[u], pmax) if len(u) else None), gauss_moments(B, lo[g], hi[g], pmax)
        return [_scatter([(g, mg[p] + lo[g] * 0)] + ([(u, mu_[p] + lo[u] * 0)] if len(u) else [])) for p in range(pmax + 1)]

    def point_integrals(B, X, s, lo, hi):
        if not len(g):
            return _ORIG["point_integrals"](B, X, s, lo, hi)
        pu = _ORIG["point_integrals"](B, X[:, u], s[u], lo[u], hi[u]) if len(u) else None
        pg = gauss_point_integrals(B, X[:, g], s[g], lo[g], hi[g])
        return [_scatter([(g, pg[q])] + ([(u, pu[q])] if len(u) else [])) for q in range(4)]

    def pair_integrals(B, X, s, t, lo, hi):
        if not len(g):
            return _ORIG["pair_integrals"](B, X, s, t, lo, hi)
        parts = [(g, gauss_pair_integrals(B, X[:, g], s[g], t[g], lo[g], hi[g]))]
        if len(u):
            parts.append((u, _ORIG["pair_integrals"](B, X[:, u], s[u], t[u], lo[u], hi[u])))
        return _scatter(parts)

    def uu(B, s, lo, hi):
        if not len(g):
            return _ORIG["uu"](B, s, lo, hi)
        parts = [(g, gauss_uu(B, s[g], lo[g], hi[g]))]
        if len(u):
            parts.append((u, _ORIG["uu"](B, s[u], lo[u], hi[u])))
        return _scatter(parts)

    return moments, point_integrals, pair_integrals, uu


@contextlib.contextmanager
def measure(kind):
    """inside the block sensref / senspostref / senspairref integrate against the measure `kind`"""
    moments, point_integrals, pair_integrals, uu = _measure_functions(kind)
    R.moments, R.point_integrals, R.pair_integrals, SP.uu = moments, point_integrals, pair_integrals, uu
    try:
        yield
    finally:
        R.moments, R.point_integrals, R.pair_integrals, SP.uu = (_ORIG[k] for k in ("moments", "point_integrals", "pair_integrals", "uu"))


def _under(fn):
    def call(kind, *args, **kw):
        with measure(kind):
            return fn(*args, **kw)
    call.__doc__ = f"{fn.__module__}.{fn.__name__} under the measure `kind` (first argument); lo = mean, hi = sd on a Gaussian coordinate"
    return call


covariances = _under(R.covariances)
main_effects = _under(R.main_effects)
post = _under(SP.post)
band = _under(SP.band)
pair_covariances = _under(SQ.pair_covariances)
pair_post = _under(SQ.pair_post)
joint_surface = _under(SQ.joint_surface)


# ---------------------------------------------------------------------------------------------------- quadrature
def nodes_weights(kind, lo, hi, n):
    """per coordinate (nodes, weights summing to 1): Gauss-Legendre on [lo, hi], Gauss-Hermite for N(lo, hi^2)"""
    out = []
    for k, a, b in zip(np.asarray(kind, int), np.asarray(lo, float), np.asarray(hi, float)):
        if k == GAUSS:
            t, w = np.polynomial.hermite_e.hermegauss(n)
            out.append((a + b * t, w / np.sqrt(2 * np.pi)))
        else:
            t, w = np.polynomial.legendre.leggauss(n)
            out.append((a + (t + 1) * (b - a) / 2, w / 2))
    return out


def sample(kind, lo, hi, rng, n):
    """n independent draws from the measure"""
    kind, lo, hi = np.asarray(kind, int), np.asarray(lo, float), np.asarray(hi, float)
    return np.where(kind == GAUSS, lo + hi * rng.standard_normal((n, len(lo))), lo + (hi - lo) * rng.random((n, len(lo))))


def quadrature_fn(kind, fna, fnb, lo, hi, n=40, grid=None):
    """tensor quadrature of two functions of the rows of a query matrix and of their conditional means, d <= 3: the dict of
    sensref.covariances plus cov_pair [npairs] (d >= 2) and, with grid [d x G], main [d x G] of fna"""
    d = len(lo)
    assert d <= 3
    nw = nodes_weights(kind, lo, hi, n)
    mesh = np.stack([g.ravel() for g in np.meshgrid(*[x for x, _ in nw], indexing="ij")], axis=1)
    W = [w for _, w in nw]
    fa = fna(mesh).reshape((n,) * d)
    fb = fa if fnb is fna else fnb(mesh).reshape((n,) * d)

    def cond(f, keep):
        for l in range(d - 1, -1, -1):
            if l not in keep:
                f = np.tensordot(f, W[l], axes=([l], [0]))
        return f

    def expect(f, keep):
        for l in keep:
            f = np.tensordot(f, W[l], axes=([0], [0]))
        return float(f)

    e0a, e0b = expect(fa, range(d)), expect(fb, range(d))

    def cov(keep):
        return expect((cond(fa, keep) - e0a) * (cond(fb, keep) - e0b), keep)

    every = list(range(d))
    out = dict(e0=np.array([e0a, e0b]), cov_all=np.array(cov(every)), cov_first=np.array([cov([j]) for j in every]),
               cov_rest=np.array([cov([l for l in every if l != j]) for j in every]))
    if d >= 2:
        out["cov_pair"] = np.array([cov(list(u)) for u in SQ.pairs(d)])
    if grid is not None:
        main = np.empty(np.shape(grid))
        for j in every:
            free = [l for l in every if l != j]
            sub = np.stack([g.ravel() for g in np.meshgrid(*[nw[l][0] for l in free], indexing="ij")], axis=1) if free else np.zeros((1, 0))
            for gi, x in enumerate(grid[j]):
                pts = np.empty((len(sub), d))
                pts[:, free] = sub
                pts[:, j] = x
                f = fna(pts).reshape((n,) * len(free))
                for l in free:
                    f = np.tensordot(f, W[l], axes=([0], [0]))
                main[j, gi] = float(f)
        out["main"] = main
    return out


def quadrature(kind, X, ma, mb, lo, hi, n=40, grid=None):
    fa = lambda q: R.mean_function(X, ma, q)
    return quadrature_fn(kind, fa, fa if mb is ma else (lambda q: R.mean_function(X, mb, q)), lo, hi, n, grid)


def quadrature_post(kind, X, model, P, G, Q, lo, hi, n=12):
    """s_none, s_all, s_first, s_rest and (d >= 2) s_pair by quadrature of c* on ALL pairs of the n^d tensor nodes, d <= 3"""
    d = len(lo)
    assert d <= 3
    nw = nodes_weights(kind, lo, hi, n)
    mesh = np.stack([g.ravel() for g in np.meshgrid(*[x for x, _ in nw], indexing="ij")], axis=1)
    cs = SP.cstar(X, model, P, G, Q, mesh, mesh).reshape((n,) * (2 * d))

    def s_of(inu):
        f = cs
        for l in range(d - 1, -1, -1):                          # axes l (of x) and l + (axes of x left) (of x')
            k = f.ndim // 2
            if inu[l]:
                f = np.tensordot(np.diagonal(f, axis1=l, axis2=k + l), nw[l][1], axes=([-1], [0]))
            else:
                f = np.tensordot(np.tensordot(f, nw[l][1], axes=([k + l], [0])), nw[l][1], axes=([l], [0]))
        return float(f)

    out = SP._pack(np.array([s_of(inu) for inu in SP._subsets(d)]), d)
    if d >= 2:
        out["s_pair"] = np.array([s_of([l in u for l in range(d)]) for u in SQ.pairs(d)])
    return out


def scaled_errors(got, ref, scale, keys):
    return R.scaled_errors(got, ref, scale, keys)


if __name__ == "__main__":
    import os
    import sys
    if "--measure" in sys.argv:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        import test_gpu_sens_measure
        test_gpu_sens_measure.measure_np_against_mp()
