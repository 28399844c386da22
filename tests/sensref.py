"""CPU references for the closed-form sensitivity analysis of the posterior mean (gpemu_sens_cov / gpemu_sens_main,
include/gpemu.h).  Test infrastructure only; no device value enters.

The function analysed is the power-exponential posterior mean without the k-vector clamp,

  m(x) = beta_0 + sum_l q_l(x_l) + A sum_i gamma_i prod_l k_l(x_il, x_l),   q_l(x) = sum_{p=1..order} beta_{p,l} x^p,
  k_l(a, x) = exp(-s_l (x - a)^2 / 2),

under independent uniform inputs on the box [lo_l, hi_l].  A model is a dict(beta [1 + order d], gamma [N], A, s [d]); two
models on one design give the cross case.  Three references:

  1. `covariances` / `main_effects` with the NP backend: the closed forms in numpy fp64 with scipy's erf / erfc,
  2. the same functions with the MP backend: mpmath at 50 digits (object arrays), which measures what fp64 loses,
  3. `quadrature`: tensor Gauss-Legendre quadrature of m and of its conditional means (d <= 3), which uses no closed form.

Every value comes with its SCALE: the sum of the absolute values of the parts it is made of -- polynomial x polynomial,
polynomial x kernel, kernel x kernel and E0a E0b for a covariance; the polynomial and the kernel part for E0 and a main
effect.  Errors are measured relative to that scale (`scaled_errors`): it is what a sum of those parts can be computed to,
however small the covariance itself.

The parts are assembled here in RAW form, E[m_u^a m_u^b] - E0a E0b with nothing centred; the device centres first.  The two
are the same number, reached by different arithmetic.

`python tests/sensref.py --measure` prints the largest scaled error of backend 1 against backend 2 over the cases of
tests/test_gpu_sens.py (minutes: mpmath); the figure it printed is written down in that file as NP_VS_MP."""
import numpy as np
import scipy.special as sp

try:
    import mpmath as _mp
except ImportError:                      # the GPU tests need backend 1 only
    _mp = None


# ---------------------------------------------------------------------------------------------------- backends
class NP:
    """numpy fp64"""
    pi = np.pi

    @staticmethod
    def arr(x):
        return np.asarray(x, dtype=np.float64)

    exp = staticmethod(np.exp)
    sqrt = staticmethod(np.sqrt)

    @staticmethod
    def derf(ulo, uhi):
        """erf(uhi) - erf(ulo) for uhi >= ulo.  Two arguments of one sign: the erfc form -- erf's difference loses all
        relative accuracy beyond |u| of about 4, erfc's does not."""
        same = (ulo > 0) | (uhi < 0)
        near = np.minimum(np.abs(ulo), np.abs(uhi))
        far = np.maximum(np.abs(ulo), np.abs(uhi))
        return np.where(same, sp.erfc(near) - sp.erfc(far), sp.erf(uhi) - sp.erf(ulo))

    @staticmethod
    def tofloat(x):
        return np.asarray(x, dtype=np.float64)


class NPNaive(NP):
    """numpy fp64 with the erf difference as written in the textbook: what the erfc form is there to avoid"""
    @staticmethod
    def derf(ulo, uhi):
        return sp.erf(uhi) - sp.erf(ulo)


def _mp_derf(ulo, uhi):
    if ulo > 0:
        return _mp.erfc(ulo) - _mp.erfc(uhi)
    if uhi < 0:
        return _mp.erfc(-uhi) - _mp.erfc(-ulo)
    return _mp.erf(uhi) - _mp.erf(ulo)


class MP:
    """mpmath, 50 digits, element-wise on numpy object arrays"""
    DPS = 50

    def __init__(self):
        assert _mp is not None, "mpmath is not installed"
        _mp.mp.dps = self.DPS
        self.pi = _mp.pi
        self.exp = np.frompyfunc(_mp.exp, 1, 1)
        self.sqrt = np.frompyfunc(_mp.sqrt, 1, 1)
        self.derf = np.frompyfunc(_mp_derf, 2, 1)
        self._mpf = np.frompyfunc(lambda v: _mp.mpf(float(v)), 1, 1)

    def arr(self, x):
        return np.asarray(self._mpf(np.asarray(x, dtype=np.float64)), dtype=object)

    @staticmethod
    def tofloat(x):
        return np.asarray(np.frompyfunc(float, 1, 1)(np.asarray(x, dtype=object)), dtype=np.float64)


# ---------------------------------------------------------------------------------------------------- pieces
def order_of(model, d):
    return (len(model["beta"]) - 1) // d


def _coef(B, model, d):
    """-> beta_0, c[p - 1][l] = beta_{p,l} (regression.c:9-67: the constant, then x, then x^2, then x^3, d columns each)"""
    beta = B.arr(model["beta"])
    order = order_of(model, d)
    return beta[0], [beta[1 + p * d:1 + (p + 1) * d] for p in range(order)]


def moments(B, lo, hi, pmax=6):
    """M[p][l] = E[x_l^p], p = 0 .. pmax"""
    w = hi - lo
    return [(hi ** (p + 1) - lo ** (p + 1)) / ((p + 1) * w) for p in range(pmax + 1)]


def point_integrals(B, X, s, lo, hi):
    """-> [I, J^1, J^2, J^3], N x d each: (1/w_l) int x^p k_l(x_il, x) dx over [lo_l, hi_l]"""
    w = hi - lo
    r = B.sqrt(s / 2)
    K0 = B.sqrt(B.pi / (2 * s)) * B.derf(r * (lo - X), r * (hi - X))
    khi = B.exp(-s * (hi - X) ** 2 / 2)
    klo = B.exp(-s * (lo - X) ** 2 / 2)
    K1 = X * K0 - (khi - klo) / s
    K2 = X * K1 + (K0 - (hi * khi - lo * klo)) / s
    K3 = X * K2 + (2 * K1 - (hi * hi * khi - lo * lo * klo)) / s
    return [K0 / w, K1 / w, K2 / w, K3 / w]


def pair_integrals(B, X, s, t, lo, hi):
    """-> II[i, i', l] = (1/w_l) int k_l^a(x_il, x) k_l^b(x_i'l, x) dx"""
    w = hi - lo
    st = s + t
    xa, xb = X[:, None, :], X[None, :, :]
    c = (s * xa + t * xb) / st
    al = B.sqrt(st / 2)
    E = B.exp(-(s * t / st) * (xa - xb) ** 2 / 2)
    return E * (B.sqrt(B.pi / (2 * st)) / w) * B.derf(al * (lo - c), al * (hi - c))


def leave_one_out(F):
    """F[..., l] -> (prod over all l, G[..., j] = prod over l != j), from prefix and suffix products: no division (the
    factors underflow to 0 for far pairs)"""
    d = F.shape[-1]
    pre = [None] * d
    run = F[..., 0] * 0 + 1
    for l in range(d):
        pre[l] = run
        run = run * F[..., l]
    out = [None] * d
    suf = F[..., 0] * 0 + 1
    for l in range(d - 1, -1, -1):
        out[l] = pre[l] * suf
        suf = suf * F[..., l]
    return run, np.stack(out, axis=-1)


def _abs(x):
    return x if x >= 0 else -x


class _Side:
    """everything about one model that involves no pair of design points"""

    def __init__(self, B, X, model, lo, hi, M):
        d = X.shape[1]
        self.A = B.arr(model["A"])[()]
        self.gamma = B.arr(model["gamma"])
        self.s = B.arr(model["s"])
        self.b0, self.c = _coef(B, model, d)
        self.IJ = point_integrals(B, X, self.s, lo, hi)
        self.P, self.Pex = leave_one_out(self.IJ[0])
        zero = lo * 0
        self.Eq = sum((cp * M[p + 1] for p, cp in enumerate(self.c)), zero)          # d
        self.S = self.b0 + self.Eq.sum()
        self.F = self.A * (self.gamma * self.P).sum()
        self.E0 = self.S + self.F


def _poly_kernel(B, a, b):
    """H[l] = E[q^a_l(x_l) f^b] = A_b sum_i gamma^b_i (sum_p beta^a_{p,l} J^{p,b}_l(i)) prod_{l' != l} I^b_l'(i)"""
    G = b.IJ[0] * 0
    for p, cp in enumerate(a.c):
        G = G + cp * b.IJ[p + 1]
    return b.A * (b.gamma[:, None] * G * b.Pex).sum(axis=0)


def covariances(B, X, ma, mb, lo, hi):
    """-> dict(e0 [2], cov_all, cov_first [d], cov_rest [d]) and the same keys with the scales, as float arrays.
    cov_first[j] = Cov(E[m^a | x_j], E[m^b | x_j]), cov_rest[j] = Cov(E[m^a | x_-j], E[m^b | x_-j])."""
    X, lo, hi = B.arr(X), B.arr(lo), B.arr(hi)
    N, d = X.shape
    M = moments(B, lo, hi)
    a, b = _Side(B, X, ma, lo, hi, M), _Side(B, X, mb, lo, hi, M)
    EQQ = lo * 0                                                # E[q^a_l q^b_l]
    for p, ca in enumerate(a.c):
        for q, cb in enumerate(b.c):
            EQQ = EQQ + ca * cb * M[p + q + 2]
    Hab, Hba = _poly_kernel(B, a, b), _poly_kernel(B, b, a)
    II = pair_integrals(B, X, a.s, b.s, lo, hi)                 # N x N x d
    IIall, IIex = leave_one_out(II)
    gg = a.gamma[:, None] * b.gamma[None, :]
    AA = a.A * b.A
    kk_all = AA * (gg * IIall).sum()
    kk_first = [AA * (gg * II[:, :, j] * a.Pex[:, None, j] * b.Pex[None, :, j]).sum() for j in range(d)]
    kk_rest = [AA * (gg * IIex[:, :, j] * a.IJ[0][:, None, j] * b.IJ[0][None, :, j]).sum() for j in range(d)]
    e00 = a.E0 * b.E0

    def assemble(inu, kk):
        """inu[l]: coordinate l belongs to u"""
        ua = sum((a.Eq[l] for l in range(d) if inu[l]), lo[0] * 0)
        ub = sum((b.Eq[l] for l in range(d) if inu[l]), lo[0] * 0)
        ca, cb = a.S - ua, b.S - ub                                # the constants: beta_0 + sum over l outside u of E q_l
        pp = ca * cb + ca * ub + cb * ua + ua * ub
        for l in range(d):
            if inu[l]:
                pp = pp + EQQ[l] - a.Eq[l] * b.Eq[l]
        pk = ca * b.F + cb * a.F
        for l in range(d):
            if inu[l]:
                pk = pk + Hab[l] + Hba[l]
        return pp + pk + kk - e00, _abs(pp) + _abs(pk) + _abs(kk) + _abs(e00)

    val, scl = {}, {}
    val["e0"], scl["e0"] = [a.E0, b.E0], [_abs(a.S) + _abs(a.F), _abs(b.S) + _abs(b.F)]
    val["cov_all"], scl["cov_all"] = assemble([True] * d, kk_all)
    fr = [assemble([l == j for l in range(d)], kk_first[j]) for j in range(d)]
    rs = [assemble([l != j for l in range(d)], kk_rest[j]) for j in range(d)]
    val["cov_first"], scl["cov_first"] = [v for v, _ in fr], [s for _, s in fr]
    val["cov_rest"], scl["cov_rest"] = [v for v, _ in rs], [s for _, s in rs]
    return ({k: B.tofloat(v) for k, v in val.items()}, {k: B.tofloat(v) for k, v in scl.items()})


def main_effects(B, X, model, lo, hi, grid):
    """grid[j][g]: values of x_j -> (dict(e0, main [d x G]), scales): main[j][g] = E[m | x_j = grid[j][g]]"""
    X, lo, hi, grid = B.arr(X), B.arr(lo), B.arr(hi), B.arr(grid)
    N, d = X.shape
    M = moments(B, lo, hi)
    a = _Side(B, X, model, lo, hi, M)
    val, scl = [], []
    for j in range(d):
        g = grid[j]
        q = g * 0
        for p, cp in enumerate(a.c):
            q = q + cp[j] * g ** (p + 1)
        const = a.S - a.Eq[j]
        k = B.exp(-a.s[j] * (g[None, :] - X[:, j, None]) ** 2 / 2)              # N x G
        kern = a.A * ((a.gamma * a.Pex[:, j])[:, None] * k).sum(axis=0)
        val.append(const + q + kern)
        scl.append(_abs(const) + np.abs(q) + np.abs(kern))
    return (dict(e0=B.tofloat(a.E0), main=B.tofloat(np.stack(val))),
            dict(e0=B.tofloat(_abs(a.S) + _abs(a.F)), main=B.tofloat(np.stack(scl))))


# ---------------------------------------------------------------------------------------------------- the function itself
def mean_function(X, model, Xq):
    """m at the rows of Xq, numpy fp64, no clamp"""
    X, Xq = np.asarray(X, float), np.asarray(Xq, float)
    d = X.shape[1]
    beta, s = np.asarray(model["beta"], float), np.asarray(model["s"], float)
    out = np.full(len(Xq), beta[0])
    for p in range(order_of(model, d)):
        out = out + (Xq ** (p + 1)) @ beta[1 + p * d:1 + (p + 1) * d]
    D2 = ((Xq[:, None, :] - X[None, :, :]) ** 2 * s).sum(axis=2)
    return out + model["A"] * np.exp(-D2 / 2) @ np.asarray(model["gamma"], float)


def quadrature(X, ma, mb, lo, hi, n=48):
    """the same dict as `covariances` returns first, by tensor Gauss-Legendre quadrature with n nodes per coordinate of m
    itself and of its conditional means: no closed form, d <= 3"""
    return quadrature_fn(lambda q: mean_function(X, ma, q), lambda q: mean_function(X, mb, q), lo, hi, n)


def quadrature_fn(fna, fnb, lo, hi, n=48):
    """`quadrature` for any two functions of the rows of a query matrix (a back-projected multi-output mean, say)"""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    d = len(lo)
    assert d <= 3
    t, wt = np.polynomial.legendre.leggauss(n)
    nodes = [lo[l] + (t + 1) * (hi[l] - lo[l]) / 2 for l in range(d)]
    mesh = np.stack([g.ravel() for g in np.meshgrid(*nodes, indexing="ij")], axis=1)
    W = wt / 2                                                  # the weights of a uniform density on one coordinate
    fa = fna(mesh).reshape((n,) * d)
    fb = fnb(mesh).reshape((n,) * d)

    def cond(f, keep):
        """E[f | x_keep] as an array over the kept axes"""
        for l in range(d - 1, -1, -1):
            if l not in keep:
                f = np.tensordot(f, W, axes=([l], [0]))
        return f

    def expect(f, naxes):
        for _ in range(naxes):
            f = np.tensordot(f, W, axes=([0], [0]))
        return float(f)

    e0a, e0b = expect(fa, d), expect(fb, d)

    def cov(keep):
        return expect((cond(fa, keep) - e0a) * (cond(fb, keep) - e0b), len(keep))

    every = list(range(d))
    return dict(e0=np.array([e0a, e0b]), cov_all=np.array(cov(every)),
                cov_first=np.array([cov([j]) for j in range(d)]),
                cov_rest=np.array([cov([l for l in every if l != j]) for j in range(d)]))


# ---------------------------------------------------------------------------------------------------- measures
KEYS = ("e0", "cov_all", "cov_first", "cov_rest")


def scaled_errors(got, ref, scale, keys=KEYS):
    """-> the largest |got - ref| / scale over every value of every key"""
    worst = 0.0
    for k in keys:
        g, r, s = (np.asarray(x[k], float).ravel() for x in (got, ref, scale))
        assert np.all(s > 0) or np.all(g[s == 0] == r[s == 0]), k
        worst = max(worst, float(np.max(np.abs(g - r)[s > 0] / s[s > 0], initial=0.0)))
    return worst


# ---------------------------------------------------------------------------------------------------- test inputs
def rng_model(seed, N, d, order, theta_len=None, amp=1.0):
    """a design on [0, 1)^d with random beta and gamma of mixed signs: -> (X, model)"""
    r = np.random.default_rng(seed)
    X = r.random((N, d))
    th = np.log(0.6) + 0.2 * r.standard_normal(d) if theta_len is None else np.asarray(theta_len, float)
    return X, dict(beta=r.standard_normal(1 + order * d), gamma=r.standard_normal(N) * 3.0, A=float(amp), s=np.exp(-2.0 * th))


def boxes(X):
    """the boxes of the tests by name: the design's own range, a narrow one inside it, one disjoint from the design in
    coordinate 0 (it starts six of the DEFAULT length scales, 6 * 0.6, above the largest x_0)"""
    lo, hi = X.min(axis=0), X.max(axis=0)
    if len(X) == 1:
        lo, hi = lo - 0.5, hi + 0.5
    mid, w = (lo + hi) / 2, hi - lo
    far_lo, far_hi = lo.copy(), hi.copy()
    far_lo[0], far_hi[0] = hi[0] + 3.6, hi[0] + 4.1
    return dict(design=(lo, hi), narrow=(mid - 0.01 * w, mid + 0.02 * w), disjoint=(far_lo, far_hi))


if __name__ == "__main__":
    import sys
    if "--measure" in sys.argv:
        import test_gpu_sens
        test_gpu_sens.measure_np_against_mp()
