"""tests/sensmeasureref.py checks itself (CPU): the closed forms under Gaussian and mixed input measures in numpy fp64 against
the same formulas in mpmath at 50 digits and against tensor quadrature of the functions themselves (Gauss-Hermite nodes on a
Gaussian coordinate, Gauss-Legendre nodes on a uniform one), which uses no closed form at all.

Settings: N <= 40 for the posterior mean and N <= 12 for the posterior covariance, d in {1, 2, 3}, regression orders 0 .. 3, one
model and the cross case, every coordinate Gaussian and alternating kinds.  A Gaussian coordinate has its mean at 0.4 + 0.1 l
and sd 0.25 (0.15 for the posterior covariance, whose quadrature runs over all PAIRS of nodes and affords fewer of them); a
uniform one the design's range.  Errors are relative to the SCALE the references return beside every value.

Bars.  As in test_sensref.py: every value is a sum of products of at most d + 2 factors good to a few ulp each; a uniform
coordinate's J^p recurrence amplifies rounding by up to 1 / (s_l w_l^2), a Gaussian coordinate's tables have no such step:
  NP_MP_BAR = 128 * 2^-52 * max(1, max over the uniform l of 1 / (s_l w_l^2)).
Quadrature: Gauss-Legendre with 40 nodes is converged far below that (test_sensref.py).  Gauss-Hermite converges geometrically
for these integrands (sums of Gaussians in the standardised variable, of width 1 / sqrt(s sd^2) >= 1.4 nodes' units); its own
remainder is measured as the difference between n and n - 8 nodes (n - 2 for the pairs of nodes) and bounds the error at n from
above, so the bar is the largest of 1e-13, NP_MP_BAR and that remainder -- which is itself asserted small (1e-12, and 1e-8
where only 12 nodes per coordinate fit), so that the comparison keeps its teeth."""
import numpy as np
import pytest

import sensref as R
import sensmeasureref as M
import senspairref as SQ
import senspostref as SP

EPS = 2.0 ** -52
NUGGET = 1e-3
CASES = [(1, 1, 0), (20, 1, 2), (40, 1, 3), (33, 2, 0), (30, 2, 1), (17, 2, 3), (25, 3, 1), (30, 3, 2), (12, 3, 3)]
POST_CASES = [(1, 1, 0), (9, 1, 2), (7, 2, 1), (12, 2, 2), (8, 3, 0), (11, 3, 1)]
PLUG_KEYS = R.KEYS + ("main",)


def kinds(name, d):
    return np.ones(d, dtype=int) if name == "gauss" else (np.arange(d) + 1) % 2      # mixed: Gaussian, uniform, Gaussian


def measure_of(kind, X, sd):
    lo, hi = R.boxes(X)["design"]
    g = np.asarray(kind) == M.GAUSS
    return np.where(g, 0.4 + 0.1 * np.arange(len(lo)), lo), np.where(g, sd, hi)


def bar(kind, s, lo, hi):
    u = np.asarray(kind) == M.UNIFORM
    return 128 * EPS * max(1.0, float(np.max(1.0 / (s[u] * (hi[u] - lo[u]) ** 2), initial=0.0)))


def with_pairs(val, scale, pv, ps):
    val, scale = dict(val), dict(scale)
    val["cov_pair"], scale["cov_pair"] = pv["cov_pair"], ps["cov_pair"]
    return val, scale


def plug(B, kind, X, ma, mb, lo, hi, grid):
    val, scale = M.covariances(kind, B, X, ma, mb, lo, hi)
    mv, ms = M.main_effects(kind, B, X, ma, lo, hi, grid)
    val["main"], scale["main"] = mv["main"], ms["main"]
    keys = PLUG_KEYS
    if X.shape[1] >= 2:
        val, scale = with_pairs(val, scale, *M.pair_covariances(kind, B, X, ma, mb, lo, hi))
        keys = keys + ("cov_pair",)
    return val, scale, keys


@pytest.mark.parametrize("measure", ["gauss", "mixed"])
@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("N,d,order", CASES)
def test_posterior_mean_against_mpmath_and_quadrature(N, d, order, cross, measure):
    """E0, V, V_j, VT_j (through cov_rest), V_jk and a main effect: numpy against mpmath, and against quadrature of m itself"""
    X, ma = R.rng_model(100 + N, N, d, order)
    mb = R.rng_model(200 + N, N, d, order)[1] if cross else ma
    kind = kinds(measure, d)
    lo, hi = measure_of(kind, X, 0.25)
    grid = np.stack([np.array([0.1, 0.45, 0.9, X[N // 2, l]]) for l in range(d)])
    val, scale, keys = plug(R.NP, kind, X, ma, mb, lo, hi, grid)
    mp, _, _ = plug(R.MP(), kind, X, ma, mb, lo, hi, grid)
    quad, coarse = (M.quadrature(kind, X, ma, mb, lo, hi, n=n, grid=grid) for n in (40, 32))
    b = bar(kind, np.minimum(ma["s"], mb["s"]), lo, hi)
    e_mp, e_q, rem = M.scaled_errors(val, mp, scale, keys), M.scaled_errors(val, quad, scale, keys), M.scaled_errors(coarse, quad, scale, keys)
    print(f"N {N} d {d} order {order} cross {cross} {measure}: numpy - mpmath {e_mp:.2e} (bar {b:.1e}), numpy - quadrature {e_q:.2e}, "
          f"quadrature 40 against 32 nodes {rem:.2e}")
    assert e_mp < b
    assert rem < 1e-12 and e_q < max(1e-13, b, rem)
    if not cross:
        V, slack = val["cov_all"], b * scale["cov_all"]
        assert V >= -slack
        for j in range(d):
            Vj, VTj = val["cov_first"][j], V - val["cov_rest"][j]
            assert -slack <= Vj <= VTj + 2 * slack and VTj <= V + 2 * slack
        for p, (j, k) in enumerate(SQ.pairs(d)):
            assert val["cov_pair"][p] - val["cov_first"][j] - val["cov_first"][k] >= -3 * slack and val["cov_pair"][p] <= V + 2 * slack
        if d == 1:
            assert abs(val["cov_first"][0] - V) <= 2 * slack and abs(val["cov_rest"][0]) <= 2 * slack


@pytest.mark.parametrize("measure", ["gauss", "mixed"])
@pytest.mark.parametrize("N,d,order", POST_CASES)
def test_posterior_covariance_against_mpmath_and_quadrature(N, d, order, measure):
    """s_none, s_all, s_first, s_rest, s_pair and UU: numpy against mpmath, and against quadrature of c* on all pairs of nodes"""
    X, m = R.rng_model(300 + 7 * N + d, N, d, order)
    y = np.random.default_rng(N + d).standard_normal(N)
    P, G, Q = SP.fit_state(X, y, order, m["A"], m["s"], NUGGET)[:3]
    kind = kinds(measure, d)
    lo, hi = measure_of(kind, X, 0.15)
    keys = SP.KEYS + (("s_pair",) if d >= 2 else ())

    def both(B):
        val, scale = M.post(kind, B, X, m, P, G, Q, lo, hi)
        if d >= 2:
            pv, ps = M.pair_post(kind, B, X, m, P, G, Q, lo, hi)
            val["s_pair"], scale["s_pair"] = pv["s_pair"], ps["s_pair"]
        return val, scale

    val, scale = both(R.NP)
    mp, _ = both(R.MP())
    n = 12 if d == 3 else 20
    quad, coarse = (M.quadrature_post(kind, X, m, P, G, Q, lo, hi, n=k) for k in (n, n - 2))
    b = bar(kind, m["s"], lo, hi)
    e_mp, e_q, rem = M.scaled_errors(val, mp, scale, keys), M.scaled_errors(val, quad, scale, keys), M.scaled_errors(coarse, quad, scale, keys)
    print(f"N {N} d {d} order {order} {measure}: numpy - mpmath {e_mp:.2e} (bar {b:.1e}), numpy - quadrature {e_q:.2e}, "
          f"quadrature {n} against {n - 2} nodes {rem:.2e}")
    assert e_mp < b
    assert rem < (1e-8 if d == 3 else 1e-12) and e_q < max(1e-13, b, rem)
    # s_none <= s_first <= s_pair <= s_all, s_none <= s_rest <= s_all
    for k in ("s_first", "s_rest"):
        slack = b * (scale[k] + scale["s_all"] + scale["s_none"])
        assert np.all(val["s_none"] <= val[k] + slack) and np.all(val[k] <= val["s_all"] + slack)
    for p, (j, k) in enumerate(SQ.pairs(d)):
        slack = b * (scale["s_pair"][p] + scale["s_all"] + scale["s_first"][j] + scale["s_first"][k])
        assert max(val["s_first"][j], val["s_first"][k]) <= val["s_pair"][p] + slack and val["s_pair"][p] <= val["s_all"] + slack
    assert val["s_none"] >= -b * scale["s_none"]


def test_the_five_forms_against_one_dimensional_quadrature():
    """I, J^1..J^3, II, E x^n and UU of one Gaussian coordinate against Gauss-Hermite quadrature with 80 nodes"""
    mu, sd, s, t = np.array([0.3]), np.array([0.7]), np.array([2.5]), np.array([1.1])
    X = np.array([[-0.4], [0.2], [1.3]])
    (x, w), = M.nodes_weights([M.GAUSS], mu, sd, 80)
    ka = np.exp(-s[0] * (X[:, 0, None] - x[None, :]) ** 2 / 2)
    kb = np.exp(-t[0] * (X[:, 0, None] - x[None, :]) ** 2 / 2)
    IJ = M.gauss_point_integrals(R.NP, X, s, mu, sd)
    for p in range(4):
        assert np.max(np.abs(IJ[p][:, 0] - (ka * x ** p) @ w)) < 1e-14
    II = M.gauss_pair_integrals(R.NP, X, s, t, mu, sd)[:, :, 0]
    assert np.max(np.abs(II - (ka * w) @ kb.T)) < 1e-14
    mom = M.gauss_moments(R.NP, mu, sd)
    for n in range(7):
        assert abs(mom[n][0] - (x ** n) @ w) < 1e-13 * max(1.0, abs(mom[n][0]))
    uu = w @ np.exp(-s[0] * (x[:, None] - x[None, :]) ** 2 / 2) @ w
    assert abs(M.gauss_uu(R.NP, s, mu, sd)[0] - uu) < 1e-14


def test_exactly_linear_function():
    """m(x) = 2 + 3 x_0 - x_1 (gamma = 0), x_0 ~ N(0.4, 0.2^2), x_1 uniform, x_2 ~ N(1, 3^2): V_j = beta_j^2 sd_j^2 on a
    Gaussian coordinate, beta_j^2 w_j^2 / 12 on the uniform one, total = first, E0 = m(the means)"""
    X, _ = R.rng_model(3, 30, 3, 1)
    m = dict(beta=np.array([2.0, 3.0, -1.0, 0.0]), gamma=np.zeros(30), A=1.0, s=np.full(3, 2.0))
    kind = [1, 0, 1]
    lo, hi = np.array([0.4, -1.0, 1.0]), np.array([0.2, 2.0, 3.0])
    val, scale = M.covariances(kind, R.NP, X, m, m, lo, hi)
    want = np.array([9.0 * 0.2 ** 2, 3.0 ** 2 / 12, 0.0])
    assert abs(val["e0"][0] - (2 + 3 * 0.4 - 0.5)) < 8 * EPS * scale["e0"][0]
    assert np.all(np.abs(val["cov_first"] - want) < 64 * EPS * scale["cov_first"])
    assert np.all(np.abs(val["cov_all"] - val["cov_rest"] - want) < 64 * EPS * scale["cov_rest"])
    assert abs(val["cov_all"] - want.sum()) < 64 * EPS * scale["cov_all"]
    pv, ps = M.pair_covariances(kind, R.NP, X, m, m, lo, hi)
    assert np.all(np.abs(pv["cov_pair"] - [want[0] + want[1], want[0] + want[2], want[1] + want[2]]) < 64 * EPS * ps["cov_pair"])


def test_all_uniform_kinds_reproduce_the_three_references_bit_for_bit():
    N, d, order = 25, 3, 2
    X, ma = R.rng_model(11, N, d, order)
    mb = R.rng_model(12, N, d, order)[1]
    y = np.random.default_rng(4).standard_normal(N)
    P, G, Q, beta, gamma, _, _ = SP.fit_state(X, y, order, ma["A"], ma["s"], NUGGET)
    lo, hi = R.boxes(X)["narrow"]
    grid = np.stack([np.linspace(lo[l], hi[l], 4) for l in range(d)])
    kind = np.zeros(d, dtype=int)

    def same(a, b):
        return all(np.array_equal(p[k], q[k]) for p, q in zip(a, b) for k in p)

    assert same(M.covariances(kind, R.NP, X, ma, mb, lo, hi), R.covariances(R.NP, X, ma, mb, lo, hi))
    assert same(M.main_effects(kind, R.NP, X, ma, lo, hi, grid), R.main_effects(R.NP, X, ma, lo, hi, grid))
    assert same(M.post(kind, R.NP, X, ma, P, G, Q, lo, hi), SP.post(R.NP, X, ma, P, G, Q, lo, hi))
    assert same(M.band(kind, R.NP, X, ma, P, G, Q, beta, gamma, lo, hi, grid), SP.band(R.NP, X, ma, P, G, Q, beta, gamma, lo, hi, grid))
    assert same(M.pair_covariances(kind, R.NP, X, ma, mb, lo, hi), SQ.pair_covariances(R.NP, X, ma, mb, lo, hi))
    assert same(M.pair_post(kind, R.NP, X, ma, P, G, Q, lo, hi), SQ.pair_post(R.NP, X, ma, P, G, Q, lo, hi))
    xj, xk = grid[0], grid[2]
    assert same(M.joint_surface(kind, R.NP, X, ma, lo, hi, 0, 2, xj, xk), SQ.joint_surface(R.NP, X, ma, lo, hi, 0, 2, xj, xk))
    # and the swap does not outlive the call: the references themselves still give the box's numbers
    with M.measure([1, 1, 1]):
        inside = R.covariances(R.NP, X, ma, mb, lo, hi)[0]["cov_all"]
    assert inside != R.covariances(R.NP, X, ma, mb, lo, hi)[0]["cov_all"]
    assert R.moments is M._ORIG["moments"] and SP.uu is M._ORIG["uu"]


def test_monte_carlo_sample_of_the_measure():
    """`sample` draws what `nodes_weights` integrates: means and variances per coordinate"""
    kind, lo, hi = [1, 0], np.array([0.3, -1.0]), np.array([0.5, 2.0])
    x = M.sample(kind, lo, hi, np.random.default_rng(1), 1 << 16)
    assert abs(x[:, 0].mean() - 0.3) < 5 * 0.5 / 256 and abs(x[:, 0].var() - 0.25) < 0.01
    assert x[:, 1].min() >= -1.0 and x[:, 1].max() <= 2.0 and abs(x[:, 1].mean() - 0.5) < 5 * 3 / np.sqrt(12) / 256
