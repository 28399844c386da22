"""tests/senspostref.py checks itself (CPU): the closed forms of the emulator-uncertainty terms S_u and of the main-effect band
in numpy fp64 against the same formulas in mpmath at 50 digits, and against Gauss-Legendre quadrature of the posterior
covariance c* itself, which uses no closed form at all.  (The figure the GPU tests take their bar from is measured over THEIR
cases by `python tests/senspostref.py --measure`; the cases here are small enough for every run.)

Settings: N <= 12, d in {1, 2, 3}, regression orders 0 .. 2, nugget 1e-3, P, G, Q from a numpy fit (`fit_state`), on the
design's own box and on a box disjoint from the design in coordinate 0.  Errors are relative to the SCALE senspostref returns
beside every value.

Bars.  As in test_sensref.py: every value is a sum of products of at most d + 2 factors good to a few ulp each, the J^p
recurrence amplifies rounding by up to 1 / (s_l w_l^2):
  NP_MP_BAR = 128 * 2^-52 * max(1, max_l 1 / (s_l w_l^2)).
Quadrature of c* on all pairs of 12^d nodes (24 nodes for the one-dimensional band) is converged far below that for these
smooth integrands; its bar is the larger of 1e-13 and NP_MP_BAR."""
import numpy as np
import pytest

import sensref as R
import senspostref as SP

EPS = 2.0 ** -52
NUGGET = 1e-3
CASES = [(1, 1, 0), (9, 1, 2), (12, 1, 1), (7, 2, 1), (10, 2, 0), (12, 2, 2), (8, 3, 0), (11, 3, 1), (12, 3, 2)]


def bar(m, lo, hi):
    return 128 * EPS * max(1.0, float(np.max(1.0 / (m["s"] * (hi - lo) ** 2))))


def fitted(N, d, order):
    X, m = R.rng_model(300 + 7 * N + d, N, d, order)
    y = np.random.default_rng(N + d).standard_normal(N)
    return (X, m) + SP.fit_state(X, y, order, m["A"], m["s"], NUGGET)


@pytest.mark.parametrize("box", ["design", "disjoint"])
@pytest.mark.parametrize("N,d,order", CASES)
def test_numpy_against_mpmath_and_quadrature(N, d, order, box):
    """(a) UU_l and every S_u against mpmath, (b) all 2 d + 2 subsets against quadrature of c* itself; the orderings"""
    X, m, P, G, Q, beta, gamma, _, _ = fitted(N, d, order)
    lo, hi = R.boxes(X)[box]
    val, scale = SP.post(R.NP, X, m, P, G, Q, lo, hi)
    mp, _ = SP.post(R.MP(), X, m, P, G, Q, lo, hi)
    B = R.MP()
    uu_mp = R.MP.tofloat(SP.uu(B, B.arr(m["s"]), B.arr(lo), B.arr(hi)))
    e_uu = float(np.max(np.abs(SP.uu(R.NP, m["s"], lo, hi) - uu_mp) / uu_mp))
    quad = SP.quadrature_post(X, m, P, G, Q, lo, hi)
    e_mp, e_q = SP.scaled_errors(val, mp, scale), SP.scaled_errors(val, quad, scale)
    b = bar(m, lo, hi)
    print(f"N {N} d {d} order {order} {box}: numpy - mpmath {e_mp:.2e}, UU {e_uu:.2e} (bar {b:.1e}), numpy - quadrature {e_q:.2e}")
    assert e_mp < b and e_uu < b
    assert e_q < max(1e-13, b)
    for k in ("s_first", "s_rest"):
        slack = b * (scale[k] + scale["s_all"] + scale["s_none"])
        assert np.all(val["s_none"] <= val[k] + slack) and np.all(val[k] <= val["s_all"] + slack)
    assert val["s_none"] >= -b * scale["s_none"]
    if d == 1:
        assert abs(val["s_first"][0] - val["s_all"]) <= 2 * b * scale["s_all"] and abs(val["s_rest"][0] - val["s_none"]) <= 2 * b * scale["s_none"]


@pytest.mark.parametrize("N,d,order", [(9, 1, 2), (7, 2, 1), (12, 2, 2)])
def test_band(N, d, order):
    """(c) the band against one-dimensional quadrature of c* (and mpmath), its average over x_j against S_{j}, its curve
    against sensref's main effects, Var*[E0] against S_none"""
    X, m, P, G, Q, beta, gamma, _, _ = fitted(N, d, order)
    lo, hi = R.boxes(X)["design"]
    b = bar(m, lo, hi)
    grid = np.stack([np.array([lo[l], hi[l], X[N // 2, l], lo[l] + 0.3 * (hi[l] - lo[l])]) for l in range(d)])
    val, scale = SP.band(R.NP, X, m, P, G, Q, beta, gamma, lo, hi, grid)
    mp, _ = SP.band(R.MP(), X, m, P, G, Q, beta, gamma, lo, hi, grid)
    assert SP.scaled_errors(val, mp, scale, keys=("var", "var_e0", "main")) < b
    quad = SP.quadrature_band(X, m, P, G, Q, lo, hi, grid)
    assert np.max(np.abs(val["var"] - quad) / scale["var"]) < max(1e-13, b)
    main = R.main_effects(R.NP, X, dict(m, beta=beta, gamma=gamma), lo, hi, grid)[0]["main"]
    assert np.max(np.abs(val["main"] - main) / scale["main"]) < b
    post, pscale = SP.post(R.NP, X, m, P, G, Q, lo, hi)
    assert abs(val["var_e0"] - post["s_none"]) < b * (scale["var_e0"] + pscale["s_none"])
    nodes = [SP.gauss_nodes(lo[l], hi[l]) for l in range(d)]
    over = SP.band(R.NP, X, m, P, G, Q, beta, gamma, lo, hi, np.stack([n for n, _ in nodes]))[0]["var"]
    for j in range(d):
        assert abs(nodes[j][1] @ over[j] - post["s_first"][j]) < max(1e-13, b) * pscale["s_first"][j]


def test_two_routes_in_numpy():
    """the closed form on P, G, Q from numpy's inverse against the Cholesky route that never forms C^-1 (what the GPU tests
    compare on the device): the band's average and the average prediction variance"""
    import test_gpu_sens_post as T
    X = np.random.default_rng(5).random((40, 2))
    e = T.routes_numpy(X, T.thetas(2), 1, *R.boxes(X)["design"])
    print("routes:", e)
    assert max(e) < 1e-13
