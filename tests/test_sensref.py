"""tests/sensref.py checks itself (CPU): the closed forms in numpy fp64 against the same formulas in mpmath at 50 digits and
against tensor Gauss-Legendre quadrature of the function itself, which uses no closed form at all.

Settings: N <= 65, d in {1, 2, 3}, regression orders 0 .. 3, one model and the cross case (two sets of lengths, weights and
coefficients on one design), on the design's own box and on a box disjoint from the design in coordinate 0 by six length
scales.  Errors are relative to the SCALE sensref returns beside every value.

Bars.  Every value is a sum of products of at most d + 2 <= 5 factors, each an erf / erfc difference, an exp or a square root
good to a few ulp, so about 20 ulp per product; J^p comes from a three-step recurrence whose steps divide a difference of
nearly equal numbers by s_l, which amplifies their rounding by up to 1 / (s_l w_l^2) (w_l the box width).  With a factor two:
  NP_MP_BAR = 128 * 2^-52 * max(1, max_l 1 / (s_l w_l^2)).
Quadrature with 48 nodes per coordinate is converged far below that for these smooth integrands (the issue's own check
reached 1e-13); its bar is the larger of 1e-13 and NP_MP_BAR."""
import numpy as np
import pytest

import sensref as R

EPS = 2.0 ** -52
CASES = [(1, 1, 0), (20, 1, 2), (65, 1, 3), (33, 2, 0), (40, 2, 1), (17, 2, 3), (25, 3, 1), (30, 3, 2), (12, 3, 3)]


def bar(ma, mb, lo, hi):
    sw2 = np.minimum(ma["s"], mb["s"]) * (hi - lo) ** 2
    return 128 * EPS * max(1.0, float(np.max(1.0 / sw2)))


def models(N, d, order, cross):
    X, ma = R.rng_model(100 + N, N, d, order)
    mb = R.rng_model(200 + N, N, d, order)[1] if cross else ma
    return X, ma, mb


@pytest.mark.parametrize("box", ["design", "disjoint"])
@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("N,d,order", CASES)
def test_numpy_against_mpmath_and_quadrature(N, d, order, cross, box):
    X, ma, mb = models(N, d, order, cross)
    lo, hi = R.boxes(X)[box]
    if box == "disjoint":
        assert lo[0] - X[:, 0].max() >= 6 * 0.6 - 1e-12
    val, scale = R.covariances(R.NP, X, ma, mb, lo, hi)
    mp, _ = R.covariances(R.MP(), X, ma, mb, lo, hi)
    quad = R.quadrature(X, ma, mb, lo, hi)
    e_mp, e_q = R.scaled_errors(val, mp, scale), R.scaled_errors(val, quad, scale)
    b = bar(ma, mb, lo, hi)
    print(f"N {N} d {d} order {order} cross {cross} {box}: numpy - mpmath {e_mp:.2e} (bar {b:.1e}), numpy - quadrature {e_q:.2e}")
    assert e_mp < b
    assert e_q < max(1e-13, b)
    if not cross:
        # one model: a variance, its first-order part and its total-effect part, ordered up to the bar
        V, slack = val["cov_all"], b * scale["cov_all"]
        assert V >= -slack
        for j in range(d):
            Vj, VTj = val["cov_first"][j], V - val["cov_rest"][j]
            assert -slack <= Vj <= VTj + 2 * slack and VTj <= V + 2 * slack
        if d == 1:
            assert abs(val["cov_first"][0] - V) <= 2 * slack and abs(val["cov_rest"][0]) <= 2 * slack


@pytest.mark.parametrize("N,d,order", [(20, 1, 2), (33, 2, 1), (25, 3, 3)])
def test_main_effects(N, d, order):
    X, ma, _ = models(N, d, order, False)
    lo, hi = R.boxes(X)["design"]
    grid = np.linspace(lo, hi, 7).T
    val, scale = R.main_effects(R.NP, X, ma, lo, hi, grid)
    mp, _ = R.main_effects(R.MP(), X, ma, lo, hi, grid)
    b = bar(ma, ma, lo, hi)
    assert R.scaled_errors(val, mp, scale, keys=("e0", "main")) < b
    # the curve against quadrature of m over the other coordinates, and its own mean and variance against the indices
    t, wt = np.polynomial.legendre.leggauss(48)
    cov, _ = R.covariances(R.NP, X, ma, ma, lo, hi)
    for j in range(d):
        fine = lo[j] + (t + 1) * (hi[j] - lo[j]) / 2
        g = np.tile(fine, (d, 1))
        curve = R.main_effects(R.NP, X, ma, lo, hi, g)[0]["main"][j]
        assert abs(curve @ wt / 2 - cov["e0"][0]) < 1e-12 * scale["e0"]
        assert abs(((curve - cov["e0"][0]) ** 2) @ wt / 2 - cov["cov_first"][j]) < 1e-12 * np.asarray(_first_scale(X, ma, lo, hi))[j]


def _first_scale(X, ma, lo, hi):
    return R.covariances(R.NP, X, ma, ma, lo, hi)[1]["cov_first"]


def test_erfc_form_is_needed():
    """order 0 with beta_0 = 0 on the disjoint box: every value is made of kernel integrals that lie six length scales and
    more from the design.  The erfc form meets the bar; the plain erf difference misses it by orders of magnitude."""
    X, ma = R.rng_model(7, 40, 2, 0)
    ma["beta"] = np.zeros(1)
    lo, hi = R.boxes(X)["disjoint"]
    mp, _ = R.covariances(R.MP(), X, ma, ma, lo, hi)
    val, scale = R.covariances(R.NP, X, ma, ma, lo, hi)
    naive, _ = R.covariances(R.NPNaive, X, ma, ma, lo, hi)
    b = bar(ma, ma, lo, hi)
    e, en = R.scaled_errors(val, mp, scale), R.scaled_errors(naive, mp, scale)
    print(f"erfc form {e:.2e}, plain erf difference {en:.2e}, bar {b:.1e}")
    assert e < b and en > 100 * b


def test_exactly_linear_function():
    """m(x) = 2 + 3 x_0 - x_1 (gamma = 0): V_j = beta_j^2 w_j^2 / 12, total = first, E0 = m(centre)"""
    X, _ = R.rng_model(3, 30, 3, 1)
    m = dict(beta=np.array([2.0, 3.0, -1.0, 0.0]), gamma=np.zeros(30), A=1.0, s=np.full(3, 2.0))
    lo, hi = np.array([0.1, -1.0, 0.0]), np.array([0.7, 2.0, 5.0])
    val, scale = R.covariances(R.NP, X, m, m, lo, hi)
    w = hi - lo
    want = np.array([9.0, 1.0, 0.0]) * w ** 2 / 12
    assert abs(val["e0"][0] - (2 + 3 * 0.4 - 0.5)) < 8 * EPS * scale["e0"][0]
    assert np.all(np.abs(val["cov_first"] - want) < 64 * EPS * scale["cov_first"])
    assert np.all(np.abs(val["cov_all"] - val["cov_rest"] - want) < 64 * EPS * scale["cov_rest"])
    assert abs(val["cov_all"] - want.sum()) < 64 * EPS * scale["cov_all"]
