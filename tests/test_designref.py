"""tests/designref.py checks itself (CPU): the closed form of the expected IMSE reduction in numpy fp64, pinned
three ways -- against the same Gram form in mpmath at 50 digits, against tensor quadrature of senspostref.cstar(...)^2 (which
uses no closed form), and against the identity it stands for: s_all of the design minus s_all of the design with the candidate
appended, both by senspostref.post on a fit of their own.  (The figures the GPU tests take their bars from are measured over
THEIR cases by `python tests/designref.py --measure`; the cases here are small enough for every run.)

Settings: N <= 12, d in {1, 2, 3}, regression orders 0 .. 2, nugget 1e-3, a, b and v from a numpy fit (`fit_ab`), uniform on the
design's own box and on a box disjoint from the design, all-Gaussian and mixed measures; candidates inside and outside the box
and one on a design point.  Errors HERE are relative to the sum of the absolute values of the TERMS inside the six parts of num
(designref's num_terms / gain_terms): that sum is what bounds the rounding error of an fp64 evaluation, and these random models
cancel heavily inside a^T K a (at N = 12, d = 2, order 2 the six parts' own sum is 1300 times smaller, up to 2150 times over the cases).  The GPU tests use the six
parts' sum, as their issue defines it, with bars measured on it.

The quadrature is taken on the design's box and under the Gaussian and mixed measures, not on the disjoint box (see the test).

Bars.  As in test_senspostref.py, NP_MP_BAR = 128 * 2^-52 * max(1, max_l 1 / (s_l w_l^2)) for numpy against mpmath (every part
is a sum of products of at most d + 2 factors good to a few ulp each).  Quadrature (24 Gauss-Legendre or Gauss-Hermite nodes
per coordinate) is converged far below that for these smooth integrands; its bar is the larger of 1e-13 and NP_MP_BAR.  The
refit identity compares two values of s_all, each good to NP_MP_BAR of its own scale (which holds A^2 sum |P_ii'| KK, entries of
size 1 / nugget): its bar is NP_MP_BAR of the sum of the two scales and the gain's, times 8 for the two fits' inverses."""
import numpy as np
import pytest

import designref as D
import sensref as R
import sensmeasureref as SM
import senspostref as SP

EPS = 2.0 ** -52
NUGGET = 1e-3
CASES = [(1, 1, 0), (9, 1, 2), (12, 1, 1), (7, 2, 1), (10, 2, 0), (12, 2, 2), (8, 3, 0), (11, 3, 1), (12, 3, 2)]


def bar(m, w):
    return 128 * EPS * max(1.0, float(np.max(1.0 / (m["s"] * w ** 2))))


def setting(N, d, order, measure):
    """-> (X, model, kind, lo, hi, w, Xq): w the widths the bar is taken from (the box, or the standard deviations)"""
    X, m = R.rng_model(300 + 7 * N + d, N, d, order)
    blo, bhi = R.boxes(X)["disjoint" if measure == "disjoint" else "design"]
    if measure in ("design", "disjoint"):
        kind, lo, hi, w = np.zeros(d, dtype=int), blo, bhi, bhi - blo
    else:
        kind = np.ones(d, dtype=int) if measure == "gauss" else (np.arange(d) % 2 == 0).astype(int)
        g = kind == SM.GAUSS
        lo, hi = np.where(g, (blo + bhi) / 2, blo), np.where(g, 0.3 * (bhi - blo), bhi)
        w = np.where(g, hi, hi - lo)
    r = np.random.default_rng(77 + N + d)
    slo, shi = X.min(axis=0) - 0.5, X.max(axis=0) + 0.5
    Xq = np.vstack([slo + (shi - slo) * r.random((5, d)), X[N // 2][None, :]])          # inside, outside, on a design point
    return X, m, kind, lo, hi, w, Xq


@pytest.mark.parametrize("measure", ["design", "disjoint", "gauss", "mixed"])
@pytest.mark.parametrize("N,d,order", CASES)
def test_numpy_against_mpmath_and_quadrature(N, d, order, measure):
    X, m, kind, lo, hi, w, Xq = setting(N, d, order, measure)
    a, b, v, _ = D.fit_ab(X, order, m["A"], m["s"], NUGGET, Xq)
    val, scale, parts = D.gain(R.NP, X, m, lo, hi, kind, Xq, a, b, v)
    mp, _, _ = D.gain(R.MP(), X, m, lo, hi, kind, Xq, a, b, v)
    terms = dict(num=scale["num_terms"], gain=scale["gain_terms"])
    e_mp = D.scaled_errors(val, mp, terms)
    # (the disjoint box is compared with mpmath alone: six length scales from the design senspostref.cstar, which the quadrature
    # squares, is itself a difference of polynomial terms in fp64 that are orders of magnitude larger than c*)
    quad = D.quadrature(X, m, order, NUGGET, lo, hi, kind, Xq) if measure != "disjoint" else val["num"]
    e_q = float(np.max(np.abs(val["num"] - quad) / terms["num"]))
    t = bar(m, w)
    print(f"N {N} d {d} order {order} {measure}: numpy - mpmath {e_mp:.2e} (bar {t:.1e}), numpy - quadrature {e_q:.2e}")
    assert np.allclose(parts.sum(axis=1), val["num"], rtol=0, atol=64 * EPS * terms["num"].max())
    assert e_mp < t
    assert e_q < max(1e-13, t)
    assert np.all(v > 0) and np.all(val["gain"] >= -t * terms["gain"])


@pytest.mark.parametrize("measure", ["design", "gauss", "mixed"])
@pytest.mark.parametrize("N,d,order", [(9, 1, 2), (7, 2, 1), (12, 2, 2), (11, 3, 1)])
def test_refit_identity(N, d, order, measure):
    """gain = s_all(design) - s_all(design + {x*}), and 0 <= gain <= s_all; a run on a design point gains least"""
    X, m, kind, lo, hi, w, Xq = setting(N, d, order, measure)
    a, b, v, (P, G, Q) = D.fit_ab(X, order, m["A"], m["s"], NUGGET, Xq)
    val, scale, _ = D.gain(R.NP, X, m, lo, hi, kind, Xq, a, b, v)
    diff, dscale = D.refit(X, m, order, NUGGET, lo, hi, kind, Xq)
    gap = float(np.max(np.abs(val["gain"] - diff) / (dscale + scale["gain_terms"])))
    t = 8 * bar(m, w)
    print(f"N {N} d {d} order {order} {measure}: refit gap {gap:.2e} (bar {t:.1e}); relative to the gain {np.max(np.abs(val['gain'] - diff) / val['gain']):.2e}")
    assert gap < t
    s_all, s_scale = (x["s_all"] for x in SM.post(kind, R.NP, X, m, P, G, Q, lo, hi))
    assert np.all(val["gain"] <= s_all + t * (s_scale + scale["gain_terms"]))
    inside = np.all((Xq[:-1] >= X.min(axis=0)) & (Xq[:-1] <= X.max(axis=0)), axis=1)      # (far outside a run gains next to nothing too)
    assert np.all(val["gain"][-1] < val["gain"][:-1][inside])


def test_two_routes_to_a_and_b_in_numpy():
    """a, b and v from numpy's inverse against the Cholesky route (what the GPU tests compare on the device)"""
    X, m = R.rng_model(5, 40, 2, 1)
    Xq = np.random.default_rng(6).random((7, 2))
    a, b, v, (P, G, Q) = D.fit_ab(X, 1, m["A"], m["s"], NUGGET, Xq)
    a2, b2, v2 = D.chol_ab(X, 1, m["A"], m["s"], NUGGET, Xq)
    sa, sb = D.ab_scales(X, 1, m["A"], m["s"], Xq, SP.fit_state(X, np.zeros(40), 1, m["A"], m["s"], NUGGET)[5])
    e = max(float(np.max(np.abs(a - a2) / sa)), float(np.max(np.abs(b - b2) / sb)))
    print("routes:", e, float(np.max(np.abs(v - v2))))
    assert e < 1e-11 and np.allclose(v, v2, rtol=1e-8, atol=0)


def test_where_a_repeated_design_point_gains_least():
    """the two cases behind tests/test_gpu_design.py::test_a_design_point_gains_least, in numpy: on its sparse design (65 points,
    d = 8) a repeated design point gains far less than every other candidate; on a dense one (130 points, d = 3: the emulator is
    sure everywhere) some candidate gains LESS than the repeat, so the property is no theorem and the GPU test names its case"""
    import test_gpu_design as T
    out = {}
    for N, d in ((65, 8), (130, 3)):
        name, X, y, th, o, kind, lo, hi, _ = T.case_of(N, d, 1, 64)
        Xq = np.vstack([T.far_candidates(X, th, 64, 5), X[17][None, :]])
        m = T.TP.model_of(th)
        a, b, v, _ = D.fit_ab(X, o, m["A"], m["s"], T.NUGGET, Xq)
        g = D.gain(R.NP, X, m, lo, hi, kind, Xq, a, b, v)[0]["gain"]
        out[N] = (g[-1], g[:-1].min())
        print(f"N {N} d {d}: the repeated design point gains {g[-1]:.3e}, the least of the other candidates {g[:-1].min():.3e}")
    assert out[65][0] < 0.1 * out[65][1]
    assert out[130][0] > out[130][1]
