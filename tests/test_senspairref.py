"""tests/senspairref.py checks itself (CPU): the second-order closed forms in numpy fp64 against the same formulas in mpmath
at 50 digits and against tensor Gauss-Legendre quadrature of the function (or of the posterior covariance) itself, which uses
no closed form; the structural identities against sensref.py and senspostref.py.

Bars, as in test_sensref.py and for its reasons:  NP_MP_BAR = 128 * 2^-52 * max(1, max_l 1 / (s_l w_l^2))  against mpmath, the
larger of 1e-13 and NP_MP_BAR against quadrature (the prototype of these formulas measured at most 5.4e-15 on the three
cases of CASES, and 2.5e-16 on the two identities)."""
import numpy as np
import pytest

import sensref as R
import senspairref as SPR
import senspostref as SP

EPS = 2.0 ** -52
NUGGET = 1e-3
CASES = [(4, 40, 2, 20), (3, 65, 1, 32), (2, 30, 3, 40)]         # d, N, order, quadrature nodes per coordinate
POST_CASES = [(7, 2, 1), (10, 2, 0), (12, 2, 2), (8, 3, 0), (11, 3, 1), (12, 3, 2)]     # N, d, order


def bar(ma, mb, lo, hi):
    sw2 = np.minimum(ma["s"], mb["s"]) * (hi - lo) ** 2
    return 128 * EPS * max(1.0, float(np.max(1.0 / sw2)))


def models(N, d, order, cross):
    X, ma = R.rng_model(100 + N, N, d, order)
    mb = R.rng_model(200 + N, N, d, order)[1] if cross else ma
    return X, ma, mb


@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("d,N,order,nodes", CASES)
def test_pairs_against_mpmath_and_quadrature(d, N, order, nodes, cross):
    X, ma, mb = models(N, d, order, cross)
    lo, hi = R.boxes(X)["design"]
    val, scale = SPR.pair_covariances(R.NP, X, ma, mb, lo, hi)
    mp, _ = SPR.pair_covariances(R.MP(), X, ma, mb, lo, hi)
    quad = SPR.quadrature_pairs(X, ma, mb, lo, hi, nodes)
    e_mp, e_q = (SPR.scaled_errors(val, r, scale, ("cov_pair",)) for r in (mp, quad))
    b = bar(ma, mb, lo, hi)
    print(f"d {d} N {N} order {order} cross {cross}: numpy - mpmath {e_mp:.2e} (bar {b:.1e}), numpy - quadrature {e_q:.2e}")
    assert val["cov_pair"].shape == (d * (d - 1) // 2,)
    assert e_mp < b
    assert e_q < max(1e-13, b)
    # the identities: two coordinates are all of d = 2, all but the third of d = 3
    cov, cscale = R.covariances(R.NP, X, ma, mb, lo, hi)
    if d == 2:
        assert abs(val["cov_pair"][0] - cov["cov_all"]) < b * (scale["cov_pair"][0] + cscale["cov_all"])
    if d == 3:
        for j, k in SPR.pairs(d):
            p, l = SPR.pair_index(j, k, d), 3 - j - k
            assert abs(val["cov_pair"][p] - cov["cov_rest"][l]) < b * (scale["cov_pair"][p] + cscale["cov_rest"][l])
    if not cross:
        # V_jk >= V_j + V_k up to the bar: the interaction variance is a variance
        for j, k in SPR.pairs(d):
            p = SPR.pair_index(j, k, d)
            slack = b * (scale["cov_pair"][p] + cscale["cov_first"][j] + cscale["cov_first"][k])
            assert val["cov_pair"][p] - cov["cov_first"][j] - cov["cov_first"][k] >= -slack
            assert val["cov_pair"][p] <= cov["cov_all"] + slack + b * cscale["cov_all"]


def test_pairs_disjoint_box():
    """the erfc path: a box six length scales from the design in coordinate 0"""
    X, ma, mb = models(40, 3, 2, True)
    lo, hi = R.boxes(X)["disjoint"]
    val, scale = SPR.pair_covariances(R.NP, X, ma, mb, lo, hi)
    mp, _ = SPR.pair_covariances(R.MP(), X, ma, mb, lo, hi)
    quad = SPR.quadrature_pairs(X, ma, mb, lo, hi, 32)
    b = bar(ma, mb, lo, hi)
    assert SPR.scaled_errors(val, mp, scale, ("cov_pair",)) < b
    assert SPR.scaled_errors(val, quad, scale, ("cov_pair",)) < max(1e-13, b)


def test_leave_two_out_and_numbering():
    F = np.random.default_rng(1).random((5, 6)) + 0.5
    G = SPR.leave_two_out(F)
    assert [SPR.pair_index(j, k, 6) for j, k in SPR.pairs(6)] == list(range(15))
    for p, (j, k) in enumerate(SPR.pairs(6)):
        assert np.allclose(G[:, p], np.prod(np.delete(F, [j, k], axis=1), axis=1), rtol=8 * EPS, atol=0)


@pytest.mark.parametrize("d,N,order,nodes", CASES)
def test_joint_surface(d, N, order, nodes):
    """joint and inter against mpmath and against quadrature of m over the other coordinates; joint - inter against the main
    effects; inter integrates to 0 over either coordinate"""
    X, m, _ = models(N, d, order, False)
    lo, hi = R.boxes(X)["design"]
    b = bar(m, m, lo, hi)
    j, k = 0, d - 1
    t = np.array([0.0, 1.0, 0.5, 0.3, 0.81])
    xj, xk = lo[j] + t * (hi[j] - lo[j]), lo[k] + t[::-1] * (hi[k] - lo[k])
    val, scale = SPR.joint_surface(R.NP, X, m, lo, hi, j, k, xj, xk)
    mp, _ = SPR.joint_surface(R.MP(), X, m, lo, hi, j, k, xj, xk)
    quad = SPR.quadrature_joint(X, m, lo, hi, j, k, xj, xk, nodes)
    keys = ("e0", "joint", "inter")
    e_mp, e_q = SPR.scaled_errors(val, mp, scale, keys), SPR.scaled_errors(val, quad, scale, keys)
    print(f"d {d} N {N} order {order}: numpy - mpmath {e_mp:.2e} (bar {b:.1e}), numpy - quadrature {e_q:.2e}")
    assert e_mp < b
    assert e_q < max(1e-13, b)
    grid = np.tile(lo[:, None], (1, len(t)))
    grid[j], grid[k] = xj, xk
    main, mscale = R.main_effects(R.NP, X, m, lo, hi, grid)
    want = main["main"][j] + main["main"][k] - main["e0"]
    slack = b * (scale["joint"] + scale["inter"] + mscale["main"][j] + mscale["main"][k] + mscale["e0"])
    assert np.all(np.abs((val["joint"] - val["inter"]) - want) < slack)
    for fixed in (j, k):
        nodes_, wt = SP.gauss_nodes(lo[j if fixed == k else k], hi[j if fixed == k else k], 32)
        for v in (xj[3] if fixed == j else xk[3],):
            a, c = (np.full(32, v), nodes_) if fixed == j else (nodes_, np.full(32, v))
            iv, isc = SPR.joint_surface(R.NP, X, m, lo, hi, j, k, a, c)
            assert abs(wt @ iv["inter"]) < max(1e-13, b) * (wt @ isc["inter"])


def fitted(N, d, order):
    X, m = R.rng_model(300 + 7 * N + d, N, d, order)
    y = np.random.default_rng(N + d).standard_normal(N)
    return (X, m) + SP.fit_state(X, y, order, m["A"], m["s"], NUGGET)


@pytest.mark.parametrize("box", ["design", "disjoint"])
@pytest.mark.parametrize("N,d,order", POST_CASES)
def test_pair_post(N, d, order, box):
    """s_pair against mpmath and against quadrature of c* itself; the identities with senspostref.post; Jensen's ordering"""
    X, m, P, G, Q, _, _, _, _ = fitted(N, d, order)
    lo, hi = R.boxes(X)[box]
    val, scale = SPR.pair_post(R.NP, X, m, P, G, Q, lo, hi)
    mp, _ = SPR.pair_post(R.MP(), X, m, P, G, Q, lo, hi)
    quad = SPR.quadrature_pair_post(X, m, P, G, Q, lo, hi)
    b = bar(m, m, lo, hi)
    e_mp, e_q = (SPR.scaled_errors(val, r, scale, ("s_pair",)) for r in (mp, quad))
    print(f"N {N} d {d} order {order} {box}: numpy - mpmath {e_mp:.2e} (bar {b:.1e}), numpy - quadrature {e_q:.2e}")
    assert e_mp < b
    assert e_q < max(1e-13, b)
    post, pscale = SP.post(R.NP, X, m, P, G, Q, lo, hi)
    for j, k in SPR.pairs(d):
        p = SPR.pair_index(j, k, d)
        if d == 2:
            assert abs(val["s_pair"][p] - post["s_all"]) < b * (scale["s_pair"][p] + pscale["s_all"])
        if d == 3:
            l = 3 - j - k
            assert abs(val["s_pair"][p] - post["s_rest"][l]) < b * (scale["s_pair"][p] + pscale["s_rest"][l])
        # s_none <= s_first[j], s_first[k] <= s_pair <= s_all
        slack = b * (scale["s_pair"][p] + pscale["s_all"] + pscale["s_first"][j] + pscale["s_first"][k])
        assert post["s_none"] <= min(post["s_first"][j], post["s_first"][k]) + slack
        assert max(post["s_first"][j], post["s_first"][k]) <= val["s_pair"][p] + slack
        assert val["s_pair"][p] <= post["s_all"] + slack


def test_pair_post_d4_against_mpmath():
    """d = 4 (two coordinates outside u), the first case of CASES, numpy against mpmath"""
    d, N, order, _ = CASES[0]
    X, m = R.rng_model(100 + N, N, d, order)
    y = np.random.default_rng(N + d).standard_normal(N)
    P, G, Q = SP.fit_state(X, y, order, m["A"], m["s"], NUGGET)[:3]
    lo, hi = R.boxes(X)["design"]
    val, scale = SPR.pair_post(R.NP, X, m, P, G, Q, lo, hi)
    mp, _ = SPR.pair_post(R.MP(), X, m, P, G, Q, lo, hi)
    assert SPR.scaled_errors(val, mp, scale, ("s_pair",)) < bar(m, m, lo, hi)
