"""The CPU reference of the gain over target points (tests/designtargetref.py) pinned three ways, without a GPU:
(a) its float64 LAPACK route against the extended-precision one (longdouble, and mpmath on a small case),
(b) the identity gain = target_var - target_var' against a refit on N + 1 points, for all three covariance functions,
(c) designref.gain: power-exponential, d <= 2, the targets a tensor Gauss-Legendre rule of the box, so that the weighted sum is
    the closed form's integral up to the quadrature error.
Figures (`python tests/designtargetref.py --measure`): the float64 route is within 1.4e-11 of the extended one on the bars'
scales over the 69 shape cases (PRECOND = 1e-10); the refit gaps are at most 1.9e-16 of kappa sum w; the Gauss-Legendre sum meets
the closed form to 1.9e-15 of the closed form's scale from 12 nodes per coordinate on (1.1e-12 to 2.7e-12 with 8)."""
import itertools

import mpmath  # noqa: F401  (pin (a) needs it: no skip without it)
import numpy as np
import pytest

import designtargetref as T
from oracle import oracle as O

REFIT_NP = 1.9e-16               # measured; asserted here with the factor the device gets
QUAD_NP = 1.9e-15
FACTOR = 8


def small(kind, order=1, N=20, d=3, S=9, M=4):
    c = T.case(65, d, order, kind, M, S, 9)
    c["X"], c["y"] = c["X"][:N], c["y"][:N]
    c["Xt"][0], c["Xq"][0] = c["X"][0], c["X"][1]
    return c


@pytest.mark.parametrize("kind", T.KINDS)
def test_kernel_is_the_oracles_element_off_the_nugget_rule(kind):
    c = small(kind)
    K = T.kernel(kind, c["th"], c["Xt"][1:], c["X"])
    ref = np.array([[O.cov(kind, x, z, c["th"]) for z in c["X"]] for x in c["Xt"][1:]])
    assert np.max(np.abs(K - ref)) <= 4 * 2.0 ** -52 * T.amp_nugget(kind, c["th"])[0]
    amp, nug = T.amp_nugget(kind, c["th"])
    assert T.kernel(kind, c["th"], c["X"][:1], c["X"][:1])[0, 0] == amp                          # no nugget on coinciding points
    assert abs(O.cov(kind, c["X"][0], c["X"][0], c["th"]) - (amp + nug)) <= 1e-15


@pytest.mark.parametrize("kind", T.KINDS)
@pytest.mark.parametrize("order", [0, 2])
def test_float64_route_against_the_extended_routes(kind, order):
    c = small(kind, order)
    f = T.float64_route(kind, order, c["X"], c["th"], c["Xt"], c["w"], c["Xq"])
    sc = T.scales(kind, c["th"], c["w"], f["var"])
    keys = ("cstar", "var", "var_t", "target_var", "num", "gain")
    ld = T.longdouble_route(kind, order, c["X"], c["th"], c["Xt"], c["w"], c["Xq"])
    e = T.errors(f, ld, sc, keys)
    assert max(e.values()) <= T.PRECOND, e
    mp = T.mpmath_route(kind, order, c["X"], c["th"], c["Xt"], c["w"], c["Xq"])
    e = T.errors(f, mp, sc, keys)
    assert max(e.values()) <= T.PRECOND, e


def test_reference_asserts_its_own_conditioning():
    c = small(O.POWEREXP)
    ref = T.reference(c)
    assert max(ref["ref_err"].values()) <= T.PRECOND
    bad = T.case(130, 1, 3, O.POWEREXP, 4, 9, 9)
    bad["th"] = np.array([0.0, np.log(1e-14), np.log(0.3)])                                      # 130 points on a line, next to no nugget
    with pytest.raises(AssertionError, match="ill-conditioned"):                                 # (var and var_t are off by 1e-8 kappa)
        T.reference(bad)


def test_gain_is_bounded_and_zero_weights_count_for_nothing():
    c = small(O.MATERN52, S=12)
    ref = T.float64_route(c["kind"], c["order"], c["X"], c["th"], c["Xt"], c["w"], c["Xq"])
    assert np.all(ref["gain"] >= 0) and np.all(ref["gain"] <= ref["target_var"] * (1 + 1e-12))
    keep = c["w"] > 0
    assert not keep.all()
    part = T.float64_route(c["kind"], c["order"], c["X"], c["th"], c["Xt"][keep], c["w"][keep], c["Xq"])
    assert np.allclose(part["num"], ref["num"], rtol=1e-14, atol=0) and np.isclose(part["target_var"], ref["target_var"], rtol=1e-14)


@pytest.mark.parametrize("i", range(len(T.REFIT_CASES)))
def test_refit_identity(i):
    """gain(x*) = target_var(design) - target_var(design + {x*}), the thetas as they are: every kind once"""
    c = T.refit_cases()[i]
    gaps = T.refit_gaps(c)
    print(c["name"], gaps)
    assert gaps.max() <= FACTOR * REFIT_NP, gaps


@pytest.mark.parametrize("i", range(len(T.QUAD_CASES)))
def test_closed_form_link(i):
    """Gauss-Legendre targets: the weighted sum is designref.gain's integral"""
    c, lo, hi = T.quad_cases()[i]
    e = T.quadrature_error(c, lo, hi)
    print(c["name"], e)
    assert e <= FACTOR * QUAD_NP, e
    assert np.isclose(c["w"].sum(), 1.0, rtol=1e-14)


def test_sweep_scale_bounds_its_error():
    """float64 against longdouble on the sweep's own computation stays within a few ulp of its scale"""
    for kind in T.KINDS:
        assert T.sweep_error(small(kind, S=70, M=5)) <= 4 * 2.0 ** -52


def test_every_value_meets_every_other():
    """the rotation of kind, M and S in shape_cases(): every pair of values of two different axes occurs in some case"""
    cases = T.shape_cases()
    axes = [T.NS, T.DS, T.ORDERS, T.KINDS, T.MS, T.MS]
    for a, b in itertools.combinations(range(6), 2):
        seen = {(c[a], c[b]) for c in cases}
        for va in axes[a]:
            for vb in axes[b]:
                if (a, b) in ((0, 1), (0, 2), (1, 2)) and not any(c[a] == va and c[b] == vb for c in cases):
                    continue                     # (N, d, order): the full cross, minus the orders that do not fit
                assert (va, vb) in seen, (a, b, va, vb)
