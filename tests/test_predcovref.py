"""tests/predcovref.py (the reference the device tests of the joint posterior covariance are judged by) against things that
do not share its route: its extended-precision repeat on every input family of tests/test_gpu_predict_cov.py; the
saddle-point form Sigma = C** - [K H*] [[C, H], [H^T, 0]]^-1 [K H*]^T solved as one indefinite system with iterative
refinement in longdouble; vargradref's variance on the diagonal; the closed form c + h_p^T Q h_q on a far block.  CPU only.

Measured, in units of the bar's scale (kappa; max(kappa, |var|) for far queries): float64 against longdouble 2.0e-16 ..
2.8e-15 on the near-query families, 2.1e-14 at d = 31 order 2 (63 basis functions), 8.3e-14 .. 2.3e-13 with the far queries
(the device tests' precondition is 1e-10: almost three orders of margin at the least); longdouble against the saddle-point
form 1.6e-19 .. 1.0e-17, far queries 2.8e-17 .. 5.5e-17; the smallest eigenvalue of the reference Sigma -1.8e-13 .. -1e-16
of scale; the diagonal against vargradref.predict's variance <= 3.5e-15; the far block against c + h^T Q h <= 1.5e-16, far
variances 1.6e3 .. 3.0e3 kappa; off-diagonal elements of the nugget-rule pairs 0.22 .. 1.02 kappa (the copy, 5e-11 apart) and 0
(two queries on one training point, where the posterior variance itself is 0)."""
import numpy as np
import pytest
import scipy.linalg as sl

import predcovref
import vargradref
from oracle import oracle as O
from test_gpu_predict_cov import FAR, PAIRS, far_cov_inputs, nugget_inputs
from test_gpu_mean_grad import clamp_inputs
from test_gpu_var_grad import entries_inputs, forms_inputs, kinds_inputs, log_mode_inputs, ragged_inputs, stale_inputs

needs_extended = pytest.mark.skipif(not vargradref.LD_IS_EXTENDED, reason="numpy's longdouble is no wider than a double here")


def families():
    """name -> (kind, order, X, y, th, Xq, far) for one member or more of every input family of the device tests"""
    out = {}
    for kind, N in ((1, 65), (3, 129), (1, 513)):
        out[f"ragged kind {kind} N {N}"] = ragged_inputs(kind, N) + ((),)
    for kind, order, N, d in ((1, 0, 300, 8), (2, 3, 300, 8), (3, 2, 300, 8), (2, 1, 200, 1), (3, 1, 200, 17), (1, 2, 330, 31), (1, 0, 200, 64)):
        out[f"kind {kind} order {order} N {N} d {d}"] = kinds_inputs(kind, order, N, d) + ((),)
    for kind in (2, 3):
        out[f"log mode kind {kind}"] = log_mode_inputs(kind) + ((),)
    for kind in (1, 2, 3):
        k, order, X, y, th, th_short, Xq = forms_inputs(kind)
        out[f"forms kind {kind}"] = (k, order, X, y, th, Xq, ())
        out[f"short length scales kind {kind}"] = (k, order, X, y, th_short, Xq, ())
        X, y, th, Xq, order = clamp_inputs(kind)
        out[f"clamped kind {kind}"] = (kind, order, X, y, th, Xq, ())
        X, y, th, Xq, order = nugget_inputs(kind)
        out[f"nugget rule kind {kind}"] = (kind, order, X, y, th, Xq, ())
        out[f"far kind {kind}"] = far_cov_inputs(kind) + (FAR,)
    out["entries"] = entries_inputs() + ((),)
    kind, order, X, y, th1, th2, y2, Xq = stale_inputs()
    out["new set-up"] = (kind, order, X, y2, th2, Xq, ())
    return out


FAMILIES = families()


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_reference_on_every_family(name):
    """the float64 reference against its extended-precision repeat (bar 1e-10, the device tests' precondition), its
    symmetry, its smallest eigenvalue, its diagonal against vargradref's variance"""
    kind, order, X, y, th, Xq, far = FAMILIES[name]
    ref = predcovref.reference(kind, order, X, y, th, Xq, far=far)
    S, kap = ref["cov"], ref["kappa"]
    asym = float(np.max(np.abs(S - S.T)) / ref["vscale"].max())
    lam = float(np.linalg.eigvalsh(0.5 * (S + S.T))[0]) / float(ref["vscale"].max())
    vg = vargradref.predict(kind, order, X, y, th, Xq, far=far)
    ed = float(np.max(np.abs(ref["var"] - vg["var"]) / vg["vscale"]))
    em = float(np.max(np.abs(ref["mean"] - vg["mean"]) / np.maximum(1.0, np.abs(vg["mean"]))))
    print(f"{name}: float64 against extended {ref['ref_err'][0]:.2e}, A N eps {ref['ref_err'][1]:.2e}, asymmetry {asym:.1e}, "
          f"smallest eigenvalue / scale {lam:.1e}, diagonal against vargradref {ed:.1e}, mean {em:.1e}")
    assert asym <= 1e-12 and lam >= -1e-12 and ed <= 1e-12 and em <= 1e-12


@needs_extended
@pytest.mark.parametrize("name", sorted(n for n in FAMILIES if FAMILIES[n][2].shape[0] <= 330))
def test_longdouble_route_against_the_saddle_point_form(name):
    """bar 1e-13 of scale, three orders under the precondition the longdouble route is there to support: both sides carry
    longdouble rounding (2^-64 = 5e-20) times the conditioning of their own system, which the order-2 basis at coordinates
    of 30 .. 40 (the far family) brings to 1e5"""
    kind, order, X, y, th, Xq, far = FAMILIES[name]
    ref = predcovref.predict(kind, order, X, y, th, Xq, far=far)
    a = predcovref.longdouble_route(kind, order, X, th, ref["Xq"], ref["K"])
    b = predcovref.saddle_route(kind, order, X, th, ref["Xq"], ref["K"])
    err = predcovref.error(a, b, ref["vscale"])
    print(f"{name}: longdouble route against the saddle-point form {err:.2e}")
    assert err <= 1e-13


def test_mpmath_route_on_a_small_case():
    """the route a platform without an extended longdouble would take, against the float64 one"""
    kind, order, X, y, th, Xq = ragged_inputs(3, 63)
    ref = predcovref.predict(kind, order, X, y, th, Xq[:9])
    err = predcovref.error(ref["cov"], predcovref.mpmath_route(kind, order, X, th, ref["Xq"], ref["K"]), ref["vscale"])
    print(f"float64 against mpmath at 40 digits {err:.2e}")
    assert err <= predcovref.PRECOND


@pytest.mark.parametrize("kind", [1, 2, 3])
def test_far_block_is_the_regression_term(kind):
    kind, order, X, y, th, Xq = far_cov_inputs(kind)
    ref = predcovref.predict(kind, order, X, y, th, Xq, far=FAR)
    assert np.all(ref["K"][FAR] == 0.0)
    H = O.hmatrix(order, X)
    Q = np.linalg.inv(H.T @ sl.cho_solve(sl.cho_factor(O.cov_matrix(kind, X, th), lower=True), H))
    hq = O.hmatrix(order, Xq[FAR])
    err = predcovref.error(ref["cov"][np.ix_(FAR, FAR)], O.cov_matrix(kind, Xq[FAR], th) + hq @ Q @ hq.T, ref["vscale"][FAR])
    print(f"kind {kind}: far block against c + h^T Q h {err:.2e}; far variances / kappa {ref['var'][FAR] / ref['kappa']}")
    assert err <= 1e-12


@pytest.mark.parametrize("kind", [1, 2, 3])
def test_nugget_rule_in_the_reference(kind):
    """what the device test relies on: the copy's rows are identical and the pairs' off-diagonal elements are of the order of
    kappa wherever the pair shares the nugget's box or lies in an unclamped neighbourhood"""
    X, y, th, Xq, order = nugget_inputs(kind)
    ref = predcovref.predict(kind, order, X, y, th, Xq)
    S, kap = ref["cov"], ref["kappa"]
    vals = [float(S[p, q] / kap) for p, q in PAIRS]
    print(f"kind {kind}: off-diagonal elements / kappa at the pairs {vals}")
    assert np.allclose(S[11], S[4], rtol=0, atol=1e-13 * kap)
    (p, q), (p2, q2) = PAIRS[0], PAIRS[1]
    assert abs(S[p, q] - S[q, q]) <= 1e-13 * kap                      # a copy: the variance itself, nugget included
    nug = float(np.exp(th[1])) if kind == 1 else float(th[1])
    # 5e-11 apart: the nugget is there for pow-exp and absent for Matern
    gap = S[q2, q2] - S[p2, q2]
    assert abs(gap - (0.0 if kind == 1 else nug)) <= 1e-6 * kap
