"""tests/jointref.py (the reference the device and host tests of hold-out validation and joint draws are judged by) on every
input family of tests/test_gpu_predict_joint.py: its own precondition -- float64 against the extended-precision repeat to
1e-10 in the bars' measures, kappa_2(S) <= 1e3, logpdf against scipy.stats.multivariate_normal -- and the identities the
device tests lean on: the leading part of a reference is the reference of the shorter call, a draw with z = werr returns the
observations, and the query sets of the other prediction tests could NOT be used (their Sigma is singular).  CPU only.

Measured over the 50 cases (25 families, with and without noise): the smallest eigenvalue of S without noise is 1.000000 ..
56.5 nuggets (never below one: Sigma - nugget I is a posterior covariance); kappa_2(S) 1.4 .. 126; float64 against
longdouble: werr 2.0e-16 .. 3.8e-15, maha <= 3.3e-16, logdet <= 5.6e-16 per point, draws <= 1.1e-15 of scale (bars 1e-10);
logpdf against scipy <= 1.6e-14 (bar 4 kappa_2 M 2^-52 = 1e-13 .. 2e-11).  The nugget e^-10 case: smallest eigenvalue 4.540e-5
= the nugget, kappa_2 4.0e3."""
import numpy as np
import pytest
import scipy.linalg as sl

import jointref
import predcovref
import vargradref
from test_gpu_predict_joint import (KINDS, entries_joint_inputs, ill_inputs, kinds_joint_inputs, log_mode_joint_inputs, normals,
                                    ragged_joint_inputs, sizes_inputs)
from test_gpu_var_grad import RAGGED, kinds_inputs, ragged_inputs


def families():
    out = {}
    for kind in (1, 3):
        out[f"sizes kind {kind}"] = sizes_inputs(kind)
    for kind, N in RAGGED:
        out[f"ragged kind {kind} N {N}"] = ragged_joint_inputs(kind, N)
    for kind, order, N, d in KINDS:
        out[f"kind {kind} order {order} N {N} d {d}"] = kinds_joint_inputs(kind, order, N, d)
    for kind in (2, 3):
        out[f"log mode kind {kind}"] = log_mode_joint_inputs(kind)
    out["entries"] = entries_joint_inputs()
    return out


FAMILIES = families()


@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_reference_on_every_family(name, noisy):
    kind, order, X, y, th, Xq = FAMILIES[name]
    M = Xq.shape[0]
    kap = vargradref.kappa(kind, th)
    noise = jointref.noise_for(kap, M, 3) if noisy else None
    ref = jointref.reference(kind, order, X, y, th, Xq, noise, z=normals(3, M, 4), nobs=3, seed=5)
    lam = np.linalg.eigvalsh(ref["S"])
    nug = kap - (float(np.exp(th[0])) if kind == 1 else float(th[0]))
    print(f"{name} noise {noisy}: lambda_min / nugget {lam[0] / nug:.6f}, kappa_2 {ref['kappa2']:.1f}, reference errors {ref['ref_err']}")
    if not noisy:
        assert lam[0] / nug >= 1.0 - 1e-9            # Sigma - nugget I is a posterior covariance: positive semi-definite
    # identities
    back = ref["mean"] + ref["werr"] @ ref["L"].T
    assert np.max(np.abs(back - ref["yobs"])) <= 1e-12 * max(1.0, float(np.max(np.abs(ref["yobs"] - ref["mean"]))))
    for Ms in (1, M // 2, M - 1):
        lead = jointref.leading(ref, Ms)
        alone = jointref.predict(kind, order, X, y, th, Xq[:Ms], None if noise is None else noise[:Ms], ref["yobs"][:, :Ms], ref["z"][:, :Ms])
        e = jointref.errors(dict(werr=lead["werr"], maha=lead["maha"], logdet=lead["logdet"], out=lead["out"]), alone, Ms,
                            float(np.max(np.abs(ref["z"]))), float(ref["var"].max()))
        assert all(v <= 1e-12 for v in e.values()), (Ms, e)
        assert np.max(np.abs(lead["logpdf"] - alone["logpdf"])) <= 1e-11 * Ms


@pytest.mark.parametrize("inputs", [ragged_inputs(1, 65), ragged_inputs(3, 513), kinds_inputs(2, 1, 300, 8)], ids=["ragged 1 65", "ragged 3 513", "kinds 2"])
def test_the_other_tests_query_sets_are_singular(inputs):
    """points on training points and copies of each other: float64 cholesky fails on their Sigma"""
    kind, order, X, y, th, Xq = inputs
    S = predcovref.predict(kind, order, X, y, th, Xq)["cov"]
    with pytest.raises(np.linalg.LinAlgError):
        sl.cholesky(0.5 * (S + S.T), lower=True)


def test_ill_conditioned_case_is_safely_positive_definite():
    kind, order, X, y, th, Xq = ill_inputs()
    S = predcovref.predict(kind, order, X, y, th, Xq)["cov"]
    lam = np.linalg.eigvalsh(0.5 * (S + S.T))
    print(f"nugget e^-10: lambda_min {lam[0]:.3e} (nugget {np.exp(-10.0):.3e}), kappa_2 {lam[-1] / lam[0]:.3g}")
    assert lam[0] >= 0.99 * np.exp(-10.0) and 1e3 <= lam[-1] / lam[0] <= 1e6


def test_mpmath_route_on_a_small_case():
    kind, order, X, y, th, Xq = ragged_joint_inputs(3, 63)
    ref = jointref.predict(kind, order, X, y, th, Xq[:9], None, None, normals(2, 9, 1))
    ref = jointref.predict(kind, order, X, y, th, Xq[:9], None, jointref.observations(ref, 2, 2), normals(2, 9, 1))
    w, o, ld = jointref.mpmath_factor(ref["S"], ref["yobs"] - ref["mean"], ref["z"])
    e = jointref.errors(ref, dict(werr=w, maha=np.sum(w * w, axis=1), logdet=ld, out=ref["mean"] + o), 9,
                        float(np.max(np.abs(ref["z"]))), float(ref["var"].max()))
    print(f"float64 against mpmath at 40 digits {e}")
    assert all(v <= jointref.PRECOND for v in e.values())
