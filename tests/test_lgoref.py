"""tests/lgoref.py (the reference the device and host tests of K-fold / leave-group-out validation are judged by) on every
input of tests/test_gpu_lgo.py: its own precondition -- the LAPACK refits on the N - b points against the closed form through
LAPACK's explicit inverse of the full matrix, to 1e-10 in the bars' measures, kappa_2(Sigma_B) <= 1e3 -- and the identities
the device tests lean on: groups of one point reproduce looref.closed_form, werr whitens with the UPPER factor of cov_B
(cov_B = U U^T, U werr = e), and relabelling the groups permutes the per-group numbers only.  CPU only."""
import numpy as np
import pytest

import lgoref
import looref
from madaiemulator_amd import synth
from oracle import oracle as O

CONFIGS = [(1, 1, 150, 3), (3, 1, 150, 3), (2, 0, 120, 2), (1, 2, 130, 4)]
RAGGED = [1, 2, 17, 33, 64]
EDGES = [1, 63, 64, 65, 129, 191]


def small_model(kind, order, N, d):
    """the inputs of test_gpu_loo.small_model (test_ragged_sizes_full_path's)"""
    X, y = synth.design(N, d, 900 + N)
    return X, y + 1.0, synth.default_thetas(kind, d)


def matrices(kind, order, N, d):
    X, y, th = small_model(kind, order, N, d)
    return O.cov_matrix(kind, X, th), O.hmatrix(order, X), y


@pytest.mark.parametrize("kind,order,N,d", CONFIGS)
@pytest.mark.parametrize("how", ["folds", "ragged"])
def test_reference_on_the_configurations(kind, order, N, d, how):
    Cm, H, y = matrices(kind, order, N, d)
    group = lgoref.folds(N, 5, seed=7) if how == "folds" else lgoref.ragged(N, RAGGED, 11)
    ref = lgoref.reference_from(Cm, H, y, group)
    print(f"kind {kind} order {order} N {N} {how}: routes disagree by {ref['ref_err']}, kappa_2 <= {ref['kappa2']:.1f}, "
          f"min offdiag {looref.min_offdiag(Cm):.2e}")
    assert looref.min_offdiag(Cm) >= looref.CLAMP
    assert np.array_equal(np.isnan(ref["mean"]), group < 0) and np.array_equal(np.isnan(ref["werr"]), group < 0)
    for r in ref["per_group"]:
        U = lgoref.upper_factor(r["cov"])
        e = U @ r["werr"]
        assert np.allclose(U, np.triu(U)) and np.all(np.diag(U) > 0)
        assert np.max(np.abs(U @ U.T - r["cov"])) <= 1e-12 * ref["kappa"] * max(1.0, ref["kappa2"])
        # werr_i depends on the errors of the members k >= i only: U e' = e row by row from the bottom
        assert abs(r["werr"][-1] - e[-1] / U[-1, -1]) <= 1e-12 * max(1.0, abs(r["werr"][-1]))


@pytest.mark.parametrize("kind", [1, 3])
def test_reference_on_the_granule_edges(kind):
    Cm, H, y = matrices(kind, 1, 513, 3)
    ref = lgoref.reference_from(Cm, H, y, lgoref.ragged(513, EDGES, 13))
    print(f"kind {kind} N 513 edges: routes disagree by {ref['ref_err']}, kappa_2 <= {ref['kappa2']:.1f}")
    assert not np.isnan(ref["mean"]).any()


def test_reference_on_three_folds_of_1000():
    Cm, H, y = matrices(1, 1, 1000, 3)
    ref = lgoref.reference_from(Cm, H, y, lgoref.folds(1000, 3, seed=17))
    print(f"N 1000 three folds: routes disagree by {ref['ref_err']}, kappa_2 <= {ref['kappa2']:.1f}")


@pytest.mark.parametrize("kind,order,N,d", [(1, 1, 130, 3), (3, 1, 150, 3)])
def test_groups_of_one_are_leave_one_out(kind, order, N, d):
    Cm, H, y = matrices(kind, order, N, d)
    ref = lgoref.reference_from(Cm, H, y, np.arange(N, dtype=np.int32))
    m, v = looref.closed_form(Cm, H, y)
    em, ev = looref.errors(ref["mean"], ref["var"], m, v, ref["kappa"])
    print(f"kind {kind} N {N}: groups of one against looref.closed_form: mean {em:.2e} var {ev:.2e}")
    assert em <= lgoref.PRECOND and ev <= lgoref.PRECOND
    # one point: werr = e / sd, maha = werr^2, logdet = log var
    e = y - m
    assert np.max(np.abs(ref["werr"] - e / np.sqrt(v))) <= lgoref.PRECOND * max(1.0, float(np.max(np.abs(e / np.sqrt(v)))))
    assert np.max(np.abs(ref["logdet"] - np.log(v))) <= lgoref.PRECOND


def test_relabelled_groups_permute_the_group_numbers():
    N = 150
    Cm, H, y = matrices(1, 1, N, 3)
    group = lgoref.folds(N, 5, seed=7)
    perm = np.array([3, 0, 4, 1, 2], dtype=np.int32)
    a = lgoref.reference_from(Cm, H, y, group)
    b = lgoref.reference_from(Cm, H, y, perm[group])
    for k in ("mean", "var", "werr"):
        assert np.array_equal(a[k], b[k])
    for k in ("maha", "logdet", "logpdf"):
        assert np.array_equal(a[k], b[k][perm])
