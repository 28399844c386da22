"""The catalogue of tests/entryorder.py is complete and its inputs keep their own preconditions (no device needed).

Every symbol of abi.SYMBOLS -- which tests/test_abi.py ties to include/gpemu.h -- is named by exactly one probe, disturber or
EXEMPT entry: a new entry cannot be added without placing it among the orders tests/test_gpu_entry_order.py runs."""
import numpy as np
import pytest

import entryorder as E
import jointref
from madaiemulator_amd import abi


def test_every_symbol_is_named_exactly_once():
    named = E.named()
    missing = sorted(set(abi.SYMBOLS) - set(named))
    assert not missing, f"not in the catalogue of tests/entryorder.py: {missing}"
    unknown = sorted(set(named) - set(abi.SYMBOLS))
    assert not unknown, f"the catalogue names what include/gpemu.h does not declare: {unknown}"
    twice = {s: w for s, w in named.items() if len(w) != 1}
    assert not twice, f"named more than once: {twice}"


def test_a_name_taken_out_of_the_catalogue_is_missed(monkeypatch):
    """the check above does fail: without the probe that names gpemu_loo, and without an EXEMPT line"""
    monkeypatch.delitem(E.ALL, "loo")
    assert "gpemu_loo" not in E.named() and "gpemu_loo_dev" not in E.named()
    with pytest.raises(AssertionError, match="gpemu_loo"):
        test_every_symbol_is_named_exactly_once()
    monkeypatch.undo()
    monkeypatch.delitem(E.EXEMPT, "gpemu_sync")
    with pytest.raises(AssertionError, match="gpemu_sync"):
        test_every_symbol_is_named_exactly_once()


def test_exempt_lines_give_a_reason_and_the_lists_are_consistent():
    assert all(isinstance(r, str) and len(r) > 10 for r in E.EXEMPT.values())
    assert set(E.PROBES) <= set(E.ALL) and len(set(E.PROBES)) == len(E.PROBES)
    assert set(E.REDUCED_B) <= set(E.PROBES)
    # the reduced list of model B has every probe that keeps state and every probe that needs what another one left
    assert {n for n in E.PROBES if E.ALL[n].keeps or E.ALL[n].after} <= set(E.REDUCED_B)
    for n, p in E.ALL.items():
        assert p.after is None or p.after in E.PROBES, n
        assert p.needs <= {"setup", "calib", "prior"}, n
    # every sized family has all four sizes and a neighbour of the same buffer family to run in between
    assert set(E.BETWEEN) == set(E.SIZED_FAMILIES)
    for fam, other in E.BETWEEN.items():
        assert other in E.ALL and E.ALL[other].family != fam
        assert all(f"{fam}_{M}" in E.ALL for M in E.SIZES)
    # what the issue lists: at least one probe each
    for n in ("predict_1", "predict_5", "predict_70", "predict_mean_70", "predict_mean_grad_70", "predict_var_grad_70", "predict_cov_70", "joint_70",
              "joint_draw_only", "loo", "lgo", "sens_cov", "sens_cov_two", "sens_main", "sens_post", "sens_main_var", "sens_pairs", "sens_pairs_post",
              "sens_joint", "design_gain_70", "design_batch_70", "target_gain_70", "target_gain_only", "calib_eval_70", "calib_grad_70",
              "calib_select_70", "calib_sample", "cinverse", "cov_matrix", "kvectors"):
        assert n in E.PROBES, n
        if n.startswith("sens_"):
            assert n + "_mixed" in E.PROBES
    # the host-buffer prediction entries stage through the pending batch's buffers and refuse while one is pending (gpemu.h at
    # gpemu_predict_batch_enqueue, gpemu_predict_cov, gpemu_predict_joint_factor); nothing else does
    assert {E.ALL[n].family or n for n in E.REFUSES_PENDING} == {"predict", "predict_mean", "predict_mean_grad", "predict_var_grad", "predict_cov",
                                                                 "joint", "joint_draw_only", "calib_grad", "calib_select"}


@pytest.mark.parametrize("name", sorted(E.SPEC))
def test_the_inputs_keep_their_preconditions(name):
    m = E.model(name)
    assert m.X.shape == (m.N, m.d) and m.Y.shape == (m.N, 3) and m.N % 64 != 0 and m.N > 64
    assert all(np.all(np.isfinite(v)) for v in (m.X, m.Y, m.lo, m.hi, m.glo, m.ghi, m.grid))
    assert np.all(m.hi > m.lo) and np.all(m.ghi[m.mkind == abi.MEASURE_GAUSS] > 0) and 0 < m.mkind.sum() < m.d
    # the components differ: training vectors and thetas
    assert not np.array_equal(m.Y[:, 0], m.Y[:, 1]) and not np.array_equal(m.Y[:, 1], m.Y[:, 2])
    assert not np.array_equal(m.ths[0], m.ths[1]) and len(m.ths[0]) == abi.nthetas_for(m.kind, m.d)
    # leave-group-out: three groups, none empty, none so large that no degree of freedom is left
    sizes = np.bincount(m.group, minlength=3)
    assert len(sizes) == 3 and sizes.min() >= 1 and m.N - sizes.max() > m.nreg
    # candidates are not design points (a tenth of a length scale away at least), at every size, and no two alike
    ln = np.exp(m.ths[0][2:])
    for M in E.SIZES:
        c = m.cand[M]
        assert c.shape == (M, m.d) and m.Xq[M].shape == (M, m.d) and m.Xj[M].shape == (M, m.d)
        assert np.sqrt((((c[:, None, :] - m.X[None, :, :]) / ln) ** 2).sum(axis=2)).min() >= 0.1
        assert len(np.unique(c, axis=0)) == M and len(np.unique(m.Xj[M], axis=0)) == M
        assert np.all(m.noise[M] > 0) and m.yobs[M].shape == (2, M) and m.z[M].shape == (3, M)
    # targets: non-negative weights that do not sum to 0
    assert m.Xt.shape == (E.NTARGETS, m.d) and np.all(m.wt >= 0) and m.wt.sum() > 0
    # the walkers start inside the prior's box, an even number of them
    assert m.walkers % 2 == 0 and m.walkers // 2 >= m.d + 1 and m.x0.shape == (m.walkers, m.d)
    assert np.all(m.x0 > m.prior[0]) and np.all(m.x0 < m.prior[1])


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("M", E.SIZES)
def test_the_joint_matrix_with_its_noise_is_positive_definite(name, M):
    """for every component and both theta vectors a case sets up with: the smallest eigenvalue of S = Sigma + diag(noise) stays
    above a tenth of the smallest noise (Sigma is positive semi-definite up to rounding)"""
    m = E.model(name)
    for col in range(3):
        for shift in (0.0, E.THETA2_SHIFT):
            th = m.ths[col].copy()
            th[2:] += shift
            S = jointref.predict(m.kind, m.order, m.X, m.Y[:, col], th, m.Xj[M], noise=m.noise[M])["S"]
            assert np.linalg.eigvalsh(S).min() > 0.1 * m.noise[M].min()


def test_the_calibration_table_is_one_for_all_models():
    c = E.calib_case()
    assert c["nr"] == 2 and c["nt"] == 3 and c["mean"].shape == (2, max(E.SIZES)) and c["S"] is None and c["rel"] is not None
    r = abi.calib_project(c["ybar"], c["A"], c["z"], sd=c["sd"])
    assert r["status"] == abi.OK and r["info"] == 0 and np.all(np.isfinite(r["sigz"]))
