"""tests/resref.py (the reference the per-launch tests of the resident-factor kernels are judged by) means what production
means: composed the way gpemu_loo and gpemu_lgo compose their kernels, on L^-1, gamma, W^T, beta and Q built in numpy from
the oracle's covariance matrix, it reproduces looref.closed_form and lgoref.closed_form; the product reference summed over
its slices is Kq L^T with L's upper part dropped.  And every bar is finite and positive, every asserted precondition holds,
on every case tests/test_gpu_resident_kernels.py uses.  CPU only."""
import numpy as np
import pytest

import lgoref
import looref
import resref as R
from madaiemulator_amd import synth
from oracle import oracle as O

LD = R.LD
N_MODEL, D_MODEL = 130, 3


def model(kind):
    """N = 130, d = 3, order 1 -> the resident state in longdouble: L^-1, gamma, W, beta, Q (and C, H, y)"""
    X, y = synth.design(N_MODEL, D_MODEL, 900 + N_MODEL)
    y = y + 1.0
    Cm, H = O.cov_matrix(kind, X, synth.default_thetas(kind, D_MODEL)), O.hmatrix(1, X)
    Lc, p = R.cholesky_ld(Cm)
    assert p == 0
    Linv = R.tri_inverse_ld(Lc)
    Ci = Linv.T @ Linv
    W = Ci @ np.asarray(H, dtype=LD)
    Rq, p = R.cholesky_ld(np.asarray(H, dtype=LD).T @ W)
    assert p == 0
    Rqi = R.tri_inverse_ld(Rq)
    Q = Rqi.T @ Rqi
    beta = Q @ (W.T @ y)
    gamma = Ci @ y - W @ beta
    return dict(Cm=Cm, H=H, y=y, Linv=Linv, W=W, Q=Q, beta=beta, gamma=gamma)


@pytest.mark.parametrize("kind", [1, 3])
def test_colsq_then_finish_is_the_leave_one_out_closed_form(kind):
    m = model(kind)
    N, Np = N_MODEL, R.round_up(N_MODEL, 64)
    lin = R.nans(Np, Np)
    lin[:N, :N] = np.asarray(m["Linv"], dtype=np.float64)
    part, bar, cls = R.colsq_reference(lin, N, Np)
    assert np.all(np.isfinite(np.asarray(part, dtype=np.float64)))
    ref = R.loo_finish_reference(part, m["gamma"], m["W"], m["Q"], m["y"], N, Np)
    mean, var = looref.closed_form(m["Cm"], m["H"], m["y"])
    em, ev = looref.errors(np.asarray(ref["mean"], dtype=np.float64), np.asarray(ref["var"], dtype=np.float64), mean, var, float(m["Cm"][0, 0]))
    print(f"kind {kind}: colsq -> finish against looref.closed_form: mean {em:.2e} var {ev:.2e}")
    assert em <= 1e-12 and ev <= 1e-12


@pytest.mark.parametrize("kind", [1, 3])
def test_gather_stage_factor_finish_is_the_leave_group_out_closed_form(kind):
    m = model(kind)
    N, Np, nreg = N_MODEL, R.round_up(N_MODEL, 64), 1 + D_MODEL
    sizes, bp = (1, 17, 33, 64), 64
    tab = R.group_tables(N, sizes, 11, bp)
    Linv64 = np.asarray(m["Linv"], dtype=np.float64)
    Z = np.asarray(R.gather_reference(Linv64, N, Np, tab, 0, len(sizes)), dtype=LD)
    ts = R.tall_rows(bp) * bp
    t = R.nans(len(sizes) * ts)
    low = R.lower_tiles(bp)
    for g in range(len(sizes)):
        Zg = Z[g * bp:(g + 1) * bp]
        t[g * ts:g * ts + bp * bp].reshape(bp, bp)[low] = np.asarray(Zg @ Zg.T, dtype=np.float64)[low]
    lin = R.nans(Np + 1 + nreg, Np)
    lin[Np, :N] = np.asarray(m["gamma"], dtype=np.float64)
    lin[Np + 1:, :N] = np.asarray(m["W"].T, dtype=np.float64)
    betaq = np.concatenate([np.asarray(m["beta"], dtype=np.float64), np.asarray(m["Q"], dtype=np.float64).ravel()])
    case = dict(t=t, lin=lin, betaq=betaq, tab=tab, N=N, Np=Np, ld=Np, bp=bp, nbc=len(sizes), g0=0, nreg=nreg, tstride=ts)
    staged, bar, cls = R.stage_reference(case)
    # the lock-step factorisation with inverse rows, in numpy: P = R R^T, w = R^-1 gamma_B, U = R^-T
    t2, res = R.nans(len(sizes) * ts), np.empty(2 * len(sizes))
    for g in range(len(sizes)):
        M = staged[g * ts:(g + 1) * ts].reshape(R.tall_rows(bp), bp)
        P = np.tril(M[:bp]) + np.tril(M[:bp], -1).T
        Rg, p = R.cholesky_ld(P)
        assert p == 0
        Ri = R.tri_inverse_ld(Rg)
        w = Ri @ M[bp]
        M2 = t2[g * ts:(g + 1) * ts].reshape(R.tall_rows(bp), bp)
        M2[bp] = np.asarray(w, dtype=np.float64)
        M2[bp + 64:] = np.asarray(Ri.T, dtype=np.float64)
        res[2 * g], res[2 * g + 1] = float(w @ w), float(2 * np.sum(np.log(np.diag(Rg))))
    fc = dict(t=t2, res=res, y=m["y"], tab=tab, N=N, bp=bp, nbc=len(sizes), g0=0, tstride=ts,
              info=np.full(len(sizes), R.INFO_NONE, dtype=np.int32), ngroups=len(sizes))
    fin = R.finish_reference(fc)
    got = dict(mean=np.asarray(fin["mean"][0], dtype=np.float64), var=np.asarray(fin["var"][0], dtype=np.float64),
               werr=np.asarray(fin["werr"][0], dtype=np.float64))
    for i, k in enumerate(("maha", "logdet", "logpdf")):
        got[k] = np.asarray(fin["stat"][0][i], dtype=np.float64)
    closed = lgoref.closed_form(m["Cm"], m["H"], m["y"], tab["groups"])
    e = lgoref.worst([lgoref.errors(g_, c, float(m["Cm"][0, 0])) for g_, c in zip(lgoref.split(got, tab["groups"]), closed)])
    print(f"kind {kind}: gather -> Z Z^T -> stage -> Cholesky -> finish against lgoref.closed_form: {e}")
    assert all(v <= 1e-12 for v in e.values()), e
    assert np.all(fin["info_out"][0] == 0)
    left_out = np.isin(np.arange(N), np.concatenate(tab["groups"]))
    assert np.array_equal(fin["mean"][2] == R.VALUE, left_out)


@pytest.mark.parametrize("Np", sorted(R.PRODUCT_SPLITS))
@pytest.mark.parametrize("kind", R.KINDS)
def test_product_slices_add_up_to_the_triangular_product(Np, kind):
    case = R.product_case(7 + Np, Np, 16, kind)
    K, ntot = case["K"], case["ntot"]
    Lz = np.asarray(np.where(np.isnan(case["lin"][:, :K]), 0.0, case["lin"][:, :K]), dtype=LD)
    n, k = np.indices((ntot, K))
    assert np.all(Lz[(n < Np) & (k > n)] == 0)
    full = np.asarray(case["kq"][:, :K], dtype=LD) @ Lz.T
    for nslice, klen in R.PRODUCT_SPLITS[Np]:
        assert klen % 16 == 0 and nslice * klen >= K
        want, bar = R.product_reference(case, nslice, klen)
        assert np.all(np.isfinite(np.asarray(want, dtype=np.float64))) and np.all(np.isfinite(np.asarray(bar, dtype=np.float64)))
        assert np.all(bar >= 0) and np.all(bar[want != 0] > 0)
        tot = want.sum(axis=0)
        if kind == "int":
            assert np.array_equal(tot, full)
        else:
            assert np.max(np.abs(tot - full) / (np.abs(np.asarray(case["kq"][:, :K], dtype=LD)) @ np.abs(Lz).T + 1e-300)) <= 2.0 ** -60
        # later slices start beyond ke(n) for the upper rows: zeros are expected there, and they are VALUE
        if nslice > 1:
            assert np.all(want[-1][:, :16] == 0) and np.all(bar[-1][:, :16] == 0)
    assert sorted(R.production_klen(Np, s) for s, _ in R.PRODUCT_SPLITS[Np] if (s, _) != (3, 80)) == \
        sorted(kl for s, kl in R.PRODUCT_SPLITS[Np] if (s, kl) != (3, 80))


def _pos_finite(bar, want=None):
    b = np.asarray(bar, dtype=np.float64)
    assert np.all(np.isfinite(b)) and np.all(b >= 0)
    if want is not None:
        assert np.all(b[np.asarray(want != 0)] > 0)


def test_bars_and_preconditions_of_the_loo_cases():
    lens = set()
    for N in R.COLSQ_N:
        lin, Np, ld = R.linv_case(100 + N, N)
        want, bar, cls = R.colsq_reference(lin, N, Np)
        _pos_finite(bar, want)
        assert not np.isnan(np.asarray(want, dtype=np.float64)).any()
        assert np.array_equal(cls == R.VALUE, R.launched(N, Np))
    for N, nreg in R.LOO_FINISH_CASES:
        c = R.loo_finish_case(200 + N, N, nreg)
        Np = c["Np"]
        ref = R.loo_finish_reference(c["part"], c["lin"][Np, :N], c["lin"][Np + 1:, :N].T, c["betaq"][nreg:].reshape(nreg, nreg), c["y"], N, Np)
        _pos_finite(ref["bar_mean"])
        _pos_finite(ref["bar_var"])
        assert np.all(ref["bar_var"] > 0) and np.all(ref["bar_mean"] > 0)
        assert np.all(ref["reg"] <= ref["pii"]) and np.all(ref["pii"] > 0)
        # the bar stays within a few hundred u of the result
        assert float(np.max(ref["bar_var"] / ref["var"])) <= 400 * float(R.U)
        nch = R.nchunks_of(N)
        lens |= {nch - (i // R.LOO_SW) * (R.LOO_SW // R.LOO_RC) for i in range(N)}
    assert lens == {1, 2, 3, 4, 5, 9, 17}, lens
    assert {nreg for _, nreg in R.LOO_FINISH_CASES} == {1, 3, 4, 5, 21, 63}


def test_bars_and_preconditions_of_the_lgo_cases():
    for N, sizes, bp in R.GATHER_CASES:
        tab = R.group_tables(N, sizes, 300 + N, bp)
        assert tab["bp"] == 128 and (tab["group"] == -1).any()
        assert all(np.any(np.diff(B) > 1) for B in tab["groups"] if len(B) > 2)       # interleaved in design order
        lin, Np, ld = R.linv_case(310 + N, N)
        Z = R.gather_reference(lin, N, Np, tab, 0, len(sizes))
        assert np.all(np.isfinite(Z)) and Z.shape == (len(sizes) * bp, Np)
    for N, bp, sizes, nreg, g0 in R.STAGE_CASES:
        c = R.stage_case(400 + nreg, N, bp, sizes, nreg, g0)
        want, bar, cls = R.stage_reference(c)
        v = cls == R.VALUE
        assert not np.isnan(np.asarray(want[v], dtype=np.float64)).any()
        _pos_finite(bar[v])
        assert np.all(R.is_prefill(c["t"])[cls == R.UNCHANGED])
    for N, bp, sizes, g0, words in R.FINISH_CASES:
        c = R.finish_case(500 + bp + g0, N, bp, sizes, g0, words)
        ref = R.finish_reference(c)
        for k in ("mean", "var", "werr"):
            want, bar, cls = ref[k]
            _pos_finite(bar)
            bad = np.isnan(np.asarray(want, dtype=np.float64))
            assert bad.sum() == sizes[g0 + list(words).index(5)]
            if k != "werr":
                assert np.all(bar[(cls == R.VALUE)] > 0)
        _pos_finite(ref["stat"][1])
        assert sorted(ref["info_out"][0][g0:].tolist()) == [0, 0, 5]
    assert {b for _, bp, sizes, g0, _ in R.FINISH_CASES if bp == 192 for b in sizes[g0:]} == {129, 130, 191, 192}


@pytest.mark.parametrize("p", R.TAIL_P)
def test_preconditions_of_the_tail_cases(p):
    mats = [R.spd(600 + g, b) for g, b in enumerate(R.TAIL_SIZES)]
    case = R.tail_case(610, R.TAIL_N, R.TAIL_BP, R.TAIL_SIZES, mats)
    for g in range(3):
        ref, kappa, cond1 = R.tail_reference(case, g)           # (asserts the condition cap)
        assert ref is not None and cond1 <= R.COND1_MAX and kappa > 0
        assert all(np.all(np.isfinite(v)) for v in ref.values())
    bad = list(mats)
    bad[1] = R.make_indefinite(mats[1], p)
    ref, _, pivot = R.tail_reference(R.tail_case(610, R.TAIL_N, R.TAIL_BP, R.TAIL_SIZES, bad), 1)
    assert ref is None and pivot == p
    # the margin: the failed pivot is negative by more than the largest diagonal entry
    Rg, _ = R.cholesky_ld(mats[1])
    dmax = float(np.max(np.diag(mats[1])))
    assert float(Rg[p - 1, p - 1]) ** 2 - 2 * dmax <= -dmax
