"""The reference of the covariance fill tests (tests/covref.py) on the CPU: its elements against the oracle's covariance
functions, its image builder on a case small enough to write down, and the conditions the inputs of
tests/test_gpu_fill_launch.py have to meet -- room under the bar in the fp64 model of the Gram form, no k-vector element at
the clamp, every entry of the exp table reached.  No GPU needed."""
import numpy as np
import pytest

import covref as R
from madaiemulator_amd import synth
from oracle import oracle as O

U = 2.0 ** -53


def ulps_off(got, ref, arg):
    """|fp64 got - ref| in units of the rounding an fp64 evaluation carries: a few roundings of the value, and the
    argument's own (each of its d terms is rounded) times |argument|"""
    return float(np.max(np.abs(got.astype(R.LD) - ref) / ((1.0 + np.abs(arg)) * U * np.abs(ref))))


@pytest.mark.parametrize("kind", [1, 2, 3])
@pytest.mark.parametrize("N,d", [(40, 1), (33, 3), (20, 16)])
def test_elements_against_the_oracle(kind, N, d):
    X = synth.design(N, d, 4100 + N + d)[0]
    X[7] = X[3]                                         # a duplicated point: off-diagonal nugget
    th = R.thetas_for_norm2(kind, X, 3.0)
    ref, arg = R.elements(kind, X, X, th)
    assert ref[7, 3] == ref[3, 3] and ref[3, 7] > ref[3, 8] + 0.5 * R.amp_nug(kind, th)[1]
    assert ulps_off(O.cov_matrix(kind, X, th), ref, arg) < 8.0
    Xq = np.vstack([synth.queries(9, d, 5), X[:2], X[4:5] + 30.0])
    th = R.thetas_for_norm2(kind, X, 15.0)              # short scales: part of the k-vectors falls below the clamp
    kref, karg = R.elements(kind, Xq, X, th, clamp=True)
    kora = np.vstack([O.kvector(kind, X, q, th) for q in Xq])
    assert np.array_equal(kora == 0.0, kref == 0) and (kref == 0).sum() > (0 if d == 1 else 5) and np.all(kref[-1] == 0)
    nz = kref != 0
    assert ulps_off(kora[nz], kref[nz], karg[nz]) < 8.0


def test_special_pairs_against_the_oracle(golden):
    """identical points, |delta| = 5e-11 / 2e-10 (the pow-exp threshold), 5e-17 (Matern), far points: the nugget where the
    oracle puts it"""
    n = 0
    for x, y, kind, d, th in zip(golden["g1_x"], golden["g1_y"], golden["g1_kind"], golden["g1_d"], golden["g1_th"]):
        kind, d = int(kind), int(d)
        th = th[:O.nthetas_for(kind, d)]
        ref, arg = R.elements(kind, x[None, :d], y[None, :d], th)
        got = np.array([[O.cov(kind, x[:d], y[:d], th)]])
        if ref[0, 0] > 1e-300:
            assert ulps_off(got, ref, arg) < 8.0, (kind, x[:d], y[:d])
        else:
            assert got[0, 0] < 1e-290
        n += 1
    assert n >= 6


def test_matern_log_mode_exponentiates_amplitude_and_nugget():
    X = synth.design(5, 2, 1)[0]
    th = np.array([0.3, -2.0, np.log(0.7)])
    for kind in (2, 3):
        a, _ = R.elements(kind, X, X, th, matern_log=True)
        b, _ = R.elements(kind, X, X, np.array([np.exp(0.3), np.exp(-2.0), th[2]]))
        assert np.max(np.abs(a - b) / b) < 4 * U


def test_staged_image_of_a_two_tile_row_case():
    """N = 65, d = 1, pow-exp, written down by hand: Np = 128, lower tiles (0,0) (1,0) (1,1), tile (0,1) above the diagonal"""
    N, Np, Rp, guard = 65, 128, 70, 2
    X = (np.arange(N, dtype=np.float64) / 64.0).reshape(N, 1)
    th = np.array([np.log(2.0), np.log(0.5), 0.0])                # amp 2, nugget 1/2, length scale 1
    pre = -1.0 - np.arange(2 * (Np + Rp + guard) * Np, dtype=np.float64).reshape(2, Np + Rp + guard, Np)
    rr = 100.0 + np.arange(2 * Rp * Np, dtype=np.float64)
    img = R.staged_image(1, X, np.array([th, th]), pre, rr, rstride=Rp * Np, Rp=Rp, guard=guard)
    for b in range(2):
        w, e, wr = img.want[b], img.elem[b], img.written[b]
        assert float(w[0, 0]) == 2.5 and float(w[64, 64]) == 2.5 and e[0, 0] and e[64, 64]
        assert abs(float(w[64, 0]) - 2.0 * np.exp(-0.5)) < 1e-15 and e[64, 0] and float(img.arg[b][64, 0]) == -0.5
        assert abs(float(w[10, 2]) - 2.0 * np.exp(-0.5 * (8.0 / 64.0) ** 2)) < 1e-15 and e[10, 2]
        assert e[2, 10] and float(w[2, 10]) == float(w[10, 2])                 # the whole diagonal tile is written
        assert w[3, 64] == pre[b, 3, 64] and w[63, 127] == pre[b, 63, 127]     # tile (0, 1): the prefill
        assert not wr[:64, 64:].any() and wr[:64, :64].all() and wr[64:128, :].all()
        assert not e[:64, 64:].any() and not e[65:Np].any() and not e[:, 65:].any() and e[:65, :65][np.tril_indices(65)].all()
        assert w[65, 65] == 1.0 and w[127, 127] == 1.0 and w[65, 64] == 0.0 and w[64, 65] == 0.0 and w[100, 3] == 0.0
        assert np.array_equal(w[Np:Np + Rp].astype(np.float64).ravel(), rr[b * Rp * Np:(b + 1) * Rp * Np])
        assert wr[Np:Np + Rp].all() and not wr[Np + Rp:].any()
        assert np.array_equal(w[Np + Rp:].astype(np.float64), pre[b, Np + Rp:])
    got = img.want.astype(np.float64)
    worst, nbad = img.check(got)
    assert nbad == 0 and worst < 1e-2                            # (the image itself, rounded to fp64)
    got[1, 3, 64] = 0.0                                           # a write above the diagonal
    got[0, Np + Rp, 5] = 0.0                                      # a write into the guard rows
    got[0, 65, 64] = 1e-300                                       # padding that is not zero
    assert img.check(got)[1] == 3
    got = img.want.astype(np.float64)
    got[0, 64, 0] *= 1.0 + 2.2e-13
    assert img.check(got)[0] > 2.0


def test_kvector_and_full_images():
    X = synth.design(3, 2, 3)[0]
    Xq = np.vstack([X[1], [0.2, 0.3]])
    th = np.array([0.0, -1.0, np.log(0.05), np.log(0.05)])
    pre = np.full((64 + 1, 64), np.nan)
    img = R.kvec_image(1, X, Xq, th, pre, guard=1)
    v = img.want[:2, :3].astype(np.float64)
    assert v[0, 1] == pytest.approx(1.0 + np.exp(-1.0)) and (v == 0).sum() >= 1
    assert np.array_equal(img.elem[:2, :3], v != 0) and img.elem.sum() == (v != 0).sum()
    assert np.all(img.want[:64, 3:] == 0) and np.all(img.want[2:64] == 0) and np.all(np.isnan(img.want[64].astype(np.float64)))
    got = np.where(img.written, img.want.astype(np.float64), pre)
    assert img.check(got)[1] == 0
    got[64, 0] = 0.0
    assert img.check(got)[1] == 1
    full = R.full_image(1, X, th, np.full((64, 64), np.nan))
    assert full.elem[:3, :3].all() and full.elem.sum() == 9 and np.all(full.want[3:] == 0) and np.all(full.want[:, 3:] == 0)


# ------------------------------------------------------------------ conditions on the inputs of the GPU tests
GRAM_INPUTS = list(R.gram_inputs())


def test_gpu_inputs_are_admitted_where_they_should_be():
    for label, kind, X, th, _ in GRAM_INPUTS:
        assert R.norm2(kind, X, th) <= R.ADMIT, label
    for kind in (1, 2, 3):
        for N, d in R.BOUNDARY_SHAPES:
            Xu, tu = R.boundary_case(kind, N, d, R.JUST_UNDER)
            Xo, to = R.boundary_case(kind, N, d, R.JUST_OVER)
            assert 16.0 * (1 - 2e-3) < R.norm2(kind, Xu, tu) < 16.0 * (1 - 5e-4)
            assert 16.0 * (1 + 5e-4) < R.norm2(kind, Xo, to) < 16.0 * (1 + 2e-3)
            # corner-clustered: every centred, scaled point is close to the bound itself
            w = R.scales(kind, d, tu)
            assert np.min((((Xu - 0.5) * w) ** 2).sum(axis=1)) > 0.9 * R.JUST_UNDER
            m = [R.norm2(kind, Xu, t) <= R.ADMIT for t in R.mixed_thetas(kind, Xu)]
            assert m == [True, False, True, False, True]


@pytest.mark.parametrize("kind", [1, 2, 3])
def test_gram_model_leaves_half_the_bar(kind):
    """the fp64 model of the Gram-form distance, at every design and theta the GPU tests send through that form: its
    elements stay under HALF the bar, so a device that computes what the model computes has room"""
    worst = 0.0
    for label, k, X, th, Xq in GRAM_INPUTS:
        if k != kind:
            continue
        r = R.gram_model_ratio(kind, X, th, Xq=Xq)
        print(f"kind {kind} {label}: model error / bar {r:.3f}")
        worst = max(worst, r)
        assert r < 0.5, (label, r)
    print(f"kind {kind}: worst model error / bar {worst:.3f}")


def test_no_kvector_element_lies_at_the_clamp():
    """the zero pattern of a k-vector may then be required to equal the reference's with no element left out"""
    for kind in (1, 2, 3):
        for N, d in R.KVEC_SHAPES:
            for M in R.KVEC_M:
                X, th, Xq = R.kvec_case(kind, N, d, M)
                assert R.clamp_margin(kind, X, Xq, th) > 1e-12, (kind, N, d, M)
                v, _ = R.elements(kind, Xq, X, th, clamp=True)
                if M > 1 and kind == 1:
                    assert (v == 0).sum() > 100 and (v != 0).sum() > 100


def test_kvector_rows_straddle_the_far_test():
    for kind in (1, 2, 3):
        for N, d in R.KVEC_SHAPES:
            X, th, Xq = R.kvec_case(kind, N, d, 65)
            n = (((Xq - 0.5) * R.scales(kind, d, th)) ** 2).sum(axis=1)
            assert 16.0 * (1 - 2e-3) < n[17] < 16.0 * (1 - 5e-4) and 16.0 * (1 + 5e-4) < n[33] < 16.0 * (1 + 2e-3) and n[50] > 1e3
            assert np.array_equal(Xq[3], X[5]) and np.array_equal(Xq[64], X[0])


def test_pair_designs_put_the_nugget_where_their_names_say():
    for kind in (1, 2, 3):
        for name in R.PAIR_OFFSETS[kind]:
            X = R.pair_design(kind, name)
            same = R.same_point(kind, X)
            want = name in ("duplicate", "all_5e-11", "all_5e-17")
            for i, j in R.PAIR_SPOTS.values():
                assert same[j, i] == want and same[i, j] == want, (kind, name, i, j)
                assert name == "duplicate" or np.all(X[j] != X[i])
            assert same.sum() == R.PAIR_N + (2 * len(R.PAIR_SPOTS) if want else 0)
    tiles = {(j // 64, i // 64, j // 16 == i // 16) for i, j in R.PAIR_SPOTS.values()}
    assert {(0, 0, True), (0, 0, False), (1, 0, False), (1, 1, False), (2, 0, False), (2, 2, False)} <= tiles


def test_ladder_sits_at_the_far_corner():
    for d in (4, 16):
        X = R.ladder_design(d)
        assert np.all(X[0] == 1.0) and X.max() == 1.0 and X.min() == 0.0
        D = X[0] - X[2:2 + 2 * len(R.LADDER)]
        assert np.allclose(D[:8, 0], R.LADDER, rtol=1e-6) and np.all(D[:8, 1:] == 0)
        assert np.allclose(D[8:], np.array(R.LADDER)[:, None], rtol=1e-6)


def test_table_case_reaches_every_entry_of_the_exp_table():
    X, th = R.table_design()
    assert R.norm2(1, X, th) <= R.ADMIT
    _, arg = R.elements(1, X, X, th)
    low = np.tril_indices(X.shape[0], -1)
    idx, octave = R.table_indices(arg[low])
    assert len(np.unique(idx)) == 1024
    assert arg.min() > -64.0 and len(np.unique(octave)) >= 80          # 64 / ln 2 = 92 octaves in all
