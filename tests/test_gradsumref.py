"""tests/gradsumref.py and gradref.value_and_gradients_matern, checked on the host before they judge the device
(tests/test_gpu_grad_sums.py): against the references the suite already trusts (gradref's LAPACK forms, the mpmath-derived
fixtures of golden_v3.npz), against 50-digit arithmetic, and every input builder of the GPU tests against the
preconditions its case states.  No device, no oracle."""
import os

import numpy as np
import pytest
import scipy.linalg as sl

import gradref
import gradsumref as R
from madaiemulator_amd import synth

LD = np.longdouble
HERE = os.path.dirname(os.path.abspath(__file__))


def test_longdouble_has_a_64_bit_mantissa():
    assert np.finfo(LD).nmant >= 63


def test_summed_slots_reproduce_the_lapack_gradients_n130():
    """A = LAPACK's inverse of gradref's matrix, z = A [y|H]: the summed literal and exact slots, through the host scalings
    of the collect half, are gradref's two gradient vectors at 1e-12"""
    N, d, order = 130, 3, 1
    X, y = synth.design(N, d, 1301)
    th = np.array([0.0, -3.0, np.log(0.6), np.log(0.75), np.log(0.5)])
    ref = gradref.value_and_gradients(X, y, order, th)
    Cm, _ = gradref.powexp_matrix(X, th)
    A, _ = gradref._inverse(Cm)
    H = gradref.hmatrix(order, X)
    z = A @ np.column_stack([y, H])
    gram = np.column_stack([y, H]).T @ z
    lit = R.literal(X, th, A, z)
    got = R.collect(1, d, 0, lit.sums, th, sigma2=LD(ref["sigma2"])).astype(float)
    assert np.max(np.abs(got - ref["literal"])) < 1e-12 * np.max(np.abs(ref["literal"])), (got, ref["literal"])
    for gram_dist in (False, True):
        exa = R.exact(1, X, th, A, z, gram=gram, gram_dist=gram_dist)
        got = R.collect(1, d, 1, exa.sums, th).astype(float)
        assert np.max(np.abs(got - ref["exact"])) < 1e-12 * np.max(np.abs(ref["exact"])), (got, ref["exact"])
        assert np.max(np.abs(exa.beta.astype(float) - ref["beta"])) < 1e-9 * np.max(np.abs(ref["beta"]))
        assert np.all(np.isnan(exa.val[:, d + 1:].astype(float))) and exa.defined == list(range(d + 1))
    assert lit.defined == list(range(2 * d + 2)) and len(R.tile_list(N)) == 6
    assert R.tile_list(200)[4] == (2, 1) and R.tile_list(200)[2 * 3 // 2 + 1] == (2, 1)      # t = tr (tr + 1) / 2 + tc


def _mpf(g):
    """a longdouble as the mpmath number it is: mantissa (its float64 head plus the rest, both exact) and exponent"""
    import mpmath as mp
    m, e = np.frexp(g)
    hi = float(m)
    return mp.ldexp(mp.mpf(hi) + mp.mpf(float(m - LD(hi))), int(e))


def _mp_pairs():
    """a dozen pairs of 3-d points: ordinary, far (exp argument beyond -700 at the short scales), 5e-11 apart, identical"""
    X = synth.uniform(4711, (12, 3))
    Y = synth.uniform(4712, (12, 3))
    Y[0] = X[0]                       # the same point under either rule
    Y[1] = X[1] + 5e-11               # same point for pow-exp, not for Matern
    Y[2] = X[2] + 3e-9
    X[3], Y[3] = np.array([0.01, 0.02, 0.03]), np.array([0.99, 0.97, 0.98])          # a far pair
    return X, Y


@pytest.mark.parametrize("kind,scale", [(1, 0.6), (1, 0.02), (2, 0.6), (2, 0.02), (3, 0.6), (3, 0.02)])
def test_single_summands_against_mpmath_at_50_digits(kind, scale):
    import mpmath as mp
    mp.mp.dps = 50
    f = mp.mpf
    X, Y = _mp_pairs()
    d = 3
    th = R.thetas_at(kind, d, scale, amp=0.25)
    amp = mp.exp(f(th[0]))
    worst = 0.0
    farthest = 0.0
    for i in range(X.shape[0]):
        D = R.diffs(X[i:i + 1], Y[i:i + 1])
        Dm = [f(float(X[i, k])) - f(float(Y[i, k])) for k in range(d)]
        u2 = R.scaled_sq_dist(kind, D, th)
        got, arg = R.exact_kernel_factor(kind, u2, np.exp(LD(th[0])))
        if kind == 1:
            e = sum(f(-0.5) * Dm[k] ** 2 * mp.exp(f(-2) * f(float(th[2 + k]))) for k in range(d))
            want, warg = amp * mp.exp(e), e
        else:
            s = mp.sqrt(sum(v * v for v in Dm)) / mp.exp(f(float(th[2])))
            c = f(1.732050808) if kind == 2 else f(2.236067978)
            warg = -c * s
            want = amp * c * c * s * s * mp.exp(warg) if kind == 2 else \
                amp * (s * s * (c * c - f(10) / 3) + (f(5) / 3) * c * s ** 3) * mp.exp(warg)
        farthest = min(farthest, float(warg))
        # longdouble: 2^-64 per operation, and the exp inherits 2^-64 |argument| from its argument
        tol = 64 * 2.0 ** -64 * (1.0 + abs(float(warg)))
        for g, w in ((got[0, 0], want), (arg[0, 0], warg)):
            err = abs(_mpf(g) - w)
            if w != 0:
                worst = max(worst, float(err / abs(w)) / tol)
                assert err <= tol * abs(w), (kind, scale, i, g, w)
            else:
                assert g == 0
        if kind == 1:
            for k, (dc, la) in enumerate(R.literal_dc(D, th)):
                e2 = mp.exp(f(-2) * f(float(th[2 + k])))
                wl = e2 * Dm[k] ** 2 * mp.exp(f(-0.5) * e2 * Dm[k] ** 2)
                gl = _mpf(dc[0, 0])
                assert abs(gl - wl) <= 64 * 2.0 ** -64 * (1.0 + abs(float(la[0, 0]))) * abs(wl), (k, i, gl, wl)
        same = bool(R.same_point(kind, np.vstack([X[i], Y[i]]))[0, 1])
        assert same == (i == 0 or (i == 1 and kind == 1)), (kind, i)
    # the far pair: beyond the literal kernel's clamp for pow-exp at the short scale, deep in the tail for the Matern kernels
    assert farthest < (-700.0 if kind == 1 else -100.0) if scale == 0.02 else farthest > -20.0
    print(f"kind {kind} scale {scale}: worst error / tolerance {worst:.2e}")


def test_matern_reference_reproduces_the_mpmath_fixtures():
    f = np.load(os.path.join(HERE, "golden", "golden_v3.npz"))
    X, y = f["X"], f["y"]
    seen = set()
    for i in range(int(f["ncases"])):
        kind, order, th = int(f[f"kind{i}"]), int(f[f"order{i}"]), f[f"th{i}"]
        if kind == 1:
            continue
        seen.add(kind)
        ref = gradref.value_and_gradients_matern(kind, X, y, order, th)
        want = f[f"grad{i}"]
        assert ref["value"] == pytest.approx(float(f[f"value{i}"]), rel=1e-8)
        assert np.max(np.abs(ref["exact"] - want)) < 1e-8 * np.max(np.abs(want)), (i, ref["exact"], want)
        assert np.all(ref["scale"] >= np.abs(ref["exact"]))
    assert seen == {2, 3}


# ---------------------------------------------------------------------------- the GPU tests' input builders
def test_operands_are_what_they_say():
    a, z, gram = R.operands(65, 4, 7, nb=3)
    for v in (a, z):
        assert np.all((np.abs(v) >= 0.5) & (np.abs(v) < 1.5)) and (v < 0).any() and (v > 0).any()
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(z[1], z[2])
    for nreg in (1, 2, 10, 63):
        g = R.operands(8, nreg, 11)[2][0]
        B = g[1:, 1:]
        assert np.array_equal(B, B.T) and np.linalg.eigvalsh(B).min() > 0 and np.linalg.cond(B) < 4.0
    for nreg in (1, 4, 63):
        a, z, gram, beta = R.integer_operands(70, nreg, 3, nb=2)
        for v in (a, z, beta):
            assert np.array_equal(v, np.round(v)) and np.abs(v).max() <= 8
        for b in range(2):
            assert np.array_equal(R.solve_beta(gram[b]).astype(float), beta[b])
            assert np.array_equal(np.linalg.solve(gram[b][1:, 1:], gram[b][1:, 0]), beta[b])


@pytest.mark.parametrize("name", sorted(R.NUGGET_CASES))
def test_nugget_pairs_land_where_the_case_says(name):
    X, pairs = R.nugget_design(name)
    N = X.shape[0]
    tiles = R.tile_list(N)
    for kind in (1, 3):
        same = R.same_point(kind, X)
        off = [(i, j) for i in range(N) for j in range(i) if same[i, j]]
        (i, j, gap), = pairs
        lo, hi = min(i, j), max(i, j)
        want_same = gap == 0.0 or (gap < 1e-10 and kind == 1)
        assert off == ([(hi, lo)] if want_same else []), (name, kind, off)
    tr, tc = hi // 64, lo // 64
    if "within_one_tile" in name:
        assert tr == tc
    if "across_two_tiles" in name:
        assert tr != tc and (tr, tc) in tiles
    if "last_ragged" in name:
        assert tr == tc == (N - 1) // 64 and N % 64 != 0
    # in the Gram form these pairs are candidates: their squared scaled distance is below the form's own error bound
    for kind, scale in ((1, 0.6), (3, 0.02)):
        th = R.thetas_at(kind, 3, scale)
        u2 = R.scaled_sq_dist(kind, R.diffs(X[hi:hi + 1], X[lo:lo + 1]), th)[0, 0]
        assert u2 <= R.gram_delta(kind, X, th)


def test_every_bar_is_positive_and_the_clamp_cases_clamp():
    N, d = 200, 3
    X = synth.design(N, d, 611)[0]
    a, z, gram = R.operands(N, 1, 5)
    for scale, clamped in ((0.6, False), (0.02, True), (0.005, True)):
        th = R.thetas_at(1, d, scale, step=0.0)
        lit = R.literal(X, th, a[0], z[0])
        args = np.array([np.min(arg.astype(float)) for _, arg in R.literal_dc(R.diffs(X), th)])
        assert R.production_noclamp(X, th) == (not clamped)
        if clamped:
            assert args.min() < -700.0               # the clamp does something in this case
        else:
            assert args.min() > -600.0               # and here the unclamped exp is inside its domain
        diag = np.array([tr == tc for tr, tc in R.tile_list(N)])
        bar = lit.bar.astype(float)
        assert np.all(bar[:, :2 * d] > 0) and np.all(bar[diag, 2 * d:] > 0) and np.all(bar[~diag, 2 * d:] == 0)
        assert np.all(lit.sums_bar.astype(float) > 0)
    for kind in (1, 2, 3):
        for scale in (0.6, 0.08, 0.02):
            th = R.thetas_at(kind, d, scale)
            for gd in (False, True):
                e = R.exact(kind, X, th, a[0], z[0], gram=gram[0], gram_dist=gd)
                nd = d if kind == 1 else 1
                assert np.all(e.bar[:, :nd].astype(float) > 0) and np.all(e.bar[diag, nd].astype(float) > 0)
                assert np.all(e.bar[~diag, nd].astype(float) == 0)       # no coinciding pair off the diagonal here


def test_interior_tiles_of_n200_are_the_three_the_cases_name():
    N = 200
    interior = [(tr, tc) for tr, tc in R.tile_list(N) if tr > tc and tr * 64 + 63 < N and tc * 64 + 63 < N]
    assert interior == [(1, 0), (2, 0), (2, 1)] and N - 3 * 64 == 8


@pytest.mark.parametrize("kind,N,d", [(1, 200, 3), (2, 200, 3), (3, 200, 3), (1, 200, 7), (1, 200, 9), (1, 200, 16), (3, 200, 16),
                                      (1, 130, 33), (3, 130, 33), (1, 130, 60)])
def test_gram_form_shapes_with_held_exponents_are_the_listed_ones(kind, N, d):
    """where grad_exact_gram_kernel's held exponent can put more into a tile than the tile's bar (gradsumref.gram_hold_u2):
    exactly the shapes of GRAM_HELD_SHAPES, which the GPU tests treat apart; everywhere else the hold is below the bar"""
    X = synth.design(N, d, 800 + N + d)[0]
    a, z, gram = R.operands(N, 4 if d == 3 else 1, 30 * N + d + kind)
    nd = d if kind == 1 else 1
    for scale in (0.6, 0.08, 0.02):
        e = R.exact(kind, X, R.thetas_at(kind, d, scale, step=0.02, amp=-0.5), a[0], z[0], gram=gram[0], gram_dist=True)
        assert bool(np.any(e.hold[:, :nd] > e.bar[:, :nd])) == ((kind, N, d, scale) in R.GRAM_HELD_SHAPES), (kind, N, d, scale)
        assert np.all(e.hold[:, nd:] == 0)
