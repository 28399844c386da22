"""The gradient's reduction kernels (gather_alpha_kernel, beta_solve_kernel, grad_part_kernel<CLAMP>, grad_exact_kernel<KIND>,
grad_exact_gram_kernel<KIND>, grad_reduce_kernel) through gpemu_test_grad_sums -- production's routine on caller-chosen
corners -- against tests/gradsumref.py: every element of a batch, every tile, every slot the form defines against ITS OWN
bar (sum tau |summand| + n u M, derived in gradsumref's header, never fitted to the device), and the second-stage sums.
a and z are random in +-[0.5, 1.5): no inverse, so no tile's share is small.  Every corner element the kernels must not
read is NaN and every output starts as NaN: a defined output that is not finite is a failure, and what a form does not
define must come back NaN.  Each test prints the worst error / bar of its kernel form.

Then the same kernels end to end through the public API where the suite had no outside number: the literal gradient with
the clamped exp (alone and as one element of a batch), and Matern exact gradients across several tiles."""
import numpy as np
import pytest
import scipy.linalg as sl
from scipy.linalg import lapack

import gradref
import gradsumref as R
from madaiemulator_amd import abi, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 130, 200, 256)
U = 2.0 ** -53
RTOL = 1e-8
COND_MAX = 5e6
MATERN_MODES = abi.MODE_EXACT_GRAD | abi.MODE_MATERN_LOG


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(0)
    yield c
    c.close()


def _ctx_with_env(monkeypatch, env):
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    c = abi.Context(0)
    for k_ in env:
        monkeypatch.delenv(k_)
    return c


def set_model(c, kind, X, order=0):
    c.set_mode(MATERN_MODES if kind != 1 else 0)
    c.set_model(kind, order, X, np.zeros(X.shape[0]))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def check_slots(what, got, b, ref):
    """element b of a device result against its reference: every tile and every defined slot against its own bar, the
    second-stage sums against theirs, undefined slots NaN -> the worst error / bar"""
    part, sums = got["part"][b], got["sums"][b]
    s = ref.defined
    undefined = [k for k in range(part.shape[1]) if k not in s]
    assert np.all(np.isfinite(part[:, s])) and np.all(np.isfinite(sums[s])), (what, b, "a defined output is not finite")
    assert np.all(np.isnan(part[:, undefined])), (what, b, "a slot the form does not define was written")
    worst = 0.0
    for name, g, val, bar in (("tile", part[:, s], ref.val[:, s], ref.bar[:, s]), ("sum", sums[s], ref.sums[s], ref.sums_bar[s])):
        err = np.abs(g.astype(R.LD) - val)
        zero = bar == 0
        assert np.all(g[zero] == 0.0), (what, b, name, "a slot without summands is not zero")
        ratio = np.where(zero, R.LD(0.0), err / np.where(zero, R.LD(1.0), bar)).astype(float)
        if ratio.max() > 1.0:
            i = np.unravel_index(np.argmax(ratio), ratio.shape)
            print(f"{what} element {b}: {name} {i} (tile, slot index) got {g[i]!r} want {val[i]!r} error/bar {ratio[i]:.3e}")
        worst = max(worst, float(ratio.max()))
    return worst


def report(form, what, worst):
    print(f"{form}: {what}: worst error / bar {worst:.3f}")
    assert worst <= 1.0, (form, what, worst)


def run_literal(c, what, X, ths, a, z, clamp=-1):
    ths = np.atleast_2d(ths)
    got = c.test_grad_sums(ths, a, z, form=0, clamp=clamp)
    worst = 0.0
    for b in range(ths.shape[0]):
        ref = R.literal(X, ths[b], a[b], z[b])
        assert same_bits(got["alpha"][b], z[b][:, 0])
        worst = max(worst, check_slots(what, got, b, ref))
    return got, worst


def run_exact(c, what, kind, X, ths, a, z, gram, gram_dist):
    ths = np.atleast_2d(ths)
    got = c.test_grad_sums(ths, a, z, gram, form=1, gram_dist=gram_dist)
    worst = 0.0
    for b in range(ths.shape[0]):
        ref = R.exact(kind, X, ths[b], a[b], z[b], gram=gram[b], gram_dist=bool(gram_dist))
        assert np.all(np.isfinite(got["alpha"][b])) and np.all(np.isfinite(got["beta"][b]))
        worst = max(worst, check_slots(what, got, b, ref))
    return got, worst


# ------------------------------------------------------------------ literal form
@pytest.mark.parametrize("N,d", [(N, 3) for N in SIZES] + [(200, d) for d in (1, 4, 5, 9)] + [(130, 33), (130, 60)])
def test_literal_tiles_unclamped_and_forced_clamp_same_bits(ctx, N, d):
    """grad_part_kernel<false> (production's choice at ordinary scales) per tile, and <true> forced on the same operands:
    the same arithmetic while every exp argument stays above -700, so the same bits.  d = 60 is where the kernel's dynamic
    LDS passes 64 KB (128 (d + 1) + 1344 doubles) and the launch has to raise the kernel's limit first"""
    X = synth.design(N, d, 500 + N + d)[0]
    set_model(ctx, 1, X)
    a, z, _ = R.operands(N, 1, 10 * N + d)
    th = R.thetas_at(1, d, 0.6)
    assert R.production_noclamp(X, th)
    got, worst = run_literal(ctx, f"literal N={N} d={d}", X, th, a, z)
    report("literal <false>", f"N={N} d={d}", worst)
    off = ctx.test_grad_sums(th, a, z, form=0, clamp=0)
    on = ctx.test_grad_sums(th, a, z, form=0, clamp=1)
    for k_ in ("part", "sums", "alpha"):
        assert same_bits(got[k_], off[k_]) and same_bits(got[k_], on[k_]), k_


@pytest.mark.parametrize("scale", [0.02, 0.005])
def test_literal_clamped_kernel_chosen_by_the_rule(ctx, scale):
    """length scales 0.02 and 0.005 on the unit cube: exp arguments far beyond -700, production's rule selects <true>"""
    N, d = 200, 3
    X = synth.design(N, d, 611)[0]
    set_model(ctx, 1, X)
    a, z, _ = R.operands(N, 1, 77)
    th = R.thetas_at(1, d, scale, step=0.0)
    assert not R.production_noclamp(X, th)
    got, worst = run_literal(ctx, f"literal clamped scale {scale}", X, th, a, z)
    report("literal <true>", f"scale {scale}", worst)
    assert all(same_bits(got[k_], ctx.test_grad_sums(th, a, z, form=0, clamp=1)[k_]) for k_ in ("part", "sums"))


def test_literal_batch_elements_keep_their_bits(ctx):
    """nb = 3 with three thetas, three a, three z: every element is its own nb = 1 run bit for bit; then element 1
    short-scaled: the rule sends the whole chunk to <true> and elements 0 and 2 keep the bits of their <false> runs"""
    N, d = 200, 3
    X = synth.design(N, d, 612)[0]
    set_model(ctx, 1, X)
    a, z, _ = R.operands(N, 1, 78, nb=3)
    ths = np.array([R.thetas_at(1, d, s) for s in (0.6, 0.45, 0.8)])
    got, worst = run_literal(ctx, "literal batch", X, ths, a, z)
    report("literal <false>", "batch of 3", worst)
    ones = [ctx.test_grad_sums(ths[b], a[b], z[b], form=0, clamp=0) for b in range(3)]
    for b in range(3):
        assert all(same_bits(got[k_][b], ones[b][k_][0]) for k_ in ("part", "sums", "alpha")), b
    mixed = ths.copy()
    mixed[1] = R.thetas_at(1, d, 0.02, step=0.0)
    assert not R.production_noclamp(X, mixed) and R.production_noclamp(X, mixed[[0, 2]])
    gm, worst = run_literal(ctx, "literal mixed batch", X, mixed, a, z)
    report("literal <true>", "batch with one short-scaled element", worst)
    for b in (0, 2):
        assert all(same_bits(gm[k_][b], ones[b][k_][0]) for k_ in ("part", "sums", "alpha")), b
    with pytest.raises(abi.GpemuError):
        ctx.test_grad_sums(mixed, a, z, form=0, clamp=0)


# ------------------------------------------------------------------ exact form
DIFF_CASES = [(k, N, 3) for k in (1, 2, 3) for N in SIZES] + [(1, 200, d) for d in (15, 16, 17)] + [(2, 200, 16), (3, 200, 17)] + \
             [(k, 130, 33) for k in (1, 3)] + [(1, 130, 60)]


@pytest.mark.parametrize("kind,N,d", DIFF_CASES)
def test_exact_difference_form_tiles(ctx, kind, N, d):
    X = synth.design(N, d, 700 + N + d)[0]
    order = 1 if d == 3 else 0
    set_model(ctx, kind, X, order)
    a, z, gram = R.operands(N, ctx.nreg, 20 * N + d + kind)
    th = R.thetas_at(kind, d, 0.6, step=0.02, amp=0.25)
    _, worst = run_exact(ctx, f"exact kind {kind} N={N} d={d}", kind, X, th, a, z, gram, 0)
    report(f"exact difference form kind {kind}", f"N={N} d={d}", worst)


GRAM_CASES = [(k, N, 3) for k in (1, 2, 3) for N in SIZES] + [(1, 200, d) for d in (7, 8, 9, 16)] + [(2, 200, 9), (3, 200, 16)] + \
             [(k, 130, 33) for k in (1, 3)] + [(1, 130, 60)]


@pytest.mark.parametrize("kind,N,d", GRAM_CASES)
def test_exact_gram_form_tiles_at_three_length_scales(ctx, kind, N, d):
    X = synth.design(N, d, 800 + N + d)[0]
    order = 1 if d == 3 else 0
    set_model(ctx, kind, X, order)
    a, z, gram = R.operands(N, ctx.nreg, 30 * N + d + kind)
    for scale in (0.6, 0.08, 0.02):
        if (kind, N, d, scale) in R.GRAM_HELD_SHAPES:      # tiles of nothing but held exponents: the case below
            continue
        th = R.thetas_at(kind, d, scale, step=0.02, amp=-0.5)
        ref = R.exact(kind, X, th, a[0], z[0], gram=gram[0], gram_dist=True)
        assert np.all(ref.hold <= np.where(np.isnan(ref.bar), np.inf, ref.bar))       # the bar's precondition (gradsumref.gram_hold_u2)
        _, worst = run_exact(ctx, f"gram kind {kind} N={N} d={d} scale {scale}", kind, X, th, a, z, gram, 1)
        report(f"exact Gram form kind {kind}", f"N={N} d={d} scale {scale}", worst)


@pytest.mark.parametrize("kind,N,d,scale", sorted(R.GRAM_HELD_SHAPES))
def test_exact_gram_form_where_the_exponent_is_held(ctx, kind, N, d, scale):
    """pow-exp, d = 16, 33 and 60 at scale 0.02: off the diagonal every exponent is beyond -600, where
    grad_exact_gram_kernel holds it (its comment: weights beyond that are 1e-261 of the amplitude either way).  The true
    length sums of whole tiles, 1e-571 and less, are no fp64 numbers, so no result meets a bar relative to them; these
    shapes are allowed bar + hold, hold = the sum over the tile's held pairs of amp e^-600 w |W| D_k^2 e^{-2 t_k}
    (gradsumref.gram_hold_u2; test_gradsumref.py checks that exactly these shapes need it).  The nugget slot has no
    exponent and keeps its bar.  Measured: sums of 2e-257 to 8e-257."""
    X = synth.design(N, d, 800 + N + d)[0]
    set_model(ctx, kind, X, 0)
    a, z, gram = R.operands(N, ctx.nreg, 30 * N + d + kind)
    th = R.thetas_at(kind, d, scale, step=0.02, amp=-0.5)
    got = ctx.test_grad_sums(th, a, z, gram, form=1, gram_dist=1)
    ref = R.exact(kind, X, th, a[0], z[0], gram=gram[0], gram_dist=True)
    assert np.any(ref.hold[:, :d] > ref.bar[:, :d]) and np.all(ref.hold[:, d] == 0)
    part, sums, s_ = got["part"][0], got["sums"][0], ref.defined
    assert np.all(np.isfinite(part[:, s_])) and np.all(np.isfinite(sums[s_])) and np.all(np.isnan(part[:, d + 1:]))
    err = np.abs(part[:, s_].astype(R.LD) - ref.val[:, s_])
    assert np.all(err <= ref.bar[:, s_] + ref.hold[:, s_]), np.argwhere(err > ref.bar[:, s_] + ref.hold[:, s_])
    errs = np.abs(sums[s_].astype(R.LD) - ref.sums[s_])
    assert np.all(errs <= ref.sums_bar[s_] + ref.hold[:, s_].sum(axis=0))
    print(f"exact Gram form kind {kind}: N={N} d={d} scale {scale}: largest |length sum| {np.max(np.abs(part[:, :d])):.3e}, "
          f"largest allowance {float(np.max(ref.bar[:, :d] + ref.hold[:, :d])):.3e}")


@pytest.mark.parametrize("kind", [1, 3])
@pytest.mark.parametrize("gram_dist", [0, 1])
def test_exact_batch_elements_keep_their_bits(ctx, kind, gram_dist):
    N, d = 200, 3
    X = synth.design(N, d, 613)[0]
    set_model(ctx, kind, X, 1)
    a, z, gram = R.operands(N, ctx.nreg, 79, nb=3)
    ths = np.array([R.thetas_at(kind, d, s, amp=amp) for s, amp in ((0.6, 0.0), (0.08, 0.3), (0.3, -0.2))])
    got, worst = run_exact(ctx, f"exact batch kind {kind}", kind, X, ths, a, z, gram, gram_dist)
    report(f"exact {'Gram' if gram_dist else 'difference'} form kind {kind}", "batch of 3", worst)
    for b in range(3):
        one = ctx.test_grad_sums(ths[b], a[b], z[b], gram[b], form=1, gram_dist=gram_dist)
        nd = d if kind == 1 else 1
        assert same_bits(got["part"][b][:, :nd + 1], one["part"][0][:, :nd + 1]) and same_bits(got["sums"][b][:nd + 1], one["sums"][0][:nd + 1])
        assert same_bits(got["alpha"][b], one["alpha"][0]) and same_bits(got["beta"][b], one["beta"][0])


@pytest.mark.parametrize("name", sorted(R.NUGGET_CASES))
@pytest.mark.parametrize("kind", [1, 3])
def test_nugget_rule_off_the_diagonal(ctx, name, kind):
    """coinciding and nearly coinciding rows: the nugget slot of every tile (the rule applies to every pair of the same
    point, not only i == j) and the length slots of those tiles -- in the Gram form the candidates' recompute path --, both
    distance forms"""
    X, pairs = R.nugget_design(name)
    N, d = X.shape
    set_model(ctx, kind, X, 1)
    a, z, gram = R.operands(N, ctx.nreg, 91 + kind)
    (i, j, gap), = pairs
    is_same = bool(R.same_point(kind, X)[max(i, j), min(i, j)])
    assert is_same == (gap == 0.0 or (gap < 1e-10 and kind == 1))
    for gram_dist in (0, 1):
        for scale in (0.6, 0.02):
            th = R.thetas_at(kind, d, scale, nugget=-1.0)
            got, worst = run_exact(ctx, f"nugget {name} kind {kind} gram {gram_dist}", kind, X, th, a, z, gram, gram_dist)
            report(f"exact {'Gram' if gram_dist else 'difference'} form kind {kind}", f"{name} scale {scale}", worst)
            ref = R.exact(kind, X, th, a[0], z[0], gram=gram[0], gram_dist=bool(gram_dist))
            t = R.tile_list(N).index((max(i, j) // 64, min(i, j) // 64))
            nd = d if kind == 1 else 1
            if is_same and i // 64 != j // 64:
                assert ref.val[t, nd] != 0 and got["part"][0][t, nd] != 0.0        # an off-diagonal tile with a nugget share


# ------------------------------------------------------------------ exact arithmetic: no tolerance
@pytest.mark.parametrize("N,d,order", [(200, 3, 0), (200, 3, 1), (65, 31, 2), (1500, 3, 1)])
def test_integer_operands_alpha_and_trace_slots_are_exact(ctx, N, d, order):
    """a, z, gram and beta integer-valued in [-8, 8] (gram chosen so that beta is the integer vector): alpha for nbeta = 0
    (literal form) and nbeta = nreg = 1, 4, 63 (exact form), the literal slots 2d and 2d + 1 of every tile and their
    second-stage sums must EQUAL the integer results.  N = 1500: 300 tiles, grad_reduce_kernel's stride loop makes a second
    pass"""
    X = synth.design(N, d, 900 + N)[0]
    set_model(ctx, 1, X, order)
    nreg = ctx.nreg
    assert nreg == {(200, 0): 1, (200, 1): 4, (65, 2): 63, (1500, 1): 4}[(N, order)]
    a, z, gram, beta = R.integer_operands(N, nreg, 40 + N + order, nb=2)
    ths = np.array([R.thetas_at(1, d, 0.6), R.thetas_at(1, d, 0.5)])
    lit = ctx.test_grad_sums(ths, a, z, form=0)
    exa = ctx.test_grad_sums(ths, a, z, gram, form=1, gram_dist=0)
    tiles = R.tile_list(N)
    assert len(tiles) == (300 if N == 1500 else len(tiles))
    for b in range(2):
        assert same_bits(lit["alpha"][b], z[b][:, 0])                                     # nbeta = 0
        assert np.array_equal(exa["beta"][b], beta[b])
        assert np.array_equal(exa["alpha"][b], z[b][:, 0] - z[b][:, 1:] @ beta[b])        # integers below 2^53: exact
        tr_want = np.array([np.trace(a[b][64 * tr:64 * tr + 64, 64 * tr:64 * tr + 64]) if tr == tc else 0.0 for tr, tc in tiles])
        aa_want = np.array([np.sum(z[b][64 * tr:64 * tr + 64, 0] ** 2) if tr == tc else 0.0 for tr, tc in tiles])
        assert np.array_equal(lit["part"][b][:, 2 * d], tr_want) and np.array_equal(lit["part"][b][:, 2 * d + 1], aa_want)
        assert lit["sums"][b][2 * d] == np.trace(a[b]) and lit["sums"][b][2 * d + 1] == np.sum(z[b][:, 0] ** 2)
        assert np.all(np.isfinite(lit["part"][b])) and np.all(np.isfinite(lit["sums"][b]))


# ------------------------------------------------------------------ beta_solve_kernel
@pytest.mark.parametrize("d,order", [(3, 0), (1, 1), (3, 3), (31, 2)])
def test_beta_against_lapack(ctx, d, order):
    """nreg = 1, 2, 10, 63: beta_out against LAPACK's Cholesky solve of the same matrix at cond_1 * nreg * 8u of the largest
    component, cond_1 from dpocon"""
    N = 70
    X = synth.design(N, d, 950 + d)[0]
    set_model(ctx, 1, X, order)
    nreg = ctx.nreg
    assert nreg == 1 + order * d and nreg in (1, 2, 10, 63)
    a, z, gram = R.operands(N, nreg, 60 + nreg, nb=2)
    got = ctx.test_grad_sums(np.array([R.thetas_at(1, d, 0.6)] * 2), a, z, gram, form=1, gram_dist=0)
    for b in range(2):
        B = gram[b][1:, 1:]
        cf = sl.cho_factor(B, lower=True)
        rcond, info = lapack.dpocon(cf[0], np.abs(B).sum(axis=0).max(), uplo="L")
        want = sl.cho_solve(cf, gram[b][1:, 0])
        err, bar = np.max(np.abs(got["beta"][b] - want)), (1.0 / rcond) * nreg * 8 * U * np.max(np.abs(want))
        print(f"beta_solve nreg={nreg} element {b}: error / bar {err / bar:.3f} (cond_1 {1.0 / rcond:.2f})")
        assert info == 0 and err <= bar


def test_regression_block_not_positive_definite_gives_nans_for_that_element_only(ctx):
    N, d = 130, 3
    X = synth.design(N, d, 960)[0]
    set_model(ctx, 1, X, 1)
    a, z, gram = R.operands(N, ctx.nreg, 61, nb=3)
    ths = np.array([R.thetas_at(1, d, s) for s in (0.6, 0.5, 0.7)])
    good = ctx.test_grad_sums(ths, a, z, gram, form=1, gram_dist=1)
    bad_gram = gram.copy()
    bad_gram[1, 2, 2] = -1.0                      # the second pivot of element 1 is negative
    bad = ctx.test_grad_sums(ths, a, z, bad_gram, form=1, gram_dist=1)
    assert np.all(np.isnan(bad["beta"][1])) and np.all(np.isnan(bad["alpha"][1]))
    diag = np.array([tr == tc for tr, tc in R.tile_list(N)])
    assert np.all(np.isnan(bad["part"][1][:, :d])) and np.all(np.isnan(bad["sums"][1][:d + 1]))
    # (the nugget slot of a tile below the diagonal has no summand here: it stays the exact zero it is)
    assert np.all(np.isnan(bad["part"][1][diag, d])) and np.all(bad["part"][1][~diag, d] == 0.0)
    for b in (0, 2):
        assert all(same_bits(bad[k_][b], good[k_][b]) for k_ in ("alpha", "beta", "part", "sums")), b
        assert np.all(np.isfinite(good["part"][b][:, :d + 1]))


# ------------------------------------------------------------------ the entry and the context
def test_entry_leaves_the_context_alone():
    """a value+gradient before and after the entry: the same bits; a prediction set-up made before it still predicts the
    same bits after it"""
    N, d = 200, 3
    X, y = synth.design(N, d, 970)
    c = abi.Context(0)
    c.set_model(1, 1, X, y)
    th = synth.default_thetas(1, d)
    a, z, gram = R.operands(N, c.nreg, 62, nb=2)
    ths = np.array([R.thetas_at(1, d, 0.5), R.thetas_at(1, d, 0.02, step=0.0)])
    for mode in (0, abi.MODE_EXACT_GRAD):
        c.set_mode(mode)
        before = c.loglik_grad(th)
        c.loglik_grad_batch_enqueue(np.array([th, th + 0.01]))
        c.test_grad_sums(ths, a, z, gram, form=1, gram_dist=-1)
        c.test_grad_sums(ths, a, z, form=0)
        pending = c.loglik_grad_batch_collect()
        after = c.loglik_grad(th)
        assert before["status"] == 0 and same_bits(before["grad"], after["grad"]) and before["value"] == after["value"]
        assert same_bits(pending["grad"][0], before["grad"]) and np.all(np.isfinite(pending["grad"]))
    c.set_mode(0)
    Xq = synth.queries(9, d, 971)
    c.predict_setup(th)
    m0, v0 = c.predict(Xq)
    inv0 = c.cinverse()
    c.test_grad_sums(ths, a, z, gram, form=1, gram_dist=0)
    m1, v1 = c.predict(Xq)
    assert same_bits(m0, m1) and same_bits(v0, v1) and same_bits(inv0, c.cinverse())
    c.close()


def test_refusals():
    N, d = 70, 3
    X, y = synth.design(N, d, 980)
    c = abi.Context(0)
    c.set_model(1, 0, X, y)
    a, z, gram = R.operands(N, 1, 63)
    th = R.thetas_at(1, d, 0.6)
    ok = c.test_grad_sums(th, a, z, form=0)

    def refused(**kw):
        args = dict(thetas=th, a=a, z=z, gram=gram, form=1, gram_dist=-1, clamp=-1)
        args.update(kw)
        with pytest.raises(abi.GpemuError) as e:
            c.test_grad_sums(**args)
        assert e.value.code == abi.ERR_ARG, kw

    refused(gram=None)                                                        # a NULL pointer (exact form needs gram)
    refused(form=2)
    refused(gram_dist=2)
    refused(form=0, clamp=0, thetas=R.thetas_at(1, d, 0.02, step=0.0))        # the rule selects the clamped kernel
    nb = 65                                                                   # beyond GPEMU_MAX_BATCH
    refused(form=0, gram=None, thetas=np.tile(th, (nb, 1)), a=np.tile(a, (nb, 1, 1)), z=np.tile(z, (nb, 1, 1)))
    args = abi.GradSumsArgs(nb=0, nthetas=th.size, form=0, gram_dist=-1, clamp=-1)
    assert c.L.gpemu_test_grad_sums(c.h, abi.C.byref(args)) == abi.ERR_ARG     # nb = 0, NULL pointers
    args.nb = 1
    assert c.L.gpemu_test_grad_sums(c.h, abi.C.byref(args)) == abi.ERR_ARG     # NULL pointers alone
    assert c.L.gpemu_test_grad_sums(c.h, None) == abi.ERR_ARG
    c.set_model(3, 0, X, y)
    thm = R.thetas_at(3, d, 0.6)
    for mode in (0, abi.MODE_EXACT_GRAD, abi.MODE_MATERN_LOG):                # a Matern model needs both flags
        c.set_mode(mode)
        refused(thetas=thm)
    c.set_mode(MATERN_MODES)
    refused(thetas=thm, form=0)                                               # no literal Matern gradient
    assert np.all(np.isfinite(c.test_grad_sums(thm, a, z, gram, form=1)["sums"][0][:2]))
    # nothing ran in a refused call: the literal run repeated afterwards has the bits it had
    c.set_mode(0)
    c.set_model(1, 0, X, y)
    again = c.test_grad_sums(th, a, z, form=0)
    assert same_bits(ok["part"], again["part"]) and same_bits(ok["sums"], again["sums"])
    c.close()


# ------------------------------------------------------------------ end to end through the public API
def _cond_1(Cm):
    cf = sl.cho_factor(Cm, lower=True)
    rcond, info = lapack.dpocon(cf[0], np.abs(Cm).sum(axis=0).max(), uplo="L")
    assert info == 0
    return 1.0 / rcond


def test_literal_gradient_with_the_clamped_kernel_against_the_oracle():
    """N = 200, d = 3, order 1, length scales 0.02: production's rule selects grad_part_kernel<true>; gpemu_grad and
    gpemu_loglik_grad against the oracle's gradFnMulti at the suite's 1e-7 form"""
    N, d, order = 200, 3, 1
    X, y = synth.design(N, d, 990)
    th = R.thetas_at(1, d, 0.02, step=0.0)
    assert not R.production_noclamp(X, th)
    assert _cond_1(gradref.powexp_matrix(X, th)[0]) <= COND_MAX
    c = abi.Context(0)
    c.set_model(1, order, X, y)
    ref, st = O.grad_fn_multi(1, order, X, y, th[1:])
    g, rc = c.grad(th)
    assert rc == 0 and st == 0
    assert np.allclose(g, ref, rtol=1e-7, atol=1e-7 * np.abs(ref).max()), (g, ref)
    one = c.loglik_grad(th)
    assert np.allclose(one["grad"], ref, rtol=1e-7, atol=1e-7 * np.abs(ref).max())
    c.close()


def test_literal_gradient_batch_with_one_short_scaled_element():
    """a batch of three whose middle element is short-scaled (the chunk runs the clamped kernel): every element against the
    oracle; the two ordinary elements keep the bits they have in a batch without it (the unclamped kernel)"""
    N, d, order = 200, 3, 1
    X, y = synth.design(N, d, 991)
    ths = np.array([R.thetas_at(1, d, 0.6), R.thetas_at(1, d, 0.02, step=0.0), R.thetas_at(1, d, 0.45)])
    assert not R.production_noclamp(X, ths) and R.production_noclamp(X, ths[[0, 2]])
    for th in ths:
        assert _cond_1(gradref.powexp_matrix(X, th)[0]) <= COND_MAX
    c = abi.Context(0)
    c.set_model(1, order, X, y)
    got = c.loglik_grad_batch(ths)
    assert np.all(got["status"] == 0)
    for b in range(3):
        ref, st = O.grad_fn_multi(1, order, X, y, ths[b][1:])
        assert st == 0 and np.allclose(got["grad"][b], ref, rtol=1e-7, atol=1e-7 * np.abs(ref).max()), (b, got["grad"][b], ref)
    two = c.loglik_grad_batch(ths[[0, 2]])
    assert same_bits(two["grad"][0], got["grad"][0]) and same_bits(two["grad"][1], got["grad"][2])
    c.close()


@pytest.mark.parametrize("kind", [2, 3])
@pytest.mark.parametrize("N", [200, 520])
def test_matern_exact_gradient_across_tiles(monkeypatch, kind, N):
    """Matern exact gradients over diagonal, interior and edge tiles against gradref.value_and_gradients_matern (LAPACK
    inverse, the kernel's derivative in log rho): gpemu_loglik_grad, an element of a batch, both GPEMU_GRAD_GRAM settings,
    at 1e-8 of the largest component AND each component within 1e-8 of its own 1/2 sum |W dC|"""
    d, order = 3, 1
    X, y = synth.design(N, d, 992 + N)
    ths = np.array([[0.0, -3.0, np.log(0.6)], [0.0, -2.5, np.log(0.15)]])
    refs = [gradref.value_and_gradients_matern(kind, X, y, order, th) for th in ths]
    for r in refs:
        assert r["cond_1"] <= COND_MAX, r["cond_1"]
    for sw in ("1", "0"):
        c = _ctx_with_env(monkeypatch, {"GPEMU_GRAD_GRAM": sw})
        c.set_mode(MATERN_MODES)
        c.set_model(kind, order, X, y)
        bat = c.loglik_grad_batch(ths)
        one = c.loglik_grad(ths[1])
        assert np.all(bat["status"] == 0) and one["status"] == 0
        for b, g in ((0, bat["grad"][0]), (1, bat["grad"][1]), (1, one["grad"])):
            ref = refs[b]
            err = np.abs(g - ref["exact"])
            print(f"Matern kind {kind} N={N} GRAD_GRAM={sw} element {b}: error / (1e-8 max) {err.max() / (RTOL * np.abs(ref['exact']).max()):.3e}, "
                  f"error / (1e-8 own scale) {np.max(err / (RTOL * ref['scale'])):.3e}")
            assert err.max() < RTOL * np.abs(ref["exact"]).max(), (b, g, ref["exact"])
            assert np.all(err <= RTOL * ref["scale"]), (b, g, ref["exact"], ref["scale"])
        assert bat["value"][0] == pytest.approx(refs[0]["value"], rel=RTOL) and one["value"] == pytest.approx(refs[1]["value"], rel=RTOL)
        c.close()
