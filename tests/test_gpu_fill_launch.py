"""The covariance fill kernels (cov_stage_gram_kernel, cov_stage_batch_kernel in both of its per-matrix forms,
cov_kvec_gram_kernel, cov_fill_kernel) ONE launch at a time through gpemu_test_fill_launch -- production's launchers on a
region of the caller's -- against tests/covref.py: EVERY element of every region against the project's element bar
(1e-13 + 1e-15 |exp argument|, the same for the Gram form and for differences, never fitted to the device), and every other
cell of the region bit for bit: identity / zero padding, right-hand-side rows, and the caller's prefill in the tiles above
the diagonal, behind the last right-hand-side row and in the guard rows.  The inputs and the conditions they meet (room
under the bar in an fp64 model, no k-vector element at the clamp, the whole exp table reached) are checked on the CPU in
tests/test_covref.py.  Each test prints the worst error / bar it saw."""
import numpy as np
import pytest

import covref as R
from madaiemulator_amd import abi

pytestmark = pytest.mark.gpu

STAGE, KVEC, FULL = abi.FILL_STAGE, abi.FILL_KVEC, abi.FILL_FULL
KINDS = (1, 2, 3)
RP = 64


def set_model(c, kind, X, matern_log=False):
    c.set_mode(abi.MODE_MATERN_LOG if matern_log else 0)
    c.set_model(kind, 0, X, np.zeros(X.shape[0]))


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.set_mode(0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def prefill(shape, pattern):
    """two patterns: NaN everywhere (whatever the launch reads of it shows), and distinct finite negative numbers"""
    if pattern == 0:
        return np.full(shape, np.nan)
    return -7.25 - np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape) * 2.0 ** -10


def rhs_rows(nb, Rp, Np, seed=1):
    return 3.0 + seed + np.arange(nb * Rp * Np, dtype=np.float64) * 2.0 ** -12


def report(what, worst, nbad=0):
    print(f"{what}: worst error / bar {worst:.3f}, cells off their bits {nbad}")
    assert nbad == 0, (what, nbad)
    assert worst <= 1.0, (what, worst)


def stage(c, kind, X, ths, form, pattern=0, Rp=RP, guard=3, shared=False, matern_log=False, pre=None, what=""):
    """one staging launch and its whole region against the image -> (region, image, form per matrix, norm2 per matrix)"""
    ths = np.atleast_2d(ths)
    nb, Np = ths.shape[0], R.round_up(X.shape[0])
    rr = rhs_rows(1 if shared else nb, Rp, Np)
    rstride = 0 if shared else Rp * Np
    fill = prefill((nb, Np + Rp + guard, Np), pattern)
    got, fo, n2 = c.test_fill_launch(STAGE, ths, fill, form=form, rrows=rr, rstride=rstride, Rp=Rp, guard=guard)
    img = R.staged_image(kind, X, ths, fill, rr, rstride=rstride, Rp=Rp, guard=guard, matern_log=matern_log, pre=pre)
    worst, nbad = img.check(got)
    report(f"{what} kind {kind} N={X.shape[0]} d={X.shape[1]} form {form} nb={nb}", worst, nbad)
    for b in range(nb):
        assert n2[b] == pytest.approx(R.norm2(kind, X, ths[b]), rel=1e-13, abs=1e-300)
    return got, img, fo, n2


# ------------------------------------------------------------------ the staging launch
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,d", R.SHAPES)
def test_stage_whole_region_every_form(ctx, kind, N, d):
    """five thetas (all admitted) in every form: the whole region of a batch of five with per-matrix right-hand sides under
    two prefill patterns, and of every matrix alone with shared right-hand sides (Rp = 70: a second, partly written block of
    rows) and of the batch with ONE shared block -- in one form, matrix b of the batch IS the matrix staged alone, bit for bit"""
    X = R.shape_design(N, d)
    ths = R.batch_thetas(kind, X)
    set_model(ctx, kind, X)
    pre = [R.elements(kind, X, X, th) for th in ths]
    Np = R.round_up(N)
    for form in (-1, 0, 1, 2):
        a, img, fo, n2 = stage(ctx, kind, X, ths, form, pattern=0, pre=pre, what="batch")
        assert list(fo) == [0 if form == 0 else 1] * 5 and np.all(n2 <= 16.0)
        # the second prefill with ONE shared block of right-hand sides (rstride = 0, as every likelihood batch stages them):
        # the image check pins that block under all five matrices; the matrices themselves keep their bits
        b_, _, _, _ = stage(ctx, kind, X, ths, form, pattern=1, shared=True, pre=pre, what="batch, shared right-hand sides, second prefill")
        assert np.array_equal(bits(a[:, :Np])[img.written[:, :Np]], bits(b_[:, :Np])[img.written[:, :Np]])
        assert all(np.array_equal(bits(b_[b, Np:Np + RP]), bits(b_[0, Np:Np + RP])) for b in range(5))
        assert not np.array_equal(bits(a[1, Np:Np + RP]), bits(a[0, Np:Np + RP]))           # (per matrix: they differ)
        for b in range(5):
            one, img1, fo1, _ = stage(ctx, kind, X, ths[b], form, pattern=b % 2, Rp=70, guard=60, shared=True, pre=[pre[b]],
                                      what=f"matrix {b} alone")
            assert fo1[0] == fo[b]
            w = img.written[b, :Np]
            assert np.array_equal(bits(one[0, :Np])[w], bits(a[b, :Np])[w]), (form, b)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,d", R.BOUNDARY_SHAPES)
def test_admission_boundary(ctx, kind, N, d):
    """corner-clustered design, every |x'|^2 close to norm2: at norm2 = 16 (1 - 1e-3) production takes the Gram form, at
    16 (1 + 1e-3) differences (and refuses the Gram form), both under the same flat bar"""
    X, th = R.boundary_case(kind, N, d, R.JUST_UNDER)
    set_model(ctx, kind, X)
    pre = [R.elements(kind, X, X, th)]
    _, _, fo, n2 = stage(ctx, kind, X, th, -1, pre=pre, what="just under 16")
    assert fo[0] == 1 and 15.9 < n2[0] < 16.0
    stage(ctx, kind, X, th, 1, pre=pre, what="just under 16")
    _, _, fo, _ = stage(ctx, kind, X, th, 0, pre=pre, what="just under 16")
    assert fo[0] == 0
    X2, th2 = R.boundary_case(kind, N, d, R.JUST_OVER)
    assert np.array_equal(X, X2)
    _, _, fo, n2 = stage(ctx, kind, X, th2, -1, what="just over 16")
    assert fo[0] == 0 and 16.0 < n2[0] < 16.1
    with pytest.raises(abi.GpemuError) as e:
        stage(ctx, kind, X, th2, 1)
    assert e.value.code == abi.ERR_ARG
    if kind != 1:
        set_model(ctx, kind, X, matern_log=True)
        thl = th.copy()
        thl[:2] = 0.4, -2.5
        _, _, fo, _ = stage(ctx, kind, X, thl, -1, matern_log=True, what="just under 16, log-scale amplitude and nugget")
        assert fo[0] == 1


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,d", R.BOUNDARY_SHAPES[:2])
def test_mixed_batch(ctx, kind, N, d):
    """thetas alternately admitted to the Gram form and refused: the batch kernel with the per-matrix switch, by
    production's rule and forced; every matrix is the one staged alone by the same kernel"""
    X, _ = R.boundary_case(kind, N, d, R.JUST_UNDER)
    ths = R.mixed_thetas(kind, X)
    set_model(ctx, kind, X)
    pre = [R.elements(kind, X, X, th) for th in ths]
    a, img, fo, n2 = stage(ctx, kind, X, ths, -1, pre=pre, what="mixed batch")
    assert list(fo) == [1, 0, 1, 0, 1] and list(n2 <= 16.0) == [True, False, True, False, True]
    Np = R.round_up(N)
    f2, _, fo2, _ = stage(ctx, kind, X, ths, 2, pattern=1, shared=True, pre=pre, what="mixed batch, shared right-hand sides")
    assert list(fo2) == [1, 0, 1, 0, 1] and np.array_equal(bits(a[:, :Np])[img.written[:, :Np]], bits(f2[:, :Np])[img.written[:, :Np]])
    assert all(np.array_equal(bits(f2[b, Np:Np + RP]), bits(f2[0, Np:Np + RP])) for b in range(5))
    _, _, fo0, _ = stage(ctx, kind, X, ths, 0, pre=pre, what="mixed batch")
    assert not fo0.any()
    with pytest.raises(abi.GpemuError):
        stage(ctx, kind, X, ths, 1)
    for b in range(5):
        one, _, fo1, _ = stage(ctx, kind, X, ths[b], 2, pre=[pre[b]], shared=True, what=f"matrix {b} alone")
        w = img.written[b, :Np]
        assert fo1[0] == fo[b] and np.array_equal(bits(one[0, :Np])[w], bits(a[b, :Np])[w]), b


@pytest.mark.parametrize("kind,name", [(k, n) for k in KINDS for n in R.PAIR_OFFSETS[k]])
def test_same_point_and_near_pairs_in_the_gram_form(ctx, kind, name):
    """pairs in a diagonal tile (inside one 16-row group, across waves), a full off-diagonal tile and the edge tiles -- all
    three store branches of the Gram tile --: the nugget exactly where the reference's rule puts it, the bar elsewhere"""
    X = R.pair_design(kind, name)
    th = R.pair_theta(kind, X)
    same = R.same_point(kind, X)
    for log in ((False,) if kind == 1 else (False, True)):
        set_model(ctx, kind, X, matern_log=log)
        pre = [R.elements(kind, X, X, th, matern_log=log)]
        amp, nug = (float(v) for v in R.amp_nug(kind, th, log))
        for form in (1, -1, 2, 0):
            got, _, fo, _ = stage(ctx, kind, X, th, form, matern_log=log, pre=pre, what=f"pairs {name}")
            assert fo[0] == (0 if form == 0 else 1)
            for i, j in R.PAIR_SPOTS.values():
                assert (got[0, j, i] > amp + 0.5 * nug) == bool(same[j, i]), (name, form, i, j)     # (a pair's distance is ~0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", [4, 16])
def test_cancellation_ladder_at_the_far_corner(ctx, kind, d):
    """partners 1e-9 .. 1e-2 away from the corner of the box, where |x'|^2 is largest, at norm2 just under 16"""
    X = R.ladder_design(d)
    th = R.ladder_theta(kind, X)
    set_model(ctx, kind, X)
    pre = [R.elements(kind, X, X, th)]
    for form in (1, -1, 2):
        _, _, fo, n2 = stage(ctx, kind, X, th, form, pre=pre, what="ladder")
        assert fo[0] == 1 and 15.9 < n2[0] < 16.0


def test_exp_table_every_entry(ctx):
    """d = 1, pow-exp: pair exponents over [0, 64) reach all 1024 entries of the Gram form's table (test_covref.py)"""
    X, th = R.table_design()
    set_model(ctx, 1, X)
    _, _, fo, _ = stage(ctx, 1, X, th, 1, what="exp table")
    assert fo[0] == 1


# ------------------------------------------------------------------ k-vectors
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,d", R.KVEC_SHAPES)
@pytest.mark.parametrize("M", R.KVEC_M)
def test_kvectors_both_forms(ctx, kind, N, d, M):
    """query rows inside the box, on design points, just inside and just outside the Gram form's far test, and one far
    row in a wave of ordinary rows, at norm2 just under 16: elements under the bar, the zero pattern of the clamp equal to
    the reference's, rows >= M and columns >= N zero, the guard rows untouched"""
    X, th, Xq = R.kvec_case(kind, N, d, M)
    set_model(ctx, kind, X)
    Np, Mp, guard = R.round_up(N), R.round_up(M), 2
    v = R.elements(kind, Xq, X, th, clamp=True)[0]
    for form, pattern in ((1, 0), (0, 1), (-1, 1)):
        fill = prefill((Mp + guard, Np), pattern)
        got, fo, n2 = ctx.test_fill_launch(KVEC, th, fill, form=form, Xq=Xq, guard=guard)
        img = R.kvec_image(kind, X, Xq, th, fill, guard=guard)
        worst, nbad = img.check(got)
        report(f"k-vectors kind {kind} N={N} d={d} M={M} form {form}", worst, nbad)
        assert fo[0] == (0 if form == 0 else 1) and 15.9 < n2[0] < 16.0
        assert np.array_equal(got[:M, :N] == 0.0, v == 0)
        if M > 1:
            assert np.all(got[50, :N] == 0.0) and got[3, 5] > got[3, 6] and got[M - 1, 0] > got[M - 1, 2]


# ------------------------------------------------------------------ the full matrix
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,d", R.SHAPES)
def test_full_matrix_is_what_cov_matrix_returns(ctx, kind, N, d):
    X = R.shape_design(N, d)
    th = R.batch_thetas(kind, X)[2]
    set_model(ctx, kind, X)
    Np, guard = R.round_up(N), 1
    fill = prefill((Np + guard, Np), 0)
    got, fo, _ = ctx.test_fill_launch(FULL, th, fill, form=0, guard=guard)
    worst, nbad = R.full_image(kind, X, th, fill, guard=guard).check(got)
    report(f"full matrix kind {kind} N={N} d={d}", worst, nbad)
    assert fo[0] == 0 and np.array_equal(bits(got[:Np]), bits(got[:Np].T))
    assert np.array_equal(bits(got[:N, :N]), bits(ctx.cov_matrix(th)))


# ------------------------------------------------------------------ refusals
def test_refusals_launch_nothing(ctx):
    import ctypes as C
    N, d = 65, 3
    X = R.shape_design(N, d)
    set_model(ctx, 1, X)
    Np = R.round_up(N)
    ok = R.thetas_for_norm2(1, X, 4.0)
    refused = R.thetas_for_norm2(1, X, 20.0)
    rr = rhs_rows(1, RP, Np)
    region = lambda nb=1, guard=0: prefill((nb, Np + RP + guard, Np), 1)

    def raises(**kw):
        fill = kw.pop("out")
        with pytest.raises(abi.GpemuError) as e:
            ctx.test_fill_launch(kw.pop("op", STAGE), kw.pop("thetas", ok), fill, **kw)
        assert e.value.code == abi.ERR_ARG
        assert np.array_equal(bits(e.value.region), bits(fill))                        # nothing was launched, nothing copied back

    got, fo, _ = ctx.test_fill_launch(STAGE, ok, region(), form=1, rrows=rr)           # the accepted call
    assert fo[0] == 1 and not np.array_equal(got, region())
    raises(out=region(), form=1, thetas=refused, rrows=rr)                              # form 1, theta not admitted
    raises(out=region(2), form=1, thetas=np.array([ok, refused]), rrows=rr)
    raises(out=region(), form=3, rrows=rr)                                              # form outside its values
    raises(out=region(), form=-2, rrows=rr)
    raises(out=region(), op=3, rrows=rr)                                                # op
    raises(out=region(), op=FULL, form=1)
    raises(out=region(), op=KVEC, form=2, Xq=X[:2])
    raises(out=region(), rrows=None)                                                    # NULL right-hand sides
    raises(out=prefill((64, Np), 1), op=KVEC, Xq=None)                                  # NULL / no query rows
    raises(out=region().ravel()[:-1], rrows=rr)                                         # one element short
    raises(out=region(guard=2).ravel()[:-1], rrows=rr, guard=3)
    raises(out=prefill((64, Np), 1), op=KVEC, Xq=X[:65])                                # Mp = 128 rows needed
    raises(out=prefill((Np - 1, Np), 1), op=FULL, form=0)
    raises(out=region(), rrows=rr, guard=-1)
    raises(out=region(), rrows=rr, Rp=-1)
    raises(out=region(), rrows=rr, rstride=-1)
    raises(out=region(2), thetas=np.array([ok, ok]), rrows=np.zeros(4 * RP * Np + 1 + RP * Np), rstride=4 * RP * Np + 1)
    raises(out=region(), op=FULL, form=0, thetas=np.array([ok, ok]))                    # nb = 2 where one matrix is filled
    raises(out=region(), thetas=ok[:d + 1], rrows=rr)                                   # too few thetas
    big = np.tile(ok, (65, 1))                                                          # nb = GPEMU_MAX_BATCH + 1
    raises(out=prefill((65, Np + RP, Np), 1), thetas=big, rrows=rr)
    # NULL pointers and nb / M < 1 the binding cannot express: the C entry itself
    L, h = ctx.L, ctx.h
    out = region()
    th = np.ascontiguousarray(ok)
    fo, n2 = np.zeros(1, dtype=np.int32), np.zeros(1)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    p = lambda a: a.ctypes.data_as(dp)
    base = dict(thetas=p(th), rrows=p(rr), xq=p(X), out=p(out), norm2_out=p(n2), form_out=fo.ctypes.data_as(ip),
                out_len=out.size, rstride=0, op=STAGE, form=-1, nb=1, nthetas=th.size, M=0, Rp=0, guard=0)
    assert L.gpemu_test_fill_launch(h, None) == abi.ERR_ARG
    assert L.gpemu_test_fill_launch(None, C.byref(abi.FillLaunchArgs(**base))) == abi.ERR_ARG
    for k_ in ("thetas", "out", "norm2_out", "form_out", "rrows"):
        assert L.gpemu_test_fill_launch(h, C.byref(abi.FillLaunchArgs(**dict(base, **{k_: None})))) == abi.ERR_ARG, k_
    for change in (dict(nb=0), dict(nb=-1), dict(op=KVEC, M=0), dict(op=KVEC, M=-3), dict(op=KVEC, M=1, xq=None)):
        assert L.gpemu_test_fill_launch(h, C.byref(abi.FillLaunchArgs(**dict(base, **change)))) == abi.ERR_ARG, change
    assert np.array_equal(bits(out), bits(region()))                                    # nothing was launched
    # a design without a centred copy (a coordinate beyond 1e300) has no Gram form
    Xh = X.copy()
    Xh[0, 0] = 1e301
    set_model(ctx, 1, Xh)
    raises(out=region(), form=1, rrows=rr)
    _, fo, n2 = ctx.test_fill_launch(STAGE, ok, region(), form=-1, rrows=rr)
    assert fo[0] == 0 and np.isnan(n2[0])
