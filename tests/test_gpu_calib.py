"""Implausibility and calibration likelihood against observations on the device (gpemu_calib_*, include/gpemu.h,
DESIGN.md 4.18), through abi.Context with the test's own mean and variance arrays: only the new kernels are under test.

Reference: the direct nt x nt form in float64 (calibref.direct64), never the r x r identity the kernels evaluate; the v = 1e30
family, which float64 cannot factor in the direct form, against the 50-digit repeat alone.  Error measure |got - ref| /
max(1, |ref|) per statistic; bars calibref.BARS = 8 x the reference's own largest error against 50 digits, measured on the
CPU (tests/test_calibref.py keeps them honest).  worst is compared exactly where the reference's top two implausibilities
differ by more than the bar and skipped elsewhere, and at most 5 % of a case's points may be skipped that way."""
import ctypes as C
import functools

import numpy as np
import pytest

import calibref as R
from madaiemulator_amd import abi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.calib_release()


@functools.lru_cache(maxsize=None)
def reference(key):
    """the case and its float64 reference, computed once and shared (the arrays are read-only)"""
    c = R.make_special(key[8:]) if key.startswith("special_") else R.make_case(*next(a for a in R.CASES if a[0] == key))
    stat, worst = R.direct64(c)
    for a in (stat, worst, c["mean"], c["var"]):
        a.setflags(write=False)
    return c, stat, worst


def setup(ctx, c):
    rc, info = ctx.calib_setup(c["ybar"], c["A"], c["z"], S=c["S"], sd=c["sd"], rel=c["rel"])
    assert rc == abi.OK and info == 0


def check(what, stat, worst, sref, wref, skip_cap=0.05):
    e = R.err(stat, sref).max(axis=1)
    print(what, " ".join(f"{n} {x:.2e}/{b:.1e}" for n, x, b in zip(R.STATS, e, R.BARS)))
    assert np.all(e <= R.BARS), (what, e, R.BARS)
    comp = R.worst_comparable(sref)
    skipped = 1.0 - comp.mean()
    print(what, f"worst: {comp.sum()} of {comp.size} compared, {skipped:.3f} skipped")
    assert skipped <= skip_cap, (what, skipped)
    assert np.array_equal(worst[comp], wref[comp]), what


# ------------------------------------------------------------------ 1. every shape against the direct form
@pytest.mark.parametrize("key", [a[0] for a in R.CASES])
def test_shapes_against_direct_form(ctx, key):
    c, sref, wref = reference(key)
    setup(ctx, c)
    stat, worst = ctx.calib_eval(c["mean"], c["var"], M=c["M"])
    assert stat.shape == (5, c["M"]) and np.all(np.isfinite(stat))
    check(key, stat, worst, sref, wref)
    if c["nt"] < 3:                                      # the missing largest-but-k are 0, exactly
        assert np.all(stat[2 + c["nt"]:] == 0.0)
    stat2, worst2 = ctx.calib_eval(c["mean"], c["var"], M=c["M"])
    assert stat.tobytes() == stat2.tobytes() and worst.tobytes() == worst2.tobytes()      # a call repeated: the same bits


def test_dev_entry_returns_the_host_entry_bits(ctx):
    c, _, _ = reference("r16_nt65_full_rel")
    setup(ctx, c)
    M, nr, ld = c["M"], c["nr"], c["mean"].shape[1]
    stat, worst = ctx.calib_eval(c["mean"], c["var"], M=M)
    dm, dv = ctx.dev_alloc(8 * nr * ld), ctx.dev_alloc(8 * nr * ld)
    ds, dw = ctx.dev_alloc(8 * 5 * M), ctx.dev_alloc(4 * M)
    try:
        ctx.upload(dm, c["mean"]); ctx.upload(dv, c["var"])
        ctx.calib_eval_dev(M, dm, dv, ld, ds, dw)
        s2, w2 = ctx.download(ds, (5, M)), ctx.download(dw, (M,), dtype=np.int32)
    finally:
        for p in (dm, dv, ds, dw):
            ctx.dev_free(p)
    assert stat.tobytes() == s2.tobytes() and worst.tobytes() == w2.tobytes()


# ------------------------------------------------------------------ 2. special inputs
@pytest.mark.parametrize("kind", ["v_zero", "v_negative"])
def test_zero_and_slightly_negative_variances(ctx, kind):
    """D singular (a point on the design), and kappa - |L^-1 k|^2 a few ulp below 0: counted as 0"""
    c, sref, wref = reference("special_" + kind)
    setup(ctx, c)
    stat, worst = ctx.calib_eval(c["mean"], c["var"], M=c["M"])
    check(kind, stat, worst, sref, wref)
    if kind == "v_negative":
        c0, _, _ = reference("special_v_zero")
        s0, w0 = ctx.calib_eval(c0["mean"], c0["var"], M=c0["M"])
        assert stat.tobytes() == s0.tobytes() and worst.tobytes() == w0.tobytes()


def test_huge_variances_against_50_digits(ctx):
    """v = 1e30 on every component: chi2 -> c_perp; the direct form cannot be factored in float64, so 50 digits alone"""
    c, _, _ = reference("special_v_huge")
    setup(ctx, c)
    stat, worst = ctx.calib_eval(c["mean"], c["var"], M=c["M"])
    pts = R.mp_points(c)
    ref, wref = R.direct_mp(c, pts)
    e = R.err(stat[:, pts], ref).max(axis=1)
    print("v_huge", e)
    assert np.all(e <= R.BARS), e
    pj = abi.calib_project(c["ybar"], c["A"], c["z"], sd=c["sd"])
    assert np.all(R.err(stat[0], pj["c_perp"]) <= R.BARS[0])
    assert np.all(np.isfinite(stat)) and np.all((worst >= 0) & (worst < c["nt"]))


def test_nan_in_one_point_only(ctx):
    c, sref, wref = reference("special_one_nan")
    setup(ctx, c)
    stat, worst = ctx.calib_eval(c["mean"], c["var"], M=c["M"])
    assert np.all(np.isnan(stat[:, 17])) and worst[17] == -1
    others = np.arange(c["M"]) != 17
    assert np.all(np.isfinite(stat[:, others]))
    check("one_nan", stat, worst, sref, wref)
    # a NaN variance likewise (the clamp of negative variances must not swallow it)
    var = c["var"].copy()
    var[0, 3] = np.nan
    stat, worst = ctx.calib_eval(c["mean"], var, M=c["M"])
    assert np.all(np.isnan(stat[:, 3])) and np.all(np.isnan(stat[:, 17])) and np.all(np.isfinite(stat[:, 4:17]))


def test_exact_ties_take_the_smallest_index(ctx):
    c, sref, wref = reference("special_ties")
    setup(ctx, c)
    stat, worst = ctx.calib_eval(c["mean"], c["var"], M=c["M"])
    assert np.all(stat[2] == stat[3]) and np.all(stat[2] > stat[4])
    assert np.all(worst == 2)
    assert np.all(R.err(stat, sref).max(axis=1) <= R.BARS)


def test_chi2_is_not_the_diagonal_rule(ctx):
    """S and A D A^T are not diagonal: the joint chi2 must differ from sum_t I_t^2, which the reference's rule would give"""
    c, sref, _ = reference("r2_nt2_full")
    setup(ctx, c)
    stat, _ = ctx.calib_eval(c["mean"], c["var"], M=c["M"])
    diag_rule = stat[2] ** 2 + stat[3] ** 2              # nt = 2: the two implausibilities are all of them
    assert np.median(np.abs(stat[0] - diag_rule) / stat[0]) > 1e-2
    assert np.all(R.err(stat[0], sref[0]) <= R.BARS[0])


# ------------------------------------------------------------------ 3. selection
def numpy_select(stat, cut_chi2, level, cut_I):
    with np.errstate(invalid="ignore"):
        return np.flatnonzero((stat[0] <= cut_chi2) & (stat[1 + level] <= cut_I)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def selection_stat(M):
    rng = np.random.default_rng(77 + M)
    stat = np.abs(rng.standard_normal((5, M))) * 3.0
    stat[2:] = -np.sort(-stat[2:], axis=0)
    if M > 10:
        stat[0, 3] = np.nan
        stat[2, 7] = np.nan
        stat[3, 9] = np.nan
    stat.setflags(write=False)
    return stat


# 64 and 65 workgroups of 1024 points (the scan's sum across its waves), 256 and 257 (its carry into a second trip), 293
LARGE_MS = [65536, 65537, 262144, 262145, 300001]
KEEP_PATTERNS = ("whole-workgroups", "last-point", "workgroups-64-255-256", "everything", "nothing", "nan-in-workgroup-256")


def keep_pattern(name, M):
    """-> stat[5, M] whose points are kept under (cut_chi2 4, level 1, cut_I 2) by the named pattern: uneven prefix sums, where
    selection_stat keeps about the same share of every workgroup"""
    rng = np.random.default_rng(177 + M)
    wg = np.arange(M) // 1024
    if name == "whole-workgroups":                        # runs of whole workgroups kept next to runs with none, of uneven lengths
        keep = rng.random(wg.max() + 1)[wg] < 0.5
    elif name == "last-point":
        keep = np.arange(M) == M - 1
    elif name == "workgroups-64-255-256":
        keep = np.isin(wg, (64, 255, 256)) & (rng.random(M) < 0.7)
    elif name == "nothing":
        keep = np.zeros(M, dtype=bool)
    else:
        keep = np.ones(M, dtype=bool)
    stat = np.empty((5, M))
    stat[0] = np.where(keep, 1.0 + rng.random(M), 5.0 + rng.random(M))
    stat[1] = rng.standard_normal(M)
    stat[2:] = -np.sort(-rng.random((3, M)), axis=0)
    if name == "nan-in-workgroup-256":                    # a NaN in either row the cuts read: never kept
        at = np.flatnonzero(wg == 256)
        stat[0, at[::3]] = np.nan
        stat[2, at[1::7]] = np.nan
    return stat


@pytest.mark.parametrize("M", [1, 63, 64, 65, 257, 1000, 1024, 1025, 2500] + LARGE_MS)
def test_select_matches_numpy(ctx, M):
    stat = selection_stat(M)
    if M in LARGE_MS:
        for name in KEEP_PATTERNS:
            st = keep_pattern(name, M)
            got = ctx.calib_select(st, 4.0, 1, 2.0)
            want = numpy_select(st, 4.0, 1, 2.0)
            print(f"M {M} {name}: {want.size} kept")
            assert np.array_equal(got, want), (M, name)
            if name == "everything":
                assert np.array_equal(got, np.arange(M, dtype=np.int32))
            if name == "nothing":
                assert got.size == 0
            if name == "last-point":
                assert got.tolist() == [M - 1]
            if name == "nan-in-workgroup-256" and M > 262144:
                assert 0 < M - got.size <= 1024 and not np.isnan(st[0, got]).any() and not np.isnan(st[2, got]).any()
    for cut_chi2, level, cut_I in [(np.inf, 1, 3.0), (4.0, 1, np.inf), (5.0, 2, 2.0), (np.inf, 3, 1.0), (np.inf, 1, np.inf),
                                   (-1.0, 1, np.inf), (np.inf, 2, -1.0)]:
        got = ctx.calib_select(stat, cut_chi2, level, cut_I)
        want = numpy_select(stat, cut_chi2, level, cut_I)
        assert np.array_equal(got, want), (M, cut_chi2, level, cut_I)
        assert np.all(np.diff(got) > 0)
    if M > 10:                                            # a NaN is never kept, whichever row the level reads
        allk = ctx.calib_select(stat, np.inf, 1, np.inf)
        assert 3 not in allk and 7 not in allk and 9 in allk
        assert 9 not in ctx.calib_select(stat, np.inf, 2, np.inf)


def test_select_edges(ctx):
    M = 2500                                              # three workgroups of 1024 points
    stat = selection_stat(M).copy()
    # survivors only in the last workgroup
    stat[2, :2048] = 100.0
    got = ctx.calib_select(stat, np.inf, 1, 50.0)
    assert np.array_equal(got, numpy_select(stat, np.inf, 1, 50.0)) and got.size > 0 and got.min() >= 2048
    # the cut exactly equal to a value: kept (<=)
    v = float(stat[2, 2100])
    got = ctx.calib_select(stat, np.inf, 1, v)
    assert 2100 in got and np.array_equal(got, numpy_select(stat, np.inf, 1, v))
    assert 2100 not in ctx.calib_select(stat, np.inf, 1, np.nextafter(v, -np.inf))
    v = float(stat[0, 11])
    assert 11 in ctx.calib_select(stat, v, 1, np.inf) and 11 not in ctx.calib_select(stat, np.nextafter(v, -np.inf), 1, np.inf)
    # no survivor, all survivors
    assert ctx.calib_select(stat, -1.0, 1, np.inf).size == 0
    clean = np.abs(selection_stat(M)) + 0.0
    clean = np.nan_to_num(clean, nan=1.0)
    assert np.array_equal(ctx.calib_select(clean, np.inf, 1, np.inf), np.arange(M, dtype=np.int32))
    # a call repeated: the same bits
    a, b = ctx.calib_select(stat, 4.0, 2, 2.5), ctx.calib_select(stat, 4.0, 2, 2.5)
    assert a.tobytes() == b.tobytes()


def test_select_on_downloaded_stat_and_dev_entry(ctx):
    c, _, _ = reference("r8_nt64_full_rel")
    setup(ctx, c)
    stat, worst = ctx.calib_eval(c["mean"], c["var"], M=c["M"])
    cut2, cutI = float(np.median(stat[0])), float(np.median(stat[2]) * 1.2)
    want = numpy_select(stat, cut2, 1, cutI)
    got = ctx.calib_select(stat, cut2, 1, cutI)
    assert 0 < want.size < c["M"] and np.array_equal(got, want)
    M = c["M"]
    ds, di = ctx.dev_alloc(8 * 5 * M), ctx.dev_alloc(4 * M)
    try:
        ctx.upload(ds, stat)
        n = ctx.calib_select_dev(M, ds, cut2, 1, cutI, di)
        idx = ctx.download(di, (M,), dtype=np.int32)
        # the survivors' rows, point-major, and their worst outputs: what a caller downloads instead of all of stat
        dw, dg, dgw = ctx.dev_alloc(4 * M), ctx.dev_alloc(8 * 5 * M), ctx.dev_alloc(4 * M)
        try:
            ctx.upload(dw, worst)
            ctx.upload(dg, np.full((M, 5), -7.0)); ctx.upload(dgw, np.full(M, -7, dtype=np.int32))
            ctx.calib_gather_dev(M, ds, dw, n, di, dg, dgw)
            g, gw = ctx.download(dg, (M, 5)), ctx.download(dgw, (M,), dtype=np.int32)
        finally:
            for p in (dw, dg, dgw):
                ctx.dev_free(p)
    finally:
        ctx.dev_free(ds); ctx.dev_free(di)
    assert n == want.size and np.array_equal(idx[:n], want)
    assert g[:n].tobytes() == np.ascontiguousarray(stat[:, want].T).tobytes() and np.array_equal(gw[:n], worst[want])
    assert np.all(g[n:] == -7.0) and np.all(gw[n:] == -7)          # nothing beyond the count is written


@pytest.mark.parametrize("M,name", [(2500, "whole-workgroups"), (262145, "workgroups-64-255-256"), (300001, "whole-workgroups")])
def test_select_dev_then_gather_dev_beyond_256(ctx, M, name):
    """gpemu_calib_select_dev then gpemu_calib_gather_dev with more than 256 survivors (the gather's workgroups >= 1), with and
    without `worst`: every gathered row is the bits of stat[:, idx], nothing beyond the count is written"""
    stat = keep_pattern(name, M)
    worst = np.random.default_rng(M).integers(0, 64, M).astype(np.int32)
    want = numpy_select(stat, 4.0, 1, 2.0)
    assert 256 < want.size < M
    ds, di, dw, dg, dgw = (ctx.dev_alloc(s) for s in (8 * 5 * M, 4 * M, 4 * M, 8 * 5 * M, 4 * M))
    try:
        ctx.upload(ds, stat)
        ctx.upload(dw, worst)
        ctx.upload(di, np.full(M, -1, dtype=np.int32))
        n = ctx.calib_select_dev(M, ds, 4.0, 1, 2.0, di)
        idx = ctx.download(di, (M,), dtype=np.int32)
        assert n == want.size and np.array_equal(idx[:n], want) and np.all(idx[n:] == -1)
        rows = np.ascontiguousarray(stat[:, want].T)
        for with_worst in (True, False):
            ctx.upload(dg, np.full((M, 5), -7.0))
            ctx.upload(dgw, np.full(M, -7, dtype=np.int32))
            ctx.calib_gather_dev(M, ds, dw if with_worst else None, n, di, dg, dgw)
            ctx.sync()
            g, gw = ctx.download(dg, (M, 5)), ctx.download(dgw, (M,), dtype=np.int32)
            assert g[:n].tobytes() == rows.tobytes(), (M, with_worst)
            assert np.all(g[n:] == -7.0)
            if with_worst:
                assert np.array_equal(gw[:n], worst[want]) and np.all(gw[n:] == -7)
            else:
                assert np.all(gw == -7)                   # without `worst` nothing is written there
    finally:
        for p in (ds, di, dw, dg, dgw):
            ctx.dev_free(p)


# ------------------------------------------------------------------ 4. error codes
def test_error_codes(ctx):
    L, h = ctx.L, ctx.h
    c, _, _ = reference("r4_nt7_full")
    nt, nr, M = c["nt"], c["nr"], c["M"]
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    info = C.c_int(0)

    def setup_rc(nt=nt, nr=nr, ybar=c["ybar"], A=c["A"], z=c["z"], S=c["S"], sd=None, rel=None):
        return L.gpemu_calib_setup(h, nt, nr, dp(ybar), dp(A), dp(z), dp(S), dp(sd), dp(rel), C.byref(info))

    ctx.calib_release()
    stat, worst = np.empty((5, M)), np.empty(M, dtype=np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    ev = lambda M=M, mean=c["mean"], var=c["var"], ld=c["mean"].shape[1], st=stat, w=worst: \
        L.gpemu_calib_eval(h, M, dp(mean), dp(var), ld, dp(st), None if w is None else ip(w))
    assert ev() == abi.ERR_STATE                               # no set-up
    # set-up: NULL pointers, both / neither of S and sd, sizes beyond the limits, non-finite input, sd <= 0, bad rel
    sdv = np.full(nt, 0.1)
    assert setup_rc(ybar=None) == abi.ERR_ARG and setup_rc(A=None) == abi.ERR_ARG and setup_rc(z=None) == abi.ERR_ARG
    assert setup_rc(S=None) == abi.ERR_ARG and setup_rc(sd=sdv) == abi.ERR_ARG
    assert L.gpemu_calib_setup(h, nt, nr, dp(c["ybar"]), dp(c["A"]), dp(c["z"]), dp(c["S"]), None, None, None) == abi.ERR_ARG
    assert setup_rc(nr=0) == abi.ERR_ARG and setup_rc(nt=0) == abi.ERR_ARG and setup_rc(nr=nt + 1) == abi.ERR_ARG
    assert setup_rc(nr=abi.CALIB_MAX_R + 1, nt=abi.CALIB_MAX_R + 2) == abi.ERR_ARG
    assert setup_rc(nt=abi.CALIB_MAX_NT + 1) == abi.ERR_ARG
    bad = c["z"].copy(); bad[1] = np.inf
    assert setup_rc(z=bad) == abi.ERR_ARG
    bad = c["A"].copy(); bad[2, 1] = np.nan
    assert setup_rc(A=bad) == abi.ERR_ARG
    bad = sdv.copy(); bad[3] = 0.0
    assert setup_rc(S=None, sd=bad) == abi.ERR_ARG
    bad = np.zeros(nt); bad[0] = -0.1
    assert setup_rc(rel=bad) == abi.ERR_ARG
    # not positive definite: S (pivot 2), and G through a column of A that is zero (pivot 3)
    Sb = c["S"].copy(); Sb[1, 1] = -1.0
    assert setup_rc(S=Sb) == abi.ERR_NOT_PD and info.value == 2
    Ab = c["A"].copy(); Ab[:, 2] = 0.0
    assert setup_rc(A=Ab) == abi.ERR_NOT_PD and info.value == 3
    assert ev() == abi.ERR_STATE                               # a failed set-up leaves none
    # a good set-up; eval: NULL pointers, M < 1, ld < M
    assert setup_rc() == abi.OK and info.value == 0
    assert ev() == abi.OK
    assert ev(mean=None) == abi.ERR_ARG and ev(var=None) == abi.ERR_ARG and ev(st=None) == abi.ERR_ARG and ev(w=None) == abi.ERR_ARG
    assert ev(M=0) == abi.ERR_ARG and ev(ld=M - 1) == abi.ERR_ARG
    # select: NULL pointers, M < 1, level outside 1 .. 3, a NaN cut
    idx, n = np.empty(M, dtype=np.int32), C.c_int(0)
    sel = lambda M=M, st=stat, level=1, c2=np.inf, cI=3.0, ix=idx, cnt=C.byref(n): \
        L.gpemu_calib_select(h, M, dp(st), c2, level, cI, None if ix is None else ip(ix), cnt)
    assert sel() == abi.OK
    assert sel(st=None) == abi.ERR_ARG and sel(ix=None) == abi.ERR_ARG and sel(cnt=None) == abi.ERR_ARG and sel(M=0) == abi.ERR_ARG
    assert sel(level=0) == abi.ERR_ARG and sel(level=4) == abi.ERR_ARG and sel(c2=np.nan) == abi.ERR_ARG and sel(cI=np.nan) == abi.ERR_ARG
    # the tables survive gpemu_set_model; after the release: GPEMU_ERR_STATE again
    from madaiemulator_amd import synth
    X, y = synth.design(70, 2, 5)
    ctx.set_model(abi.POWEREXP, 1, X, y)
    s1 = stat.copy()
    assert ev() == abi.OK and s1.tobytes() == stat.tobytes()
    ctx.calib_release()
    assert ev() == abi.ERR_STATE
    assert L.gpemu_calib_release(None) == abi.ERR_ARG
