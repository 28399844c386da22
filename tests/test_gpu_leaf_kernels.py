"""The 64-column Cholesky leaf kernels one launch at a time through gpemu_test_leaf_launch -- leaf_factor_kernel, the four
leaf_solve_kernel<STAGED, PRE> with the deferred-rows workgroup (c0b), leaf_pair_kernel with and without its factor-ahead
tile -- against tests/leafref.py: every element of the arena is unchanged bit for bit, a value inside a derived bar, or
unspecified (the contract and the bars are in leafref's docstring; tests/test_leafref.py holds the same inputs against the
bars on the CPU).  Everything that is not an operand is NaN, inside the footprint too: the upper triangles of the diagonal
16 x 16 blocks, blocks (0,2) and (1,3), the parked inverses for pre = 0, the rows behind m_below, the gaps of a batch.
Matrix b of a batch is the case's matrix times 4^b (every value scales exactly, so the CPU self-test covers it).

Measured error / bar on an MI355X is printed by every test and collected in DESIGN.md."""
import ctypes as C

import numpy as np
import pytest

import leafref as R
from madaiemulator_amd import abi

pytestmark = pytest.mark.gpu

BASES = ((192, 0), (200, 64))                    # (ld, c0)
FORMS = ((0, 1), (1, 1), (0, 0), (1, 0))         # (staged, pre)
WORST = {}


def note(key, value, what=""):
    WORST[key] = max(WORST.get(key, 0.0), value)
    assert value < 1, (key, value, what)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def launch(ctx, arena, lay, **args):
    return ctx.test_leaf_launch(arena, **lay, **args)


def assert_unchanged(what, before, after, cls):
    keep = cls == R.UNCHANGED
    diff = np.flatnonzero(keep & (bits(before) != bits(after)))
    assert diff.size == 0, (what, f"{diff.size} elements outside the result changed, the first at arena index", diff[:8].tolist(),
                            after[diff[:8]].tolist())


def nblk(lay):
    return max(lay["nbatch"], 1)


def block(arena, lay, rows, b, c0):
    return R.matrix(arena, lay, rows, b)[c0:c0 + 64, c0:c0 + 64]


def staged_problem(Ks, ld, c0, nbatch, extra_rows=2, pair=False):
    """arena with matrix b filled from Ks[b] at c0; extra_rows NaN rows behind the panel"""
    rows = c0 + Ks[0].shape[0] + extra_rows
    arena, lay = R.layout(ld, rows, nbatch)
    for b in range(nblk(lay)):
        R.fill(R.matrix(arena, lay, rows, b), c0, Ks[b], pair=pair)
    return arena, lay, rows


def batch_of(K, nbatch):
    return [K * 4.0 ** b for b in range(max(nbatch, 1))]


def factored(ctx, arena, lay, rows, c0):
    got, info = launch(ctx, arena, lay, op=R.FACTOR, c0=c0)
    assert not info.any(), info
    assert_unchanged("factor", arena, got, R.classes(arena.size, lay, rows, dict(op=R.FACTOR, c0=c0)))
    return got


def without_parked(arena, lay, rows, *c0s):
    out = arena.copy()
    for b in range(nblk(lay)):
        for c0 in c0s:
            D = block(out, lay, rows, b, c0)
            for r, c in R.PARKED:
                D[16 * r:16 * r + 16, 16 * c:16 * c + 16] = np.nan
    return out


# ------------------------------------------------------------------ factor
@pytest.mark.parametrize("nbatch", [0, 3])
@pytest.mark.parametrize("cls", R.INPUT_CLASSES)
def test_factor(gpu_ctx, cls, nbatch):
    for (ld, c0), m in zip(BASES, (1, 130)):
        K = R.problem(cls, R.seed(cls, m), m)[:64, :64]
        Ks = batch_of(K, nbatch)
        arena, lay, rows = staged_problem(Ks, ld, c0, nbatch)
        got = factored(gpu_ctx, arena, lay, rows, c0)
        for b, Kb in enumerate(Ks):
            blk = block(got, lay, rows, b, c0)
            res = R.check_factor(Kb, blk)
            print(f"factor {cls} ld {ld} c0 {c0} matrix {b}/{nbatch}: error/bar factor {res['factor']:.3f} inverses {res['inverse']:.3f}")
            note(("factor", cls), res["factor"])
            note(("parked inverse", cls), res["inverse"])
            if cls == "well":
                L = np.linalg.cholesky(Kb)
                err = np.max(np.abs(np.tril(blk) - L)) / np.max(np.abs(L))
                assert err < 1e-13, err


# ------------------------------------------------------------------ failed pivots
def _failed_factor(ctx, K, row_expected, what):
    """single matrix at (192, 0), and the middle of a batch of 3 at (200, 64) between two healthy matrices"""
    good = R.problem("well", R.seed("well", 2), 2)[:64, :64]
    for (ld, c0), nbatch in zip(BASES, (0, 3)):
        Ks = [K] if nbatch == 0 else [good, K, good * 4.0]
        arena, lay, rows = staged_problem(Ks, ld, c0, nbatch)
        got, info = launch(ctx, arena, lay, op=R.FACTOR, c0=c0)
        bad = 0 if nbatch == 0 else 1
        want = [0] * nblk(lay)
        want[bad] = c0 + row_expected
        assert list(info) == want, (what, list(info), want)
        assert_unchanged(what, arena, got, R.classes(arena.size, lay, rows, dict(op=R.FACTOR, c0=c0), failed=(bad,)))
        for b, Kb in enumerate(Ks):
            if b != bad:
                res = R.check_factor(Kb, block(got, lay, rows, b, c0))
                note(("factor", "well"), res["factor"], what)
                note(("parked inverse", "well"), res["inverse"], what)


@pytest.mark.parametrize("row", R.FAIL_ROWS)
def test_failed_pivot_row(gpu_ctx, row):
    _failed_factor(gpu_ctx, R.fail_pivot(R.problem("well", 7, 0), row), row, f"pivot {row} negative")


def test_failed_pivot_nan_zero_and_two(gpu_ctx):
    K = R.problem("well", 7, 0)
    for row in (1, 17, 64):
        _failed_factor(gpu_ctx, R.fail_pivot(K, row, "nan"), row, f"pivot {row} NaN")
    _failed_factor(gpu_ctx, R.fail_pivot(K, 1, "zero"), 1, "pivot 1 exactly 0.0")
    _failed_factor(gpu_ctx, R.fail_pivot(K, (33, 17)), 17, "pivots 17 and 33 fail: the first is reported")


def test_failed_pivot_in_the_pair_tile(gpu_ctx):
    """the factor-ahead tile of the pair reports c0 + 64 + row; in a batch of 3 only the middle matrix fails and the
    others leave as full factors"""
    for row in R.FAIL_ROWS:
        K, _ = R.pair_problem_with_failed_tile("well", 64, row)
        good = R.problem("well", R.seed("well", 64), 64)
        for (ld, c0), nbatch in zip(BASES, (0, 3)) if row == 17 else (((200, 64), 0),):
            Ks = [K] if nbatch == 0 else [good, K, good * 4.0]
            arena, lay, rows = staged_problem(Ks, ld, c0, nbatch, pair=True)
            a1 = factored(gpu_ctx, arena, lay, rows, c0)
            solved, _ = launch(gpu_ctx, a1, lay, op=R.SOLVE, c0=c0, m_below=64, staged=0, pre=1)
            args = dict(op=R.PAIR, c0=c0, m_below=64, fa=1)
            got, info = launch(gpu_ctx, a1, lay, **args)
            bad = 0 if nbatch == 0 else 1
            want = [0] * nblk(lay)
            want[bad] = c0 + 64 + row
            assert list(info) == want, (row, list(info), want)
            assert_unchanged(f"pair tile fails at {row}", a1, got, R.classes(a1.size, lay, rows, args, failed=(bad,)))
            for b, Kb in enumerate(Ks):
                if b != bad:
                    X = R.matrix(solved, lay, rows, b)[c0 + 64:c0 + 128, c0:c0 + 64]
                    out = R.matrix(got, lay, rows, b)[c0 + 64:c0 + 128, c0 + 64:c0 + 128]
                    res = R.check_update(Kb[64:, 64:128], X, X, out, 1)
                    for k in ("factor", "inverse"):
                        note(("pair " + k, "well"), res[k])


# ------------------------------------------------------------------ solve
def _solve_all_forms(ctx, what, a1, lay, rows, c0, m, cls, **more):
    """the four forms on the factored arena a1 (pre = 0: parked blocks NaN): the same bits in every VALUE element, each
    within the step-wise bars, nothing else changed -> the arena after the first form"""
    args = dict(op=R.SOLVE, c0=c0, m_below=m, **more)
    kinds = R.classes(a1.size, lay, rows, args)
    outs = []
    for staged, pre in FORMS:
        before = a1 if pre else without_parked(a1, lay, rows, c0, *([more["c0b"]] if "c0b" in more else []))
        got, info = launch(ctx, before, lay, staged=staged, pre=pre, **args)
        assert not info.any()
        assert_unchanged(f"{what} staged {staged} pre {pre}", before, got, kinds)
        worst = 0.0
        for b in range(nblk(lay)):
            M0, M1 = R.matrix(a1, lay, rows, b), R.matrix(got, lay, rows, b)
            worst = max(worst, R.check_solve(M0[c0:c0 + 64, c0:c0 + 64], M0[c0 + 64:c0 + 64 + m, c0:c0 + 64],
                                             M1[c0 + 64:c0 + 64 + m, c0:c0 + 64]))
        print(f"{what} staged {staged} pre {pre}: error/bar {worst:.3f}")
        note((f"solve staged {staged} pre {pre}", cls), worst, what)
        outs.append(got)
    val = kinds == R.VALUE
    for (staged, pre), o in zip(FORMS[1:], outs[1:]):
        assert np.array_equal(bits(outs[0])[val], bits(o)[val]), (what, "forms differ", staged, pre)
    return outs[0]


@pytest.mark.parametrize("m", R.SOLVE_M)
@pytest.mark.parametrize("cls", R.INPUT_CLASSES)
def test_solve_forms(gpu_ctx, cls, m):
    K = R.problem(cls, R.seed(cls, m), m)
    for (ld, c0), nbatch in zip(BASES, (0, 3)):
        arena, lay, rows = staged_problem(batch_of(K, nbatch), ld, c0, nbatch, extra_rows=3)
        a1 = factored(gpu_ctx, arena, lay, rows, c0)
        out = _solve_all_forms(gpu_ctx, f"solve {cls} m {m} ld {ld} c0 {c0} batch {nbatch}", a1, lay, rows, c0, m, cls)
        # the plain leaf (factor + solve in one call, automatic form) is the two launches
        both, info = launch(gpu_ctx, arena, lay, op=R.FACTOR_SOLVE, c0=c0, m_below=m)
        assert not info.any() and np.array_equal(bits(both), bits(out))


@pytest.mark.parametrize("m", [17, 64, 130])
@pytest.mark.parametrize("cls", R.INPUT_CLASSES)
def test_solve_with_deferred_rows(gpu_ctx, cls, m):
    """c0b = c0 - 64: the extra workgroup solves the 64 rows under the block at c0b to the bits of an ordinary solve of
    them, and the rest of the launch is what it is without c0b"""
    ld, c0, c0b = 200, 64, 0
    K0, K1 = R.problem(cls, R.seed(cls, 64), 64), R.problem(cls, R.seed(cls, m), m)
    for nbatch in (0, 3):
        rows = 128 + m + 2
        arena, lay = R.layout(ld, rows, nbatch)
        for b in range(nblk(lay)):
            R.fill(R.matrix(arena, lay, rows, b), c0b, K0 * 4.0 ** b)
            R.fill(R.matrix(arena, lay, rows, b), c0, K1 * 4.0 ** b)
        a1 = factored(gpu_ctx, factored(gpu_ctx, arena, lay, rows, c0b), lay, rows, c0)
        out = _solve_all_forms(gpu_ctx, f"deferred rows {cls} m {m} batch {nbatch}", a1, lay, rows, c0, m, cls, c0b=c0b)
        first, _ = launch(gpu_ctx, a1, lay, op=R.SOLVE, c0=c0b, m_below=64, staged=0, pre=1)
        plain, _ = launch(gpu_ctx, a1, lay, op=R.SOLVE, c0=c0, m_below=m, staged=0, pre=1)
        for b in range(nblk(lay)):
            Mo, Mf, Mp, M1 = (R.matrix(x, lay, rows, b) for x in (out, first, plain, a1))
            assert R.same_bits(Mo[64:128, 0:64], Mf[64:128, 0:64]), (b, "the deferred rows")
            assert R.same_bits(Mo[128:, 64:128], Mp[128:, 64:128]), (b, "the launch's own rows")
            note(("solve deferred rows", cls), R.check_solve(M1[0:64, 0:64], M1[64:128, 0:64], Mo[64:128, 0:64]))


@pytest.mark.parametrize("m", [1024, 960])
def test_solve_automatic_form_both_sides_of_the_rule(gpu_ctx, m):
    """staged = -1, 64 matrices of ld 64: 16 x 64 = 1024 workgroups take the staged form, 15 x 64 = 960 the direct one;
    either way the bits of both explicit forms"""
    K = R.problem("well", R.seed("well", 64), 64)[:64, :64]
    arena, lay, rows = staged_problem([K], 64, 0, 0, extra_rows=0)
    blk = block(factored(gpu_ctx, arena, lay, rows, 0), lay, rows, 0, 0).copy()
    rows = 64 + m
    arena, lay = R.layout(64, rows, 64)
    for b in range(64):
        M = R.matrix(arena, lay, rows, b)
        M[:64] = blk
        M[64:] = R.big_rows(b, m)
    args = dict(op=R.SOLVE, c0=0, m_below=m, pre=1)
    outs = [launch(gpu_ctx, arena, lay, staged=s, **args)[0] for s in (-1, 0, 1)]
    assert_unchanged("automatic form", arena, outs[0], R.classes(arena.size, lay, rows, args))
    assert np.array_equal(bits(outs[0]), bits(outs[1])) and np.array_equal(bits(outs[0]), bits(outs[2]))
    for b in (0, 63):
        note(("solve automatic", "well"), R.check_solve(blk, R.matrix(arena, lay, rows, b)[64:], R.matrix(outs[0], lay, rows, b)[64:]))


@pytest.mark.parametrize("m", [1, 17, 64, 130])
def test_solve_integer_case_is_exact(gpu_ctx, m):
    blk, B, _, X = R.int_problem(m, m)
    for (ld, c0), nbatch in zip(BASES, (0, 3)):
        rows = c0 + 64 + m + 1
        arena, lay = R.layout(ld, rows, nbatch)
        for b in range(nblk(lay)):
            M = R.matrix(arena, lay, rows, b)
            M[c0:c0 + 64, c0:c0 + 64] = blk
            M[c0 + 64:c0 + 64 + m, c0:c0 + 64] = B * (b + 1)
        out = _solve_all_forms(gpu_ctx, f"integer solve m {m}", arena, lay, rows, c0, m, "integer")
        for b in range(nblk(lay)):
            assert np.array_equal(R.matrix(out, lay, rows, b)[c0 + 64:c0 + 64 + m, c0:c0 + 64], X * (b + 1))


# ------------------------------------------------------------------ pair
def _pair_case(ctx, Ks, ld, c0, nbatch, m):
    arena, lay, rows = staged_problem(Ks, ld, c0, nbatch, extra_rows=1, pair=True)
    a1 = factored(ctx, arena, lay, rows, c0)
    solved, _ = launch(ctx, a1, lay, op=R.SOLVE, c0=c0, m_below=m, staged=1, pre=1)
    return a1, lay, rows, solved


@pytest.mark.parametrize("nbatch", [0, 3])
@pytest.mark.parametrize("m", R.PAIR_M)
@pytest.mark.parametrize("cls", R.INPUT_CLASSES)
def test_pair(gpu_ctx, cls, m, nbatch):
    K = R.problem(cls, R.seed(cls, m), m)
    Ks = batch_of(K, nbatch)
    for ld, c0 in BASES:
        a1, lay, rows, solved = _pair_case(gpu_ctx, Ks, ld, c0, nbatch, m)
        for fa in (0, 1):
            what = f"pair {cls} m {m} ld {ld} c0 {c0} batch {nbatch} fa {fa}"
            args = dict(op=R.PAIR, c0=c0, m_below=m, fa=fa)
            got, info = launch(gpu_ctx, a1, lay, **args)
            assert not info.any(), (what, info)
            # the diagonal block and the first 64 rows of columns c0 .. c0+63 are in the unchanged class
            assert_unchanged(what, a1, got, R.classes(a1.size, lay, rows, args))
            for b, Kb in enumerate(Ks):
                Mg, Ms = R.matrix(got, lay, rows, b), R.matrix(solved, lay, rows, b)
                assert R.same_bits(Mg[c0 + 128:c0 + 64 + m, c0:c0 + 64], Ms[c0 + 128:c0 + 64 + m, c0:c0 + 64]), (what, b, "solved rows")
                X = Ms[c0 + 64:c0 + 64 + m, c0:c0 + 64]
                res = R.check_update(Kb[64:, 64:128], X, X[:64], Mg[c0 + 64:c0 + 64 + m, c0 + 64:c0 + 128], fa)
                print(what, "matrix", b, {k: f"{v:.3g}" for k, v in res.items()})
                assert res.pop("relerr") < 1e-13 or cls != "well"
                for k, v in res.items():
                    note(("pair " + k, cls), v, what)


@pytest.mark.parametrize("m", [64, 128, 320])
def test_pair_integer_case_is_exact(gpu_ctx, m):
    blk, B, C2, X = R.int_problem(m, m)
    for (ld, c0), nbatch in zip(BASES, (0, 3)):
        rows = c0 + 64 + m + 1
        arena, lay = R.layout(ld, rows, nbatch)
        for b in range(nblk(lay)):
            M = R.matrix(arena, lay, rows, b)
            M[c0:c0 + 64, c0:c0 + 64] = blk
            M[c0 + 64:c0 + 64 + m, c0:c0 + 64] = B * (b + 1)
            M[c0 + 64:c0 + 64 + m, c0 + 64:c0 + 128] = C2
            M[c0 + 64:c0 + 128, c0 + 64:c0 + 128][np.triu_indices(64, 1)] = np.nan
        args = dict(op=R.PAIR, c0=c0, m_below=m, fa=0)
        got, _ = launch(gpu_ctx, arena, lay, **args)
        assert_unchanged(f"integer pair m {m}", arena, got, R.classes(arena.size, lay, rows, args))
        i, j = np.indices((m, 64))
        for b in range(nblk(lay)):
            Mg = R.matrix(got, lay, rows, b)
            Xb = X * (b + 1)
            assert np.array_equal(Mg[c0 + 128:c0 + 64 + m, c0:c0 + 64], Xb[64:])
            assert np.array_equal(Mg[c0 + 64:c0 + 64 + m, c0 + 64:c0 + 128][i >= j], (C2 - Xb @ Xb[:64].T)[i >= j])


@pytest.mark.parametrize("nbatch", [0, 3])
@pytest.mark.parametrize("fa", [0, 1])
@pytest.mark.parametrize("m", [128, 320])
def test_pair_sequence_equals_the_two_launch_path(gpu_ctx, m, fa, nbatch):
    """pair, then the second block's leaf with c0b  ==  leaf solve, K = 64 triangular update on 64 x 64 tiles (same fa), then
    the second block's leaf: every specified element the same bits (the claim of leaf_pair_kernel's header comment)"""
    for cls, (ld, c0) in zip(("well", "cov2"), BASES):
        K = R.problem(cls, R.seed(cls, m), m)
        a1, lay, rows, solved = _pair_case(gpu_ctx, batch_of(K, nbatch), ld, c0, nbatch, m)
        second = dict(op=R.SOLVE if fa else R.FACTOR_SOLVE, c0=c0 + 64, m_below=m - 64)
        p, info_p = launch(gpu_ctx, a1, lay, op=R.PAIR, c0=c0, m_below=m, fa=fa)
        one, info_1 = launch(gpu_ctx, p, lay, c0b=c0, **second)
        row0 = lay["off"] + (c0 + 64) * ld
        g, info_g = gpu_ctx.test_gemm_launch(solved, offC=row0 + c0 + 64, offA=row0, offB=row0, ldc=ld, lda=ld, ldb=ld,
                                             bsC=lay["bstride"], bsA=lay["bstride"], bsB=lay["bstride"], alpha=-1.0, beta=1,
                                             m=m, n=64, k0=c0, k1=c0 + 64, tri=1, nbatch=nbatch, force_cfg=2, fa=fa, fa_c0=c0 + 64)
        two, info_2 = launch(gpu_ctx, g, lay, **second)
        assert not (info_p.any() or info_1.any() or info_g.any() or info_2.any())
        spec = np.ones(a1.size, dtype=bool)
        free = ~R.written_by_factor()
        for b in range(nblk(lay)):
            R.matrix(spec, lay, rows, b)[c0 + 64:c0 + 128, c0 + 64:c0 + 128][free] = False
        diff = np.flatnonzero(spec & (bits(one) != bits(two)))
        assert diff.size == 0, (cls, m, fa, nbatch, diff.size, diff[:8].tolist())
        assert not np.isnan(R.matrix(one, lay, rows, nblk(lay) - 1)[c0 + 64:c0 + 64 + m, c0:c0 + 64]).any()


# ------------------------------------------------------------------ refused launches
def _raw(ctx, arena, args, null=None):
    """the C entry itself on a copy of the arena -> (return code, the copy afterwards)"""
    out = np.ascontiguousarray(arena, dtype=np.float64).copy()
    a = abi.LeafLaunchArgs(**{k: int(v) for k, v in args.items()})
    info = np.zeros(64, dtype=np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    rc = ctx.L.gpemu_test_leaf_launch(ctx.h, None if null == "arena" else out.ctypes.data_as(dp), out.size,
                                      None if null == "args" else C.byref(a), None if null == "info" else info.ctypes.data_as(ip))
    return rc, out


def test_refused_arguments(gpu_ctx):
    """every rule of the entry, one changed argument at a time from a launch that works: GPEMU_ERR_ARG, arena unchanged"""
    m, ld, c0 = 17, 200, 64
    K0, K1 = R.problem("well", R.seed("well", 64), 64), R.problem("well", R.seed("well", m), m)
    rows = 128 + 64
    arena, lay = R.layout(ld, rows, 3)
    for b in range(3):
        R.fill(R.matrix(arena, lay, rows, b), 0, K0)
        R.fill(R.matrix(arena, lay, rows, b), c0, K1, pair=False)
        R.matrix(arena, lay, rows, b)[128:192, 64:192] = 1.0
    arena = factored(gpu_ctx, factored(gpu_ctx, arena, lay, rows, 0), lay, rows, c0)
    solve = dict(lay, op=R.SOLVE, c0=c0, m_below=m, staged=1, pre=1, c0b=0, fa=0)
    pair = dict(lay, op=R.PAIR, c0=0, m_below=128, staged=-1, pre=1, c0b=-1, fa=1)
    factor = dict(lay, op=R.FACTOR, c0=c0, m_below=0, staged=-1, pre=1, c0b=-1, fa=0)
    for base in (solve, pair, factor):
        assert _raw(gpu_ctx, arena, base)[0] == 0                  # the base launches themselves are fine
    # the shortest arena that holds the solve: the last element of the last matrix's footprint is its last element
    need = lay["off"] + 2 * lay["bstride"] + (c0 + 64 + m - 1) * ld + c0 + 63 + 1
    assert _raw(gpu_ctx, arena[:need], solve)[0] == 0
    refused = [
        ("op = 4", solve, dict(op=4)), ("op = -1", solve, dict(op=-1)),
        ("staged = 2", solve, dict(staged=2)), ("staged = -2", solve, dict(staged=-2)),
        ("pre = 2", solve, dict(pre=2)), ("pre = -1", solve, dict(pre=-1)),
        ("fa = 2", pair, dict(fa=2)), ("fa without the pair", solve, dict(fa=1)),
        ("c0b = -2", solve, dict(c0b=-2)),
        ("nbatch = -1", solve, dict(nbatch=-1)), ("nbatch = 65", solve, dict(nbatch=65)),
        ("pair with m_below = 32", pair, dict(m_below=32)), ("pair with m_below = 96", pair, dict(m_below=96)),
        ("pair with m_below = 0", pair, dict(m_below=0)),
        ("solve with m_below = 0", solve, dict(m_below=0)), ("solve with m_below = -1", solve, dict(m_below=-1)),
        ("factor with m_below = 1", factor, dict(m_below=1)),
        ("odd off", solve, dict(off=lay["off"] + 1)), ("odd ld", solve, dict(ld=ld - 1)), ("odd c0", solve, dict(c0=c0 + 1)),
        ("odd c0b", solve, dict(c0b=1)), ("odd bstride", solve, dict(bstride=lay["bstride"] + 1)),
        ("c0b with the factor alone", factor, dict(c0b=0)), ("c0b with the pair", pair, dict(c0b=0)),
        ("off before the arena", solve, dict(off=-2)),
        ("the rows of the last matrix leave the arena", solve, dict(m_below=rows)),
        ("the last matrix lies outside", solve, dict(bstride=arena.size)),
        ("the block at c0b leaves the arena", solve, dict(c0b=130)),
        ("the pair's columns leave the row", pair, dict(c0=ld - 126)),
        ("a negative stride leaves the arena at the front", solve, dict(bstride=-lay["bstride"])),
    ]
    for why, base, change in refused:
        rc, out = _raw(gpu_ctx, arena, dict(base, **change))
        assert rc == abi.ERR_ARG, (why, rc)
        assert np.array_equal(bits(out), bits(arena)), why
    rc, out = _raw(gpu_ctx, arena[:need - 1], solve)               # one element short for the last matrix of the batch
    assert rc == abi.ERR_ARG and np.array_equal(bits(out), bits(arena[:need - 1]))
    for null in ("arena", "args", "info"):
        rc, out = _raw(gpu_ctx, arena, solve, null=null)
        assert rc == abi.ERR_ARG and np.array_equal(bits(out), bits(arena)), null
    a = abi.LeafLaunchArgs(**{k: int(v) for k, v in solve.items()})
    assert gpu_ctx.L.gpemu_test_leaf_launch(None, None, 0, C.byref(a), None) == abi.ERR_ARG
    with pytest.raises(abi.GpemuError) as e:
        gpu_ctx.test_leaf_launch(arena, **dict(solve, op=7))
    assert e.value.code == abi.ERR_ARG


def test_worst_ratios_report():
    """the largest error / bar of this session per kernel and input class (every one asserted < 1 where it was measured)"""
    for k in sorted(WORST):
        print(f"worst error/bar  {k[0]:<28s} {k[1]:<8s} {WORST[k]:.3f}")
    assert all(v < 1 for v in WORST.values())
