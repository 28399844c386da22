"""Every launch mode of gemm_nt_kernel, one launch at a time through gpemu_test_gemm_launch, against tests/gemmref.py.

Exact method: the operands are integers in [-8, 8], so every product and partial sum is an exact fp64 integer and the
numpy product is the only correct answer in any summation order; these cases assert equality, element by element, and
state no tolerance.  Every launch is also checked for what it must NOT touch: the whole arena comes back, and everything
outside the C rectangles (padding columns, rows past m, the gaps between the matrices of a batch, the guard bands, A and
B) must have the bits that were uploaded.  The background holds non-integers, so a read outside the operands shows as
well.  A failure prints mode, tile shape, matrix of the batch, (i, j), got, want and the class of the element
(gemmref.mismatches).

The only tolerances are the two the suite already uses: relerr < 1e-13 (error relative to the largest element) for
standard-normal operands at K <= 256 (test_gemm_nt_asymmetric) and for the 64x64 factor (test_potrf_matches_lapack)."""
import numpy as np
import pytest

import gemmref as R
from madaiemulator_amd import abi

pytestmark = pytest.mark.gpu

CFGS = (2, 8)            # force_cfg: 64x64 tiles, 128x128 tiles
RELERR = 1e-13


def relerr(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _ctx_with_env(monkeypatch, env, device=0):
    """a context whose schedule switches come from `env` (copied into the context when it is created)"""
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    c = abi.Context(device)
    for k_ in env:
        monkeypatch.delenv(k_)
    return c


def run_exact(ctx, what, arena, args, cfgs=CFGS, quantum=1.0, fa_failed=(), ref=None):
    """one launch per tile shape; every element of the arena in its class (gemmref), both shapes the same bits.
    ref: (want, mask) of an earlier call with the same arena and args.
    -> (want, mask, [arena after the launch per cfg], [info per cfg])"""
    want, mask = ref or R.expected(arena, args, exact=True, quantum=quantum, fa_failed=fa_failed)
    outs, infos = [], []
    for cfg in cfgs:
        got, info = ctx.test_gemm_launch(arena, **dict(args, force_cfg=cfg))
        count, lines = R.mismatches(got, want, arena, mask, args)
        if count:
            print(f"{what}, cfg {cfg}: {count} elements wrong, the first:")
            print("\n".join(lines))
        assert count == 0, (what, cfg, count, lines[:2])
        outs.append(got)
        infos.append(info)
    for o in outs[1:]:
        assert np.array_equal(outs[0][mask == R.MUST], o[mask == R.MUST]), what
    return want, mask, outs, infos


def run_rounded(ctx, what, arena, args, cfgs=CFGS):
    """standard-normal operands: the must-equal elements at the suite's 1e-13 bar against float64 numpy, both tile shapes
    the same bits, everything outside the C rectangles untouched"""
    want, mask = R.expected(arena, args, exact=False)
    must = mask == R.MUST
    outs = []
    for cfg in cfgs:
        got, _ = ctx.test_gemm_launch(arena, **dict(args, force_cfg=cfg))
        bg = mask == R.BACKGROUND
        assert np.array_equal(got[bg].view(np.int64), arena[bg].view(np.int64)), (what, cfg)
        err = relerr(got[must], want[must])
        print(f"{what}, cfg {cfg}: relerr {err:.3e} (bar {RELERR:.0e})")
        assert err < RELERR, (what, cfg, err)
        outs.append(got)
    for o in outs[1:]:
        assert np.array_equal(outs[0][must], o[must]), what
    return outs


ALPHA_BETA = ((-1.0, 1), (1.0, 0), (0.5, 0))     # the update, the plain product, the general-alpha epilogue (a power of two: exact)


# ------------------------------------------------------------------ dense
@pytest.mark.parametrize("m,n,K", [(64, 64, 16), (129, 257, 48), (200, 72, 64), (320, 320, 2048)])
def test_dense_padded_and_offset(gpu_ctx, m, n, K):
    """lda, ldb > K, ldc > n, k0 = 32 with non-zero, non-integer columns before it; C, A and B inside ONE matrix with one
    leading dimension, as in the trailing update"""
    arena, args = R.case_trailing(np.random.default_rng(m * 13 + n + K), m, n, K, 1.0, 0)
    assert args["k0"] == 32 and args["lda"] > args["k1"] + n and args["offA"] == args["offB"]
    for alpha, beta in ALPHA_BETA:
        run_exact(gpu_ctx, f"dense {m}x{n}x{K} alpha {alpha} beta {beta}", arena, dict(args, alpha=alpha, beta=beta))


@pytest.mark.parametrize("m", [63, 64, 65, 127, 128, 129])
def test_ragged_launch_leaves_its_neighbours_alone(gpu_ctx, m):
    """m and n one below, at and one above both tile sizes: the rows and columns just outside C keep their bits"""
    for n in (63, 64, 65, 127, 128, 129):
        arena, args = R.case_trailing(np.random.default_rng(m * 131 + n), m, n, 32, 1.0, 0)
        for alpha, beta in ALPHA_BETA[:2]:
            run_exact(gpu_ctx, f"ragged {m}x{n} alpha {alpha} beta {beta}", arena, dict(args, alpha=alpha, beta=beta))


# ------------------------------------------------------------------ triangular update
TRI_SHAPES = [(64, 64), (320, 320), (576, 576), (448, 320)]


def _tri_case(m, n, K=32):
    arena, args = R.case_trailing(np.random.default_rng(m * 17 + n), m, n, K, -1.0, 1, tri=1)
    assert args["offA"] == args["offB"]          # A is B: the SYRK form of the factorisation's updates
    return arena, args


@pytest.mark.parametrize("m,n", TRI_SHAPES)
def test_triangular_update(gpu_ctx, m, n):
    """tri, alpha = -1, beta = 1, dense enumeration of the lower-triangular tiles (order_mode 2); the elements above the
    diagonal are old or fully updated, never anything else"""
    arena, args = _tri_case(m, n)
    run_exact(gpu_ctx, f"tri {m}x{n}", arena, args)


def test_triangular_update_with_busy_idle_waves(monkeypatch):
    """GPEMU_IDLE_WAVES=0: the waves above the diagonal of a diagonal tile compute and store their output"""
    c = _ctx_with_env(monkeypatch, {"GPEMU_IDLE_WAVES": "0"})
    try:
        for m, n in TRI_SHAPES:
            arena, args = _tri_case(m, n)
            want, mask, outs, _ = run_exact(c, f"tri {m}x{n}, idle waves compute", arena, args)
            # with idle waves off, every tile that is launched is stored whole: 64x64 tiles with tn <= tm
            got = R.mat(outs[0], args["offC"], args["ldc"], m, n)
            full = R.mat(want, args["offC"], args["ldc"], m, n)
            i, j = np.indices((m, n))
            assert np.array_equal(got[j // 64 <= i // 64], full[j // 64 <= i // 64])
    finally:
        c.close()


def test_triangular_update_tile_table(gpu_ctx, monkeypatch):
    """2048 x 2048 on 64x64 tiles: 528 >= 512 lower-triangular tiles, the XCD-blocked table (order_mode 3); the same
    launch with GPEMU_GEMM_TABLE=0 (dense enumeration) gives the same arena"""
    arena, args = _tri_case(2048, 2048)
    want, mask, outs, _ = run_exact(gpu_ctx, "tri 2048 table", arena, args, cfgs=(2,))
    c = _ctx_with_env(monkeypatch, {"GPEMU_GEMM_TABLE": "0"})
    try:
        _, _, outs0, _ = run_exact(c, "tri 2048 enumeration", arena, args, cfgs=(2,), ref=(want, mask))
    finally:
        c.close()
    assert np.array_equal(outs[0][mask == R.MUST], outs0[0][mask == R.MUST])


@pytest.mark.parametrize("m,n,cfg", [(1470, 1465, 2), (2940, 2930, 8)])
def test_dense_tile_table(gpu_ctx, m, n, cfg):
    """non-triangular launches of 23 x 23 = 529 >= 512 tiles: the XCD-blocked table, ragged last tile row and column"""
    arena, args = R.case_trailing(np.random.default_rng(m + cfg), m, n, 16, -1.0, 1)
    run_exact(gpu_ctx, f"dense table {m}x{n}", arena, args, cfgs=(cfg,))


# ------------------------------------------------------------------ batch
@pytest.mark.parametrize("tri", [0, 1])
def test_batch_with_three_strides(gpu_ctx, tri):
    arena, args = R.case_batch(np.random.default_rng(40 + tri), 192, 192, 64, 3, tri)
    assert len({args["bsC"], args["bsA"], args["bsB"]}) == 3
    run_exact(gpu_ctx, f"batch of 3, tri {tri}", arena, args)


# ------------------------------------------------------------------ corner product (row-start skipping)
@pytest.mark.parametrize("Np,nbatch", [(192, 0), (192, 2), (448, 0), (448, 2)])
def test_corner_product_enumeration(gpu_ctx, Np, nbatch):
    """C^-1 = U U^T: tri, kstart_mode, kstart_off = 64, A is B = [Z^T; U]; below 16 tile rows the row-major dense
    enumeration of the triangle"""
    arena, args = R.case_corner(np.random.default_rng(Np + nbatch), Np, nbatch)
    assert (Np + 64 + 63) // 64 < 16
    run_exact(gpu_ctx, f"corner Np {Np} batch {nbatch}", arena, args)


@pytest.mark.parametrize("Np,cfg,nbatch", [(960, 2, 0), (960, 2, 2), (1984, 8, 0), (1984, 8, 2)])
def test_corner_product_row_table(gpu_ctx, monkeypatch, Np, cfg, nbatch):
    """16 tile rows: whole tile rows per XCD from the row table; GPEMU_CORNER_ROW_TABLE=0 (enumeration) gives the same"""
    arena, args = R.case_corner(np.random.default_rng(Np + nbatch), Np, nbatch)
    assert (Np + 64) // (64 if cfg == 2 else 128) == 16
    want, mask, outs, _ = run_exact(gpu_ctx, f"corner Np {Np} batch {nbatch} row table", arena, args, cfgs=(cfg,))
    c = _ctx_with_env(monkeypatch, {"GPEMU_CORNER_ROW_TABLE": "0"})
    try:
        _, _, outs0, _ = run_exact(c, f"corner Np {Np} batch {nbatch} enumeration", arena, args, cfgs=(cfg,), ref=(want, mask))
    finally:
        c.close()
    assert np.array_equal(outs[0][mask == R.MUST], outs0[0][mask == R.MUST])


def test_skipping_rounds_towards_the_kept_range(gpu_ctx):
    """The offsets of the two call sites (kstart_off = 64, kend_off = 0) are multiples of 16, where the first kept k-block
    starts and the last one ends on the operand's own boundary and the direction of the rounding cannot show.  The contract
    (GemmArgs: floor_BK for the start, ceil_BK for the end) is pinned here with offsets of 8 modulo 16: a start rounded up or
    an end rounded down drops eight columns in which the operand is not zero."""
    arena, args = R.case_corner(np.random.default_rng(72), 192, 0, off=72)
    assert args["kstart_off"] == 72 and args["m"] == 264
    run_exact(gpu_ctx, "corner, kstart_off 72", arena, args)
    arena, args = R.case_predict(np.random.default_rng(8), 64, 192, kend_off=8)
    assert args["kend_off"] == 8
    run_exact(gpu_ctx, "prediction, kend_off 8", arena, args)


# ------------------------------------------------------------------ prediction product (column-end skipping)
@pytest.mark.parametrize("Np", [192, 1024])
@pytest.mark.parametrize("m", [17, 64, 130])
def test_prediction_product(gpu_ctx, m, Np):
    """kend_mode against [L^-1; 64 dense rows]: n = Np + 64, k1 = Np, ldc = Np + 64"""
    arena, args = R.case_predict(np.random.default_rng(m + Np), m, Np)
    assert args["ldc"] == args["n"] == Np + 64
    run_exact(gpu_ctx, f"prediction m {m} Np {Np}", arena, args)


@pytest.mark.parametrize("Np", [1024, 1040])
@pytest.mark.parametrize("m", [17, 64])
def test_prediction_split_k(gpu_ctx, m, Np):
    """k-slices of the prediction product at C + s * bsC: every slice on its own, and their in-order sum equal to the
    unsplit product.  Np = 1040, ksplit = 3: klen = 352 does not divide 1040, the last slice is short."""
    arena, args = R.case_predict(np.random.default_rng(m + Np), m, Np)
    want1, _ = R.expected(arena, args)
    whole = R.mat(want1, args["offC"], args["ldc"], m, Np + 64)
    for ksplit in (2, 3, 8):
        arena_s, args_s = R.case_predict(np.random.default_rng(m + Np), m, Np, ksplit=ksplit)
        assert args_s["bsC"] == R.round_up(m, 64) * (Np + 64)
        _, _, outs, _ = run_exact(gpu_ctx, f"prediction split-K m {m} Np {Np} ksplit {ksplit}", arena_s, args_s, cfgs=(2,))
        total = np.zeros((m, Np + 64))
        for s in range(ksplit):
            total += R.mat(outs[0], args_s["offC"] + s * args_s["bsC"], args_s["ldc"], m, Np + 64)
        assert np.array_equal(total, whole), (m, Np, ksplit)


# ------------------------------------------------------------------ factor-ahead
def _check_factor(out, args, S, b):
    blk = R.mat(out, args["offC"] + b * args["bsC"], args["ldc"], 64, 64)
    err = relerr(np.tril(blk), np.linalg.cholesky(S[b]))
    print(f"factor-ahead matrix {b}: relerr of the 64x64 factor {err:.3e} (bar {RELERR:.0e})")
    assert err < RELERR, (b, err)


def test_factor_ahead(gpu_ctx):
    """fa: tile (0,0) of a triangular update leaves as the Cholesky factor of the updated block (exactly S = G G^T + 64 I
    here, gemmref.case_factor_ahead), info 0; every other tile is the exact update"""
    arena, args, S = R.case_factor_ahead(np.random.default_rng(71), 256, 64, 2)
    _, _, outs, infos = run_exact(gpu_ctx, "factor-ahead", arena, args, cfgs=(2,), quantum=R.FA_QUANTUM)
    assert list(infos[0]) == [0, 0]
    for b in range(2):
        _check_factor(outs[0], args, S, b)


def test_factor_ahead_reports_the_first_failed_pivot(gpu_ctx):
    """the updated block of matrix 1 has its first non-positive pivot at row 37: info = fa_c0 + 37 (gpemu_test_potrf's
    convention: 1-based, global); matrix 0 of the same batch is factored correctly"""
    arena, args, S = R.case_factor_ahead(np.random.default_rng(72), 256, 64, 2, bad_row=37, bad_matrix=1, fa_c0=128)
    _, _, outs, infos = run_exact(gpu_ctx, "factor-ahead, failed pivot", arena, args, cfgs=(2,), quantum=R.FA_QUANTUM,
                                  fa_failed=(1,))
    assert list(infos[0]) == [0, 128 + 37]
    _check_factor(outs[0], args, S, 0)


# ------------------------------------------------------------------ rounding
def test_rounding_with_normal_operands(gpu_ctx):
    """one pass per mode family with standard-normal operands (the zero patterns stay exact zeros), K <= 256, at the
    suite's bar; the smallest shape of each family (split-K at Np = 192 to stay at K <= 256)"""
    rng = np.random.default_rng(99)
    run_rounded(gpu_ctx, "dense normal", *R.case_trailing(rng, 129, 257, 48, -1.0, 1, kind="normal"))
    run_rounded(gpu_ctx, "dense normal K 256", *R.case_trailing(rng, 200, 72, 256, 1.0, 0, kind="normal"))
    run_rounded(gpu_ctx, "tri normal", *R.case_trailing(rng, 320, 320, 32, -1.0, 1, kind="normal", tri=1))
    run_rounded(gpu_ctx, "corner normal", *R.case_corner(rng, 192, 0, kind="normal"))
    run_rounded(gpu_ctx, "prediction normal", *R.case_predict(rng, 17, 192, kind="normal"))
    run_rounded(gpu_ctx, "split-K normal", *R.case_predict(rng, 17, 192, ksplit=2, kind="normal"), cfgs=(2,))


# ------------------------------------------------------------------ refused launches
def test_refused_arguments(gpu_ctx):
    """everything launch_gemm refuses or takes on trust, and every launch that could address an element outside the arena,
    comes back as GPEMU_ERR_ARG before anything runs"""
    arena, args = R.case_batch(np.random.default_rng(5), 64, 64, 32, 2, 0)
    gpu_ctx.test_gemm_launch(arena, **args)                        # the base launch itself is fine
    m, n, ldc, lda, ldb = args["m"], args["n"], args["ldc"], args["lda"], args["ldb"]
    refused = {
        "k0 no multiple of 16": dict(k0=8),
        "k1 no multiple of 16": dict(k1=24),
        "k1 = k0": dict(k0=32),
        "k1 < k0": dict(k0=32, k1=16),
        "beta = 2": dict(beta=2),
        "beta = 1 with alpha = 0.5": dict(alpha=0.5),
        "split-K with beta": dict(ksplit=2, nbatch=0),
        "split-K with a batch": dict(ksplit=2, beta=0, alpha=1.0),
        "force_cfg = 4": dict(force_cfg=4),
        "m = 0": dict(m=0),
        "C ends one element behind the arena": dict(offC=arena.size - args["bsC"] - (m - 1) * ldc - n + 1),
        "C starts before the arena": dict(offC=-1),
        "A starts before the arena": dict(offA=-8),
        "a row of A too many": dict(offA=arena.size - args["bsA"] - (m - 1) * lda - args["k1"] + 1),
        "B: n reaches behind the arena": dict(n=(arena.size - args["offB"]) // ldb + 64),
        "the last matrix of the batch lies outside": dict(bsC=arena.size),
        "a negative stride leaves the arena at the front": dict(bsB=-(args["offB"] + 1)),
        "k1 beyond the arena": dict(k1=1 << 19),
        "factor-ahead on 128x128 tiles": dict(fa=1, tri=1, force_cfg=8),
        "factor-ahead without tri": dict(fa=1, force_cfg=2),
        "factor-ahead with alpha = 1": dict(fa=1, tri=1, force_cfg=2, alpha=1.0, beta=0),
    }
    for why, change in refused.items():
        with pytest.raises(abi.GpemuError) as e:
            gpu_ctx.test_gemm_launch(arena, **dict(args, **change))
        assert e.value.code == abi.ERR_ARG, why
    # the last element of the arena may be C's last element
    ok = dict(args, offC=arena.size - args["bsC"] - (m - 1) * ldc - n, alpha=1.0, beta=0)
    got, _ = gpu_ctx.test_gemm_launch(arena, **ok)
    want, mask = R.expected(arena, ok)
    assert R.mismatches(got, want, arena, mask, ok)[0] == 0
