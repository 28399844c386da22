"""Right-hand-side rows riding in the diagonal tiles of a big-tile trailing update (GPEMU_RHS_RIDE, gemm_nt_kernel RIDE):
one trailing_update() at a time through gpemu_test_update_launch, ride = 1 against ride = 0.

The contract is bits.  A rider feeds the matrix unit, per accumulator, the chain the 64x64 launch it replaces fed it, so
the whole arena -- matrix rows, right-hand-side rows, guard bands, the gaps between the matrices of a batch -- must come
back the same with the switch on and off, and the rows rhs_live .. 63 of the right-hand-side block, which a rider does not
touch and the old launch rewrites as 0 - 0 b, must keep the bits they were uploaded with in both runs.  The ridden rows
are also checked against tests/gemmref.py (integer operands: the numpy product is the only correct answer, no tolerance).

Who ran is observed, not assumed: _rode() uploads non-zero rows 16 .. 63 under rhs_live <= 16 -- outside the contract of
the entry, on purpose -- which a rider leaves alone and the old launch updates.  Every case that should ride and every
fallback is pinned this way.

The contexts are created under GPEMU_GEMM_BIG_TILES=1 (the suite's setting for 128x128 tiles at test sizes)."""
import os

import numpy as np
import pytest

import gemmref as R
from madaiemulator_amd import abi, synth

pytestmark = pytest.mark.gpu

RP = 64
BIG = {"GPEMU_GEMM_BIG_TILES": "1"}


def _ctx_with_env(env, device=0):
    """a context whose schedule switches come from `env` (copied into the context when it is created)"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return abi.Context(device)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def big_ctx():
    c = _ctx_with_env(BIG)
    yield c
    c.close()


def make_case(seed, c0, k, c_rows, ncols, rhs_live, nbatch=0, kind="mixed", dead=0.0, inv=0):
    """the tall matrices of one update in an arena: ld = c0 + k + c_rows matrix rows, RP right-hand-side rows under them and,
    with inv, the c0 + k identity rows the update takes under those (operand values: in production they hold fill-in).
    Operands fill the update's footprint (panel columns c0 .. c0+k-1 and C columns c0+k .. c0+k+ncols-1 of the rows from
    c0+k on); rows rhs_live .. RP-1 of the right-hand-side block hold `dead` there (+0: the contract); everything else is
    gemmref's background.  kind "int": integers in [-8, 8]; "mixed": standard normal with every third column negative
    and every fifth row scaled by 1e-150 (tiny, and tiny x tiny underflows).  The stride of a batch is no multiple of
    the matrix size.  -> (arena, args)"""
    rng = np.random.default_rng(seed)
    ld = c0 + k + c_rows
    r0 = c0 + k
    rows = ld + RP + (r0 if inv else 0)
    nb = max(nbatch, 1)
    stride = R.round_up(rows * ld, 8) + 72
    off = R.GUARD
    arena = R.background(off + nb * stride + R.GUARD)

    def values(m, n):
        if kind == "int":
            return R.operand(rng, m, n, "int")
        v = rng.standard_normal((m, n))
        v[:, ::3] = -np.abs(v[:, ::3])
        v[::5, :] *= 1e-150
        return v

    for b in range(nb):
        fp = R.mat(arena, off + b * stride + r0 * ld + c0, ld, rows - r0, k + ncols)
        fp[:] = values(rows - r0, k + ncols)
        fp[c_rows + rhs_live:c_rows + RP, :] = dead
    args = dict(off=off, ld=ld, stride=stride if nbatch else 0, c0=c0, k=k, ncols=ncols, rp=RP, inv=inv, rhs_live=rhs_live, nbatch=nbatch)
    return arena, args


def rhs_rows(arena, args, b=0, lo=0, hi=RP):
    """rows lo .. hi-1 of the right-hand-side block of matrix b, all ld columns"""
    ld = args["ld"]
    stride = args["stride"] if args["nbatch"] else 0
    return R.mat(arena, args["off"] + b * stride + (ld + lo) * ld, ld, hi - lo, ld)


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


def run_pair(ctx, what, arena, args, rides):
    """ride = 1 and ride = 0 on the same arena: the same bits everywhere; where the update rides, rows rhs_live .. RP-1 keep
    their bits in both runs.  -> the arena after the update"""
    on, _ = ctx.test_update_launch(arena, **dict(args, ride=1))
    off, _ = ctx.test_update_launch(arena, **dict(args, ride=0))
    diff = np.flatnonzero(on.view(np.int64) != off.view(np.int64))
    if diff.size:
        e = int(diff[0])
        rel = (e - args["off"]) % max(args["stride"], 1) if args["nbatch"] else e - args["off"]
        print(f"{what}: {diff.size} elements differ, the first at arena[{e}] = row {rel // args['ld']}, column {rel % args['ld']}: "
              f"ride {float(on[e])!r}, no ride {float(off[e])!r}, before {float(arena[e])!r}")
    assert diff.size == 0, (what, diff.size)
    if rides:
        for b in range(max(args["nbatch"], 1)):
            for out in (on, off):
                assert same_bits(rhs_rows(out, args, b, args["rhs_live"]), rhs_rows(arena, args, b, args["rhs_live"])), (what, b)
    return on


def _rode(ctx, c0, k, c_rows, ncols, rhs_live, nbatch=0, inv=0):
    """did the riders run?  Rows 16 .. RP-1 hold ones under rhs_live <= 16 (outside the entry's contract, to tell the two
    apart): a rider leaves them alone, the launch of their own updates them."""
    arena, args = make_case(7, c0, k, c_rows, ncols, min(rhs_live, 16), nbatch, kind="int", dead=1.0, inv=inv)
    args["rhs_live"] = rhs_live
    out, _ = ctx.test_update_launch(arena, **dict(args, ride=1))
    return same_bits(rhs_rows(out, args, 0, 16), rhs_rows(arena, args, 0, 16))


# ------------------------------------------------------------------ smallest shapes
@pytest.mark.parametrize("rhs_live", [1, 10, 16])
@pytest.mark.parametrize("K", [16, 32, 48])
def test_one_diagonal_tile(big_ctx, K, rhs_live):
    """c_rows = ncols = 128: one diagonal tile, nothing else.  K = 16: one chunk (the prologue's loads only), 32: the
    hand-over from the x to the y fragments and one prefetch, 48: an odd chunk count.  Negative and tiny operands."""
    arena, args = make_case(K + rhs_live, 0, K, 128, 128, rhs_live)
    assert _rode(big_ctx, 0, K, 128, 128, rhs_live)
    run_pair(big_ctx, f"one tile K {K} live {rhs_live}", arena, args, rides=True)


def test_trapezoid(big_ctx):
    """c_rows = 384, ncols = 256, K = 64, c0 = 192: two diagonal tiles with rectangular tiles beside and below them"""
    arena, args = make_case(3, 192, 64, 384, 256, 10)
    assert _rode(big_ctx, 192, 64, 384, 256, 10)
    run_pair(big_ctx, "trapezoid", arena, args, rides=True)


def test_batch_of_three(big_ctx):
    """nbatch = 3, the stride no multiple of the matrix size: every matrix under its own right-hand-side rows"""
    arena, args = make_case(4, 64, 32, 256, 256, 10, nbatch=3)
    assert args["stride"] % ((args["ld"] + RP) * args["ld"]) != 0
    assert _rode(big_ctx, 64, 32, 256, 256, 10, nbatch=3)
    run_pair(big_ctx, "batch of 3", arena, args, rides=True)


@pytest.mark.parametrize("nbatch", [0, 3])
def test_with_identity_rows(big_ctx, nbatch):
    """inv = 1: the identity rows under the right-hand-side rows keep their launch (launch c), the right-hand-side rows' own
    launch between the two is dropped -- alone and in a lock-step batch of 3, the shape of a value+gradient batch.  The
    identity rows must change (they are operands here, not zeros) and change alike with the switch on and off."""
    arena, args = make_case(6 + nbatch, 64, 32, 256, 256, 10, nbatch=nbatch, inv=1)
    assert _rode(big_ctx, 64, 32, 256, 256, 10, nbatch=nbatch, inv=1)
    out = run_pair(big_ctx, f"identity rows, batch {nbatch}", arena, args, rides=True)
    ld, r0 = args["ld"], args["c0"] + args["k"]
    for b in range(max(nbatch, 1)):
        off = args["off"] + b * args["stride"] + (ld + RP) * ld + r0
        before, after = R.mat(arena, off, ld, r0, 256), R.mat(out, off, ld, r0, 256)
        assert np.all(np.any(before != after, axis=1)), b


def test_tile_table_order(big_ctx):
    """one matrix, c_rows = ncols = 4096, K = 16: 528 >= 512 tiles, so under the default GPEMU_GEMM_TABLE (8, relied on
    here: big_ctx sets GPEMU_GEMM_BIG_TILES alone) the XCD-blocked table decides which workgroup gets a diagonal tile.
    That the order differs is not observable through the entry; what is: a context under GPEMU_GEMM_TABLE=0 (the closed-form
    order of the smaller cases) gives the same arena, and both ride."""
    arena, args = make_case(5, 0, 16, 4096, 4096, 10)
    assert 32 * 33 // 2 == 528 and "GPEMU_GEMM_TABLE" not in os.environ
    assert _rode(big_ctx, 0, 16, 4096, 4096, 10)
    out = run_pair(big_ctx, "tile table", arena, args, rides=True)
    c = _ctx_with_env(dict(BIG, GPEMU_GEMM_TABLE="0"))
    try:
        assert _rode(c, 0, 16, 4096, 4096, 10)
        plain, _ = c.test_update_launch(arena, **dict(args, ride=1))
    finally:
        c.close()
    assert same_bits(out, plain)
    # the ridden rows changed at all: every column of the update was reached by a diagonal tile (every fifth panel row is
    # tiny, make_case: its column moves by less than half an ulp)
    r0 = args["c0"] + args["k"]
    before, after = rhs_rows(arena, args, 0, 0, 10)[:, r0:], rhs_rows(out, args, 0, 0, 10)[:, r0:]
    changed = np.any(before != after, axis=0)
    assert np.all(changed[np.arange(4096) % 5 != 0])


# ------------------------------------------------------------------ fallbacks
def test_fallbacks_run_the_old_launches(big_ctx):
    """rhs_live = 17, ncols = 192 and a context without idle waves: ride = 1 runs the launch of their own for the
    right-hand-side rows (seen by _rode), and gives the bits of ride = 0"""
    assert not _rode(big_ctx, 0, 32, 256, 256, 17)
    arena, args = make_case(17, 0, 32, 256, 256, 17)
    run_pair(big_ctx, "rhs_live 17", arena, args, rides=False)
    assert not _rode(big_ctx, 0, 32, 256, 192, 10)
    arena, args = make_case(18, 0, 32, 256, 192, 10)
    run_pair(big_ctx, "ncols 192", arena, args, rides=False)
    assert not _rode(big_ctx, 0, 32, 256, 256, 0)
    c = _ctx_with_env(dict(BIG, GPEMU_IDLE_WAVES="0"))
    try:
        assert not _rode(c, 0, 32, 256, 256, 10)
        arena, args = make_case(19, 0, 32, 256, 256, 10)
        busy = run_pair(c, "idle waves off", arena, args, rides=False)
    finally:
        c.close()
    # and the context with idle waves, riding, gives the lower triangle and the right-hand-side rows of that run
    out = run_pair(big_ctx, "idle waves on", arena, args, rides=True)
    ld, r0 = args["ld"], args["c0"] + args["k"]
    a = R.mat(out, args["off"] + r0 * ld + r0, ld, 256, 256)
    b = R.mat(busy, args["off"] + r0 * ld + r0, ld, 256, 256)
    assert same_bits(np.tril(a), np.tril(b)) and same_bits(rhs_rows(out, args), rhs_rows(busy, args))


def test_context_switch_off(big_ctx):
    """GPEMU_RHS_RIDE=0 at context creation is the default the entry restores; ride = 1 of the call still rides"""
    c = _ctx_with_env(dict(BIG, GPEMU_RHS_RIDE="0"))
    try:
        assert _rode(c, 0, 32, 256, 256, 10)
        arena, args = make_case(20, 0, 32, 256, 256, 10)
        assert same_bits(run_pair(c, "context switch off", arena, args, rides=True), run_pair(big_ctx, "on", arena, args, rides=True))
    finally:
        c.close()


# ------------------------------------------------------------------ exact reference
@pytest.mark.parametrize("c0,K,c_rows,ncols,rhs_live,nbatch,inv", [(0, 48, 128, 128, 16, 0, 0), (192, 64, 384, 256, 10, 0, 0),
                                                                     (64, 32, 256, 256, 10, 3, 0), (64, 32, 256, 256, 10, 3, 1)])
def test_ridden_rows_against_the_exact_reference(big_ctx, c0, K, c_rows, ncols, rhs_live, nbatch, inv):
    """integer operands: the matrix rows as the triangular update of test_gpu_gemm_modes.py, the right-hand-side rows as the
    dense update C_r - R P^T (with inv the identity rows under them likewise), all from gemmref.expected on the uploaded
    arena (the panel is only read); every other element of the arena keeps its bits"""
    arena, args = make_case(c0 + K, c0, K, c_rows, ncols, rhs_live, nbatch, kind="int", inv=inv)
    ld, r0, off = args["ld"], c0 + K, args["off"]
    common = dict(ldc=ld, lda=ld, ldb=ld, n=ncols, k0=0, k1=K, alpha=-1.0, beta=1, nbatch=nbatch, bsC=args["stride"], bsA=args["stride"],
                  bsB=args["stride"], offB=off + r0 * ld + c0)
    tri = dict(common, offC=off + r0 * ld + r0, offA=off + r0 * ld + c0, m=c_rows, tri=1)
    rhs = dict(common, offC=off + ld * ld + r0, offA=off + ld * ld + c0, m=RP, tri=0)
    want, mask = R.expected(arena, tri)
    want_r, mask_r = R.expected(arena, rhs)
    want[mask_r == R.MUST] = want_r[mask_r == R.MUST]
    mask = np.maximum(mask, mask_r)
    if inv:
        ident = dict(common, offC=off + (ld + RP) * ld + r0, offA=off + (ld + RP) * ld + c0, m=r0, tri=0)
        want_i, mask_i = R.expected(arena, ident)
        want[mask_i == R.MUST] = want_i[mask_i == R.MUST]
        mask = np.maximum(mask, mask_i)
    assert _rode(big_ctx, c0, K, c_rows, ncols, rhs_live, nbatch, inv)
    got, _ = big_ctx.test_update_launch(arena, **dict(args, ride=1))
    count, lines = R.mismatches(got, want, arena, mask, rhs)
    if count:
        print(f"{count} elements wrong (positions relative to the right-hand-side block), the first:")
        print("\n".join(lines))
    assert count == 0, (count, lines[:2])


# ------------------------------------------------------------------ refused calls
def test_refused_arguments(big_ctx):
    """argument errors come back as GPEMU_ERR_ARG before anything runs"""
    arena, args = make_case(1, 64, 32, 128, 128, 10, nbatch=2)
    big_ctx.test_update_launch(arena, **args)
    refused = {
        "k no multiple of 16": dict(k=24),
        "k = 0": dict(k=0),
        "c0 < 0": dict(c0=-2),
        "odd c0": dict(c0=63),
        "odd ld": dict(ld=args["ld"] + 1),
        "odd stride": dict(stride=args["stride"] + 1),
        "odd offset": dict(off=args["off"] + 1),
        "ncols = 0": dict(ncols=0),
        "columns beyond ld": dict(ncols=136),
        "rhs_live > rp": dict(rhs_live=RP + 1),
        "rhs_live < 0": dict(rhs_live=-1),
        "ride = 2": dict(ride=2),
        "inv = 2": dict(inv=2),
        "the matrices overlap": dict(stride=args["ld"] * 8),
        "the last matrix leaves the arena": dict(off=args["off"] + 2 * R.GUARD),
        "the identity rows leave the arena": dict(inv=1),
        "a negative offset": dict(off=-2),
    }
    for why, change in refused.items():
        with pytest.raises(abi.GpemuError) as e:
            big_ctx.test_update_launch(arena, **dict(args, **change))
        assert e.value.code == abi.ERR_ARG, why
    assert big_ctx.L.gpemu_test_update_launch(None, None, 0, None, None) == abi.ERR_ARG


# ------------------------------------------------------------------ whole path
def _whole_path(env):
    N, d = 1500, 4
    X, y = synth.design(N, d, 8)
    th = synth.default_thetas(1, d)
    ths = np.array([synth.perturbed_thetas(1, d, 3, i) for i in range(3)])
    c = _ctx_with_env(env)
    try:
        c.set_model(1, 1, X, y)
        lb = c.loglik_batch(ths)
        lg = c.loglik_grad(th)
        gb = c.loglik_grad_batch(ths)
        c.predict_setup(th)
        pm, pv = c.predict(synth.design(64, d, 99)[0])
    finally:
        c.close()
    out = {"pm": pm, "pv": pv}
    out.update({"batch_" + k_: np.asarray(v) for k_, v in lb.items()})
    out.update({"grad_" + k_: np.asarray(v) for k_, v in lg.items()})
    out.update({"gradbatch_" + k_: np.asarray(v) for k_, v in gb.items()})
    return out


@pytest.mark.parametrize("env", [{}, BIG], ids=["default", "big-tiles"])
def test_whole_path_keeps_every_bit(env):
    """N = 1500, d = 4, order 1: a likelihood batch of 3, a value+gradient evaluation, a value+gradient batch of 3 (lock-step
    matrices with inverse rows) and 64 predictions under
    GPEMU_RHS_RIDE=0 and under the default, with the automatic tile choice and with 128x128 tiles everywhere (where the
    updates of this size do ride): every output equal"""
    on, off = _whole_path(env), _whole_path(dict(env, GPEMU_RHS_RIDE="0"))
    assert set(on) == set(off) and "gradbatch_grad" in on and on["gradbatch_grad"].shape == (3, 5)
    for name in on:
        assert np.array_equal(on[name], off[name]), name
