"""panel_rows_kernel: the rows under a finished 256-column group in one pass (GPEMU_LEAF_PANEL_ROWS of
gpemu_test_leaf_launch, GPEMU_PANEL_ROWS in the schedule).  The contract is bits: every element leaves as the group's
five launches -- pair, solve with the deferred rows, K = 128 update with its factor-ahead tile, pair, solve -- leave it.

  one launch     the five launches over ALL rows on one copy of an arena, the same five cut at r_far followed by the new
                 launch on another: the two arenas are equal, every element, NaN where NaN was (everything outside the
                 operands is NaN, as in test_gpu_leaf_kernels.py: what a kernel reads beside them shows in its output).
                 Directly under the square (r_far = cg + 256) the cut leaves the last solve no rows of its own; its extra
                 workgroup's job -- the 64 rows under the block at cg + 128 -- is then the plain solve of those rows (the
                 schedule never cuts there: it keeps at least 64 rows for that launch).
  one element    the far rows of a well-conditioned case against longdouble, step by step from the device's own X with the
                 constants of tests/leafref.py: a block that is updated and solved without reaching memory in between has
                 the update's bar carried through the inverse of the step (as leafref does for the factor-ahead tile);
                 K = 64 m fused accumulations count m C_UPDATE.
  factorisations GPEMU_PANEL_ROWS=2 against 0 in fresh contexts: every element of L, a likelihood batch and its elements
                 alone, the index of a failed pivot, a value+gradient batch (which keeps the launches it had)."""
import numpy as np
import pytest

import leafref as R
from madaiemulator_amd import abi, synth

pytestmark = pytest.mark.gpu

PANEL_ROWS = abi.LEAF_PANEL_ROWS
G = 4 * R.LEAF                                   # columns of a group


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def group_problem(cg, ld, n_below, nbatch, seed):
    """arena of NaN with, per matrix, the lower triangle of the square at (cg, cg) and the n_below rows under it, columns
    cg .. cg+255, from a seeded positive definite matrix (matrix b: times 4^b) -> arena, lay, rows, K"""
    n = G + n_below
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((n, 96))
    K = F @ F.T + 96.0 * np.eye(n)
    rows = cg + n
    arena, lay = R.layout(ld, rows, nbatch)
    i, j = np.indices((G, G))
    for b in range(max(nbatch, 1)):
        M = R.matrix(arena, lay, rows, b)
        Kb = K * 4.0 ** b
        M[cg:cg + G, cg:cg + G][i >= j] = Kb[:G, :G][i >= j]
        M[cg + G:cg + n, cg:cg + G] = Kb[G:, :G]
    return arena, lay, rows, K


def five_launches(ctx, arena, lay, cg, row_end):
    """the launches of a 256-column group on the rows cg .. row_end-1, as potrf_rec issues them"""
    ld, nb = lay["ld"], lay["nbatch"]

    def leaf(a, **args):
        out, info = ctx.test_leaf_launch(a, **lay, **args)
        assert not info.any(), (args, info)
        return out
    a = leaf(arena, op=R.FACTOR, c0=cg)
    a = leaf(a, op=R.PAIR, c0=cg, m_below=row_end - (cg + 64), fa=1)
    a = leaf(a, op=R.SOLVE, c0=cg + 64, m_below=row_end - (cg + 128), c0b=cg)
    o = lay["off"] + (cg + 128) * ld
    a, info = ctx.test_gemm_launch(a, offC=o + cg + 128, offA=o + cg, offB=o + cg, ldc=ld, lda=ld, ldb=ld, bsC=lay["bstride"],
                                   bsA=lay["bstride"], bsB=lay["bstride"], alpha=-1.0, beta=1, m=row_end - (cg + 128), n=128,
                                   k0=0, k1=128, tri=1, nbatch=nb, fa=1, fa_c0=cg + 128)
    assert not info.any(), info
    a = leaf(a, op=R.PAIR, c0=cg + 128, m_below=row_end - (cg + 192), fa=1)
    if row_end > cg + G:
        return leaf(a, op=R.SOLVE, c0=cg + 192, m_below=row_end - (cg + G), c0b=cg + 128)
    return leaf(a, op=R.SOLVE, c0=cg + 128, m_below=64)          # (the extra workgroup's rows alone, see the docstring)


def both_ways(ctx, cg, ld, r_off, m_far, nbatch, seed):
    arena, lay, rows, K = group_problem(cg, ld, r_off + m_far, nbatch, seed)
    r_far = cg + G + r_off
    whole = five_launches(ctx, arena, lay, cg, rows)
    cut = five_launches(ctx, arena, lay, cg, r_far)
    got, info = ctx.test_leaf_launch(cut, **lay, op=PANEL_ROWS, c0=cg, r_far=r_far, m_far=m_far)
    assert not info.any()
    return arena, lay, rows, cut, whole, got


@pytest.mark.parametrize("nbatch", [1, 3])
@pytest.mark.parametrize("m_far", [64, 192, 640])
@pytest.mark.parametrize("cg", [0, 256])
def test_one_launch_bit_for_bit(gpu_ctx, cg, m_far, nbatch):
    for extra in (0, 2, 62):
        for r_off in (0, 128):
            what = (cg, m_far, nbatch, extra, r_off)
            arena, lay, rows, cut, whole, got = both_ways(gpu_ctx, cg, cg + G + extra, r_off, m_far, nbatch, 7 * m_far + extra + r_off + cg)
            assert np.array_equal(got, whole, equal_nan=True), what
            same = bits(got) == bits(whole)
            assert np.all(same | np.isnan(whole)), (what, "differs in a sign of zero", np.flatnonzero(~same)[:8].tolist())
            # the new launch wrote its rows, all of them, and nothing else
            r_far = cg + G + r_off
            touched = np.zeros(arena.size, dtype=bool)
            for b in range(nbatch):
                T = R.matrix(touched, lay, rows, b)
                T[r_far:r_far + m_far, cg:cg + G] = True
                assert np.all(np.isfinite(R.matrix(got, lay, rows, b)[r_far:r_far + m_far, cg:cg + G])), what
            assert np.array_equal(bits(got)[~touched], bits(cut)[~touched]), what


def test_refusals(gpu_ctx):
    cg, ld, m_far, nbatch = 256, 256 + G + 2, 64, 3
    arena, lay, rows, _ = group_problem(cg, ld, m_far, nbatch, 5)
    ok = dict(lay, op=PANEL_ROWS, c0=cg, r_far=cg + G, m_far=m_far)
    need = lay["off"] + (nbatch - 1) * lay["bstride"] + (rows - 1) * ld + cg + G - 1 + 1
    sq = five_launches(gpu_ctx, arena, lay, cg, rows)
    gpu_ctx.test_leaf_launch(sq[:need], **ok)                    # the shortest arena that holds the launch
    refused = [("m_far = 0", sq, dict(m_far=0)), ("m_far = 65", sq, dict(m_far=65)), ("m_far = -64", sq, dict(m_far=-64)),
               ("one element past the arena", sq[:need - 1], {}), ("rows inside the square", sq, dict(r_far=cg + G - 64)),
               ("odd c0", sq, dict(c0=cg + 1, r_far=cg + G + 2)), ("odd ld", sq, dict(ld=ld - 1)), ("odd off", sq, dict(off=lay["off"] + 1)),
               ("odd bstride", sq, dict(bstride=lay["bstride"] + 1)), ("m_below with the panel rows", sq, dict(m_below=64)),
               ("c0b with the panel rows", sq, dict(c0b=0)), ("fa with the panel rows", sq, dict(fa=1)),
               ("columns leave the row", sq, dict(c0=cg + 4, r_far=cg + G + 4)),
               ("r_far with another op", sq, dict(op=R.FACTOR, r_far=cg + G, m_far=0)),
               ("m_far with another op", sq, dict(op=R.FACTOR, r_far=0, m_far=64))]
    for why, a, change in refused:
        with pytest.raises(abi.GpemuError) as e:
            gpu_ctx.test_leaf_launch(a, **dict(ok, **change))
        assert e.value.code == abi.ERR_ARG, why


# ------------------------------------------------------------------ one element against extended precision
def check_block(Ljj, Bj, bar_in, X):
    """leafref.check_solve for rows whose right-hand side Bj (longdouble, from the device's own earlier X) carries the error
    bar bar_in of an update that never reached memory: the step's inverse carries it into X"""
    L = np.tril(np.asarray(Ljj, dtype=R.LD))
    X = np.asarray(X, dtype=R.LD)
    worst = 0.0
    for j in range(4):
        s = slice(16 * j, 16 * j + 16)
        inv, bound = R.tri_inverse_exact(L[s, s]), R.series_bound(L[s, s])
        acc, aabs = Bj[:, s].copy(), np.abs(Bj[:, s])
        for i in range(j):
            t = slice(16 * i, 16 * i + 16)
            acc -= X[:, t] @ L[s, t].T
            aabs += np.abs(X[:, t]) @ np.abs(L[s, t]).T
        bar = R.C_SOLVE * R.U * (aabs @ np.abs(inv).T) + R.C_INV * R.U * (aabs @ bound.T) + bar_in[:, s] @ np.abs(inv).T
        worst = max(worst, R.ratio(np.abs(X[:, s] - acc @ inv.T), bar))
    return worst


def test_far_rows_against_longdouble(gpu_ctx):
    cg, m_far = 256, 192
    arena, lay, rows, cut, whole, got = both_ways(gpu_ctx, cg, cg + G + 2, 128, m_far, 0, 11)
    r_far = cg + G + 128
    Sq = np.asarray(R.matrix(cut, lay, rows)[cg:cg + G, cg:cg + G], dtype=R.LD)       # the finished square the launch read
    B = np.asarray(R.matrix(cut, lay, rows)[r_far:r_far + m_far, cg:cg + G], dtype=R.LD)
    X = np.asarray(R.matrix(got, lay, rows)[r_far:r_far + m_far, cg:cg + G], dtype=R.LD)
    blk = lambda M, a, b=None: M[:, 64 * a:64 * a + 64] if b is None else M[64 * a:64 * a + 64, 64 * b:64 * b + 64]
    assert R.check_solve(blk(Sq, 0, 0), blk(B, 0), blk(X, 0)) < 1
    for a in (1, 2, 3):
        Ba, mag = blk(B, a).copy(), np.abs(blk(B, a))
        for b in range(a):
            Ba -= blk(X, b) @ blk(Sq, a, b).T
            mag += np.abs(blk(X, b)) @ np.abs(blk(Sq, a, b)).T
        worst = check_block(blk(Sq, a, a), Ba, a * R.C_UPDATE * R.U * mag, blk(X, a))
        print(f"far rows, block {a}: error/bar {worst:.3f}")
        assert worst < 1, (a, worst)
    # and the finished product: X L^T gives the rows back
    L = np.tril(Sq)
    for a in range(4):                         # (the parked inverses sit above the diagonals of the diagonal blocks)
        L[64 * a:64 * a + 64, 64 * a:64 * a + 64] = np.tril(blk(Sq, a, a))
    err = np.abs(X @ L.T - B).max() / np.abs(B).max()
    assert err < 1e-13, err


# ------------------------------------------------------------------ whole factorisations
# (the default cut, 64 rows under the group, passes the rows under every group that has 128 rows below it; with the cut at
# the end of the outer panel's square, GPEMU_PANEL_SPLIT=0, a panel of 512 columns passes the rows under its first group)
ENVS = [{"GPEMU_NB_TOP": "256"}, {"GPEMU_NB_TOP": "512"}, {"GPEMU_NB_TOP": "512", "GPEMU_PANEL_SPLIT": "0"},
        {"GPEMU_NB_TOP": "256", "GPEMU_PANEL_SPLIT": "2"}, {"GPEMU_PANEL_SPLIT": "0"}]


def fresh(monkeypatch, env, panel_rows):
    for k in ("GPEMU_NB_TOP", "GPEMU_PANEL_SPLIT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("GPEMU_PANEL_ROWS", str(panel_rows))      # copied into the context when it is created
    return abi.Context(0)


@pytest.mark.parametrize("env", ENVS)
def test_factor_every_element(monkeypatch, env):
    outs = []
    for pr in (0, 2):
        c = fresh(monkeypatch, env, pr)
        res = []
        for n in (576, 1100, 1536):
            rng = np.random.default_rng(n)
            M = rng.standard_normal((n, n))
            L, info = c.test_potrf(M @ M.T + n * np.eye(n))
            assert info == 0
            res.append(L)
        S = np.eye(700)                        # a failed pivot inside a group, and a later one: the first is reported
        S[57, 57] = -1.0
        S[450, 450] = -2.0
        res.append(c.test_potrf(S)[1])
        c.close()
        outs.append(res)
    for a, b in zip(outs[0][:3], outs[1][:3]):
        assert np.array_equal(bits(a), bits(b))
    assert outs[0][3] == outs[1][3] == 58


@pytest.mark.parametrize("env", ENVS)
def test_likelihood_and_gradient_batches(monkeypatch, env):
    N, d = 1500, 4
    X, y = synth.design(N, d, 8)
    ths = np.array([synth.perturbed_thetas(1, d, 3, i) for i in range(3)])
    keys = ("value", "sigma2", "beta", "logdet", "info")
    outs = []
    for pr in (0, 2):
        c = fresh(monkeypatch, env, pr)
        c.set_model(1, 1, X, y)
        first, batch, alone, grad = c.loglik_batch(ths), c.loglik_batch(ths), c.loglik(ths[1]), c.loglik_grad_batch(ths)
        c.close()
        assert np.all(batch["status"] == 0) and alone["status"] == 0 and np.all(grad["status"] == 0)
        for k in keys:                         # plain launches and the recorded graph; the batch and its element alone
            assert np.array_equal(bits(first[k]), bits(batch[k])), k
            assert np.array_equal(bits(np.asarray(batch[k])[1]), bits(alone[k])), k
        outs.append((batch, grad))
    for k in keys:
        assert np.array_equal(bits(outs[0][0][k]), bits(outs[1][0][k])), k
    for k in ("value", "sigma2", "beta", "grad", "info"):
        assert np.array_equal(bits(outs[0][1][k]), bits(outs[1][1][k])), k
