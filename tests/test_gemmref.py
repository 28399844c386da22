"""Self-tests of tests/gemmref.py, the CPU reference of the GEMM launch-mode tests (no GPU needed)."""
import numpy as np
import pytest

import gemmref as R

K_MAX = 4096     # the largest contraction length the exact method is stated for (test_gpu_gemm_modes.py uses up to 2048)


def test_integer_operands_are_integers_in_range():
    A = R.operand(np.random.default_rng(1), 300, 200, "int")
    assert A.dtype == np.float64 and np.array_equal(A, np.rint(A))
    assert A.min() == -8 and A.max() == 8


def test_zero_patterns():
    rng = np.random.default_rng(2)
    A = R.kstart_operand(rng, 192 + 64, 192, 64)
    for i in range(A.shape[0]):
        assert not np.any(A[i, :max(0, i - 64)])
    assert np.all(np.count_nonzero(A[:64], axis=1) > 150)                   # the first kstart_off rows are dense
    assert all(np.count_nonzero(A[i, max(0, i - 64):]) > 0.8 * (192 - max(0, i - 64)) for i in range(64, 250))
    B = R.kend_operand(rng, 192 + 64, 192, 0, 192)
    for j in range(192):
        assert not np.any(B[j, j + 1:])
        assert np.count_nonzero(B[j, :j + 1]) > 0.7 * (j + 1) - 3
    assert np.all(np.count_nonzero(B[192:], axis=1) > 150)                  # the augmented rows are dense
    # the patterns are exact zeros also for normal operands, and the same where an offset shifts them
    B = R.kend_operand(rng, 96, 64, 16, 64, "normal")
    j, k = np.indices(B.shape)
    assert not np.any(B[(k > j - 16) & (j < 64)]) and np.all(B[(k <= j - 16) | (j >= 64)] != 0.0)


def test_zero_patterns_make_the_skipped_product_the_full_product():
    """what expected() relies on: element (i, j) contracted over element_bounds alone equals the full product"""
    rng = np.random.default_rng(3)
    arena, args = R.case_corner(rng, 192, 0)
    want, _ = R.expected(arena, args)
    A = R.mat(arena, args["offA"], args["lda"], args["m"], 192)
    Cw = R.mat(want, args["offC"], args["ldc"], args["m"], args["n"])
    for i, j in [(0, 0), (63, 5), (64, 64), (100, 3), (200, 130), (255, 255), (255, 0)]:
        lo, hi = R.element_bounds(args, i, j)
        assert lo == max(0, i - 64) and hi == 192
        assert Cw[i, j] == A[i, lo:hi] @ A[j, lo:hi]
    arena, args = R.case_predict(rng, 17, 192, ksplit=3)
    want, _ = R.expected(arena, args)
    A = R.mat(arena, args["offA"], args["lda"], 17, 192)
    B = R.mat(arena, args["offB"], args["ldb"], 256, 192)
    for s in range(3):
        Cw = R.mat(want, args["offC"] + s * args["bsC"], args["ldc"], 17, 256)
        for i, j in [(0, 0), (16, 63), (3, 64), (5, 100), (9, 191), (2, 192), (16, 255)]:
            lo, hi = R.element_bounds(args, i, j, s)
            assert hi == lo or hi <= (192 if j >= 192 else j + 1)       # (empty: the slice lies behind column j)
            assert Cw[i, j] == A[i, lo:hi] @ B[j, lo:hi]


def test_exactness_precondition_at_the_largest_k():
    rng = np.random.default_rng(4)
    A, B, C0 = R.operand(rng, 8, K_MAX, "int"), R.operand(rng, 8, K_MAX, "int"), R.operand(rng, 8, 8, "int")
    bound = R.assert_exact(A, B, C0, -1.0)
    assert bound == K_MAX * 64 + 8 and bound < 2 ** 53
    # ... and with the factor-ahead block's quantum on top
    assert R.assert_exact(A, B, C0 * R.FA_QUANTUM + 4096.0, -1.0, R.FA_QUANTUM) / R.FA_QUANTUM < 2 ** 53
    # every order of summation gives the same bits
    want = A @ B.T
    assert np.array_equal(want, (A[:, ::-1].copy() @ B[:, ::-1].copy().T))
    assert np.array_equal(want, np.einsum("ik,jk->ij", A.astype(np.int64), B.astype(np.int64)).astype(np.float64))
    with pytest.raises(AssertionError):
        R.assert_exact(A + 0.5, B)
    with pytest.raises(AssertionError):
        R.assert_exact(A * 2.0 ** 40, B * 2.0 ** 10)


@pytest.mark.parametrize("k0,k1,ksplit", [(0, 1024, 2), (0, 1024, 3), (0, 1024, 8), (0, 1040, 2), (0, 1040, 3), (0, 1040, 8),
                                           (32, 192, 2), (0, 16, 3), (64, 4096, 7)])
def test_slices_tile_the_k_range(k0, k1, ksplit):
    sl = R.slice_bounds(k0, k1, ksplit)
    klen = -(-(-(-(k1 - k0) // ksplit)) // 16) * 16
    assert len(sl) == ksplit and sl[0][0] == k0 and sl[-1][1] == k1
    for s, (lo, hi) in enumerate(sl):
        assert lo % 16 == 0 and lo <= hi <= k1 and hi - lo <= klen
        assert lo == min(k1, k0 + s * klen)
        if s:
            assert lo == sl[s - 1][1]
    assert sum(hi - lo for lo, hi in sl) == k1 - k0
    if (k0, k1, ksplit) == (0, 1040, 3):
        assert sl == [(0, 352), (352, 704), (704, 1040)]          # the last slice is short


def test_slices_sum_to_the_unsplit_product():
    rng = np.random.default_rng(5)
    arena, args = R.case_predict(rng, 17, 192, ksplit=3)
    want, mask = R.expected(arena, args)
    one = dict(args, ksplit=0, bsC=0)
    want1, _ = R.expected(arena, one)
    parts = [R.mat(want, args["offC"] + s * args["bsC"], args["ldc"], 17, 256) for s in range(3)]
    assert np.array_equal(parts[0] + parts[1] + parts[2], R.mat(want1, args["offC"], args["ldc"], 17, 256))
    assert all(np.any(p) for p in parts)


def test_mask_classes_and_background():
    rng = np.random.default_rng(6)
    arena, args = R.case_trailing(rng, 129, 65, 32, -1.0, 1, tri=1)
    bg = R.background(arena.size)
    assert not np.any(bg == np.rint(bg)) and np.all(np.isfinite(bg))
    want, mask = R.expected(arena, args)
    cm = R.mat(mask, args["offC"], args["ldc"], 129, 65)
    i, j = np.indices(cm.shape)
    assert np.all(cm[j <= i] == R.MUST) and np.all(cm[j > i] == R.EITHER)
    assert np.count_nonzero(mask) == 129 * 65
    # everything outside the C rectangle is untouched in `want`, guard bands of at least GUARD elements at both ends
    assert np.array_equal(want[mask == R.BACKGROUND], arena[mask == R.BACKGROUND])
    first, last = np.flatnonzero(arena != bg)[[0, -1]]
    assert first >= R.GUARD and arena.size - 1 - last >= R.GUARD
    # a stray store, a wrong element and a lost update are each found and located
    got = want.copy()
    got[args["offC"] + 129 * args["ldc"] + 3] = 7.0             # one row past m
    got[args["offC"] + 5 * args["ldc"] + 2] += 1.0              # (5, 2) wrong
    got[args["offC"] + 2 * args["ldc"] + 9] = 123.0             # (2, 9), above the diagonal: neither old nor updated
    count, lines = R.mismatches(got, want, arena, mask, args)
    assert count == 3 and "(i, j) = (2, 9)" in lines[0] and "(i, j) = (5, 2)" in lines[1] and "(i, j) = (129, 3)" in lines[2]
    assert "either" in lines[0] and "must-equal" in lines[1] and "background" in lines[2]
    got = want.copy()
    upper = np.flatnonzero(mask == R.EITHER)
    got[upper[::2]] = arena[upper[::2]]                          # idle waves: old values above the diagonal are fine
    assert R.mismatches(got, want, arena, mask, args)[0] == 0


def test_factor_ahead_case_is_exact_and_fails_where_asked():
    rng = np.random.default_rng(7)
    arena, args, S = R.case_factor_ahead(rng, 256, 64, 2, bad_row=37, bad_matrix=1)
    want, mask = R.expected(arena, args, quantum=R.FA_QUANTUM, fa_failed=(1,))
    for b in range(2):
        blk = R.mat(want, args["offC"] + b * args["bsC"], args["ldc"], 64, 64)
        assert np.array_equal(blk, S[b])                         # the updated block is S itself, no rounding
        cm = R.mat(mask, args["offC"] + b * args["bsC"], args["ldc"], 64, 64)
        assert np.all(np.triu(cm, 1)[np.triu_indices(64, 1)] == R.UNSPECIFIED)
        assert np.all(cm[np.tril_indices(64)] == (R.FACTOR if b == 0 else R.UNSPECIFIED))
    np.linalg.cholesky(S[0])
    np.linalg.cholesky(S[1][:36, :36])                           # pivots 1 .. 36 of the bad matrix are positive
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(S[1][:37, :37])
