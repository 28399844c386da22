"""tests/leafref.py against itself and against mpmath, and its bars against a float64 restatement of the leaf kernels'
formulas (the series inverse, the panel factorisation with rank-16 updates, the block chain of the solve, the K = 64
update) on every input tests/test_gpu_leaf_kernels.py uses: error / bar < 1 everywhere, so that no device test is born
failing.  CPU only.

Measured here: factor <= 0.08, parked inverses <= 0.02, solve <= 0.01, pair update <= 0.12, pair factor <= 0.11 of their bars."""
import numpy as np
import pytest

import leafref as R

LD = R.LD


# ------------------------------------------------------------------ the kernels' formulas in float64
def model_series_inverse(D):
    """tri_inverse16_to: L = d (I + N); (I - N)(I + N^2)(I + N^4)(I + N^8), column q times 1/L_qq"""
    d = np.diag(D)
    N = np.tril(D, -1) * (1.0 / d)[:, None]
    I = np.eye(16)
    S = N @ N
    Q = (I - N) @ (I + S)
    for _ in range(2):
        S = S @ S
        Q = Q @ (I + S)
    return Q * (1.0 / d)[None, :]


def model_factor(A):
    """leaf_factor_kernel: four 16-column panels, 1/sqrt of the pivot, rank-16 trailing updates; the inverses parked
    -> (block: L below, inverses parked, NaN elsewhere; 1-based first failed pivot or 0)"""
    A = np.tril(np.array(A, dtype=np.float64))
    bad = 0
    for P in range(4):
        for k in range(16 * P, 16 * P + 16):
            p = A[k, k]
            if not (p > 0.0) and bad == 0:
                bad = k + 1
            with np.errstate(invalid="ignore", divide="ignore"):
                rs = 1.0 / np.sqrt(p)
                A[k:, k] = A[k:, k] * rs
                for c in range(k + 1, 16 * P + 16):
                    A[c:, c] -= A[c:, k] * A[c, k]
        e = 16 * P + 16
        with np.errstate(invalid="ignore"):
            A[e:, e:] -= np.tril(A[e:, 16 * P:e] @ A[e:, 16 * P:e].T)
    blk = np.full((64, 64), np.nan)
    i, j = np.indices((64, 64))
    blk[i >= j] = A[i >= j]
    for q, (r, c) in enumerate(R.PARKED):
        blk[16 * r:16 * r + 16, 16 * c:16 * c + 16] = model_series_inverse(A[16 * q:16 * q + 16, 16 * q:16 * q + 16])
    return blk, bad


def model_solve(blk, B):
    """leaf_solve_kernel / leaf_chain: X_j = (B_j - sum_{i<j} X_i L_ji^T) P_j^T with the parked inverses P_j"""
    X = np.zeros_like(B)
    for j in range(4):
        s = slice(16 * j, 16 * j + 16)
        acc = B[:, s].copy()
        for i in range(j):
            t = slice(16 * i, 16 * i + 16)
            acc -= X[:, t] @ blk[s, t].T
        r, c = R.PARKED[j]
        X[:, s] = acc @ blk[16 * r:16 * r + 16, 16 * c:16 * c + 16].T
    return X


def model_pair(blk, B, C2, fa):
    X = model_solve(blk, B)
    out = C2 - X @ X[:64].T
    bad = 0
    if fa:
        out[:64], bad = model_factor(out[:64])
    return X, out, bad


# ------------------------------------------------------------------ the reference's own pieces
def test_exact_pieces_against_mpmath():
    """tri_inverse_exact, solve_exact and series_bound on a 16 x 16 block of the d = 1 covariance class, against mpmath at
    50 digits: the longdouble routes agree to 1e-17 relative to the bound the bars are built on (the bars start at 64 u)"""
    import mpmath as mp
    mp.mp.dps = 50
    K = R.problem("cov1", 5, 0)
    L = np.linalg.cholesky(K)[16:32, 16:32]
    Lm = mp.matrix(L.tolist())
    inv_m = mp.inverse(Lm)
    inv = R.tri_inverse_exact(L)
    bound = R.series_bound(L)
    d = [abs(Lm[i, i]) for i in range(16)]
    Nm = mp.matrix(16, 16)
    for i in range(16):
        for j in range(i):
            Nm[i, j] = abs(Lm[i, j]) / d[i]
    I = mp.eye(16)
    Sm = (I + Nm) * (I + Nm ** 2) * (I + Nm ** 4) * (I + Nm ** 8)
    worst_inv = worst_bound = 0.0
    for i in range(16):
        for j in range(16):
            want_b = Sm[i, j] / d[j]
            if j > i:
                assert inv[i, j] == 0 and bound[i, j] == 0
                continue
            worst_inv = max(worst_inv, float(abs(mp.mpf(float(inv[i, j])) + mp.mpf(float(inv[i, j] - LD(float(inv[i, j])))) - inv_m[i, j]) / want_b))
            worst_bound = max(worst_bound, float(abs(mp.mpf(float(bound[i, j])) - want_b) / want_b))
            assert abs(inv_m[i, j]) <= want_b * (1 + mp.mpf(10) ** -30)          # the series bound does bound the inverse
    print(f"longdouble inverse against mpmath: {worst_inv:.2e} of the series bound; bound itself {worst_bound:.2e}")
    assert worst_inv < 1e-17 and worst_bound < 1e-15
    B = np.random.default_rng(3).standard_normal((5, 16))
    X = R.solve_exact(L, B)
    Xm = mp.matrix(B.tolist()) * inv_m.T
    scale = np.abs(B) @ np.asarray(bound, dtype=np.float64).T
    err = max(abs(float(mp.mpf(float(X[i, j])) - Xm[i, j])) / scale[i, j] for i in range(5) for j in range(16))
    assert err < 1e-16, err


def test_classes_of_a_factor_launch():
    arena, lay = R.layout(200, 128)
    cls = R.classes(arena.size, lay, 128, dict(op=R.FACTOR, c0=64))
    D = R.matrix(cls, lay, 128)[64:128, 64:128]
    assert cls.sum() == D.sum() == 64 * 65 // 2 + 4 * 256
    for blk in ((0, 2), (1, 3)):
        assert not D[16 * blk[0]:16 * blk[0] + 16, 16 * blk[1]:16 * blk[1] + 16].any()
    for q in range(4):
        assert not np.triu(D[16 * q:16 * q + 16, 16 * q:16 * q + 16], 1).any()
    cls = R.classes(arena.size, lay, 128, dict(op=R.FACTOR, c0=64), failed=(0,))
    assert (cls == R.VALUE).sum() == 0 and (cls == R.UNSPECIFIED).sum() == 64 * 65 // 2 + 4 * 256


def test_classes_of_a_pair_launch():
    arena, lay = R.layout(192, 64 + 64 + 128, nbatch=3)
    for fa in (0, 1):
        cls = R.classes(arena.size, lay, 256, dict(op=R.PAIR, c0=64, m_below=128, fa=fa))
        for b in range(3):
            M = R.matrix(cls, lay, 256, b)
            assert not M[:128].any() and not M[128:192, 64:128].any()         # diagonal block, first 64 rows: unchanged
            assert (M[192:256, 64:192] == R.VALUE).all()
            D2 = M[128:192, 128:192]
            assert (np.tril(D2) == R.VALUE)[np.tril_indices(64)].all()
            assert (D2 == R.UNSPECIFIED).sum() == 64 * 63 // 2 - (4 * 256 if fa else 0)
        assert (cls != 0).sum() == 3 * (64 * 64 + 128 * 64)


def test_a_wrong_value_misses_its_bar():
    """the bars see one element of a well-conditioned case off by 1e-12 relative, and on a covariance block a dropped
    series factor and two swapped parked blocks"""
    K = R.problem("well", R.seed("well", 17), 17)
    blk, bad = model_factor(K[:64, :64])
    assert bad == 0
    X = model_solve(blk, K[64:, :64])
    assert R.check_solve(blk, K[64:, :64], X) < 1
    X2 = X.copy()
    X2[3, 40] *= 1 + 1e-12
    assert R.check_solve(blk, K[64:, :64], X2) > 1
    b2 = blk.copy()
    b2[20, 3] *= 1 + 1e-12
    assert R.check_factor(K[:64, :64], b2)["factor"] > 1
    K = R.problem("cov1", R.seed("cov1", 17), 17)
    blk, bad = model_factor(K[:64, :64])
    b3 = blk.copy()
    b3[0:16, 16:32], b3[16:32, 32:48] = blk[16:32, 32:48], blk[0:16, 16:32]
    assert R.check_inverses(b3) > 1
    D = blk[16:32, 16:32]
    d = np.diag(D)
    N = np.tril(D, -1) / d[:, None]
    short = (np.eye(16) - N) @ (np.eye(16) + N @ N) @ (np.eye(16) + np.linalg.matrix_power(N, 4)) / d[None, :]   # no (I + N^8)
    b4 = blk.copy()
    b4[16:32, 32:48] = short
    assert R.check_inverses(b4) > 1


# ------------------------------------------------------------------ every GPU input through the float64 restatement
WORST = {}


def note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), value)
    assert value < 1, (key, value)


@pytest.mark.parametrize("cls", R.INPUT_CLASSES)
def test_model_meets_the_bars_factor_and_solve(cls):
    for m in R.SOLVE_M:
        K = R.problem(cls, R.seed(cls, m), m)
        blk, bad = model_factor(K[:64, :64])
        assert bad == 0
        res = R.check_factor(K[:64, :64], blk)
        note(("factor", cls), res["factor"])
        note(("inverse", cls), res["inverse"])
        note(("solve", cls), R.check_solve(blk, K[64:, :64], model_solve(blk, K[64:, :64])))
    if cls == "well":
        L = np.linalg.cholesky(K[:64, :64])
        assert np.max(np.abs(np.tril(blk) - L)) / np.max(np.abs(L)) < 1e-13
    print({k: f"{v:.3f}" for k, v in WORST.items() if k[1] == cls})


@pytest.mark.parametrize("cls", R.INPUT_CLASSES)
def test_model_meets_the_bars_pair(cls):
    for m in R.PAIR_M:
        K = R.problem(cls, R.seed(cls, m), m)
        blk, _ = model_factor(K[:64, :64])
        for fa in (0, 1):
            X, out, bad = model_pair(blk, K[64:, :64], K[64:, 64:128].copy(), fa)
            assert bad == 0
            res = R.check_update(K[64:, 64:128], X, X[:64], out, fa)
            assert res.pop("relerr") < 1e-13 or cls != "well"
            for k, v in res.items():
                note(("pair " + k, cls), v)
    print({k: f"{v:.3f}" for k, v in WORST.items() if k[1] == cls and k[0].startswith("pair")})


@pytest.mark.parametrize("how,rows", [("negative", R.FAIL_ROWS), ("nan", (1, 17, 64)), ("zero", (1,))])
def test_model_reports_the_failed_pivot(how, rows):
    for row in rows:
        K = R.fail_pivot(R.problem("well", 7, 0), row, how)
        _, bad = model_factor(K)
        assert bad == row
    K = R.fail_pivot(R.problem("well", 7, 0), (33, 17))
    assert model_factor(K)[1] == 17


def test_model_fails_the_pair_tile_at_the_row():
    """the second block column is built so that the UPDATED block has the failing pivot: C2 = X0 X0^T + S"""
    for row in R.FAIL_ROWS:
        K, S = R.pair_problem_with_failed_tile("well", 64, row)
        blk, _ = model_factor(K[:64, :64])
        _, _, bad = model_pair(blk, K[64:, :64], K[64:, 64:128].copy(), 1)
        assert bad == row


def test_model_meets_the_bars_on_the_big_launch_rows():
    blk, _ = model_factor(R.problem("well", R.seed("well", 64), 64)[:64, :64])
    for m in (1024, 960):
        for b in (0, 63):
            B = R.big_rows(b, m)
            note(("solve automatic", "well"), R.check_solve(blk, B, model_solve(blk, B)))


def test_integer_case_is_exact():
    for m in (1, 17, 64, 128, 130, 320):
        blk, B, C2, X = R.int_problem(m, m)
        assert 9 * (64 * np.abs(X).max() ** 2 + 8) < 2.0 ** 52                  # the GPU test scales B by up to 3
        got = model_solve(blk, B)
        assert np.array_equal(got, X)
        assert R.check_solve(blk, B, got) == 0.0
        if m % 64 == 0:
            _, out, _ = model_pair(blk, B, C2.copy(), 0)
            assert np.array_equal(out, C2 - X @ X[:64].T)
