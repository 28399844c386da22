"""Reference for ONE launch of the Cholesky leaf kernels (leaf_factor_kernel, leaf_solve_kernel<STAGED, PRE>,
leaf_pair_kernel) through gpemu_test_leaf_launch: tests/test_gpu_leaf_kernels.py on the device, tests/test_leafref.py on
the CPU.  Test infrastructure only; plain numpy in numpy.longdouble (x87 extended, 2^-64), no device value is produced here.

The contract.  A launch leaves every element of the arena in one of three classes (classes()):

  UNCHANGED    the bits that were uploaded: everything outside the launch's footprint, and inside it
                 - factor: blocks (0,2) and (1,3) of the 4 x 4 grid of 16 x 16 blocks, and the strict upper triangles of the
                   four diagonal 16 x 16 blocks;
                 - solve: the whole diagonal block, and the panel rows >= m_below;
                 - pair: the diagonal block at c0, and the FIRST 64 rows under it in columns c0 .. c0+63 (every workgroup
                   solves them again for itself, a store there is a race; the next solve stores them, c0b);
  VALUE        a specified value with a bar (below);
  UNSPECIFIED  the footprint of a matrix whose pivot failed, and the strict upper part of the pair's second diagonal block
                 (with fa: outside the four parked inverses, which are VALUE).

The tests fill everything that is not an operand with NaN -- also inside the footprint: the upper triangles, blocks (0,2)
(1,3) and, for pre = 0, the parked blocks -- so whatever a kernel reads beside its operands shows in a VALUE element.

The bars.  u = 2^-53.  Every constant is a count of roundings (first order in u: with c u < 4e-14 the second-order terms
are below 1e-13 of the bar); the bars are evaluated in longdouble from the values the DEVICE returned, so that nothing
propagates from one step to the next and a bar never depends on the conditioning of the whole block.

  C_FACTOR = 78   |L L^T - A|_ij <= C_FACTOR u (|L||L^T|)_ij, the componentwise backward bound of the Cholesky
                  factorisation (Higham, Accuracy and Stability, Thm 10.3) with the constant of THIS algorithm:
                  64  element (i,j) is a_ij minus at most 63 products, each subtracted with ONE rounding (fma in the panel,
                      the matrix unit's fused accumulation in the trailing updates), and one product by 1/sqrt(pivot);
                  14  = 2 x (6 + 1): l_ij l_jj = a'_ij p rs^2, rs = 1/sqrt(p) from the hardware estimate and two Newton
                      steps of three roundings each (t = p rs; e = fma(-t, rs, 1); rs = fma(rs/2, e, rs)) -- at most 6 u
                      however the errors of the steps combine -- and the rounding of p rs and a rs.
  C_INV = 276     parked inverse P_j of the RETURNED diagonal block L_jj = D (I + N):  |P_j - L_jj^-1| <= C_INV u S / |d|,
                  S = (I + |N|)(I + |N|^2)(I + |N|^4)(I + |N|^8), the kernel's own products evaluated on |N| (every
                  intermediate of the series is bounded by its |N| version), column q divided by |d_q|.  A product of two
                  16 x 16 factors with relative coefficients a and b (|fl(X) - X| <= a u |X|_N) has a + b + 16 (sixteen fused
                  accumulations); adding I costs 1:
                    N = L / d (two-step Newton reciprocal, 2, and the product, 1)                3
                    N^2 = 3 + 3 + 16 = 22,  N^4 = 22 + 22 + 16 = 60,  N^8 = 60 + 60 + 16 = 136
                    Q1 = (I - N)(I + N^2) = 4 + 23 + 16 = 43,  Q2 = Q1 (I + N^4) = 43 + 61 + 16 = 120
                    Q3 = Q2 (I + N^8) = 120 + 137 + 16 = 273,  P = Q3 / d                      276
                  Above its diagonal S is zero: the parked block is exactly zero there.
  C_SOLVE = 64    step j of X L^T = B, row form, from the device's own X_i, i < j:
                    X_j = (B_j - sum_{i<j} X_i L_ji^T) L_jj^-T,  acc = |B_j| + sum_{i<j} |X_i||L_ji|^T
                    |X_j - exact| <= C_SOLVE u acc |L_jj^-1|^T + C_INV u acc (S/|d|)^T
                  48 fused accumulations at most into B_j, 16 in the product with the inverse; the second term is the error
                  of the inverse the kernel multiplies with (C_INV), applied to the same absolute accumulator.
  C_UPDATE = 64   C2 - X1 X0^T, K = 64 fused accumulations into C2:  <= C_UPDATE u (|C2| + |X1||X0|^T), from the device's X.
                  (tests/test_gpu_gemm_modes.py's bar, 1e-13 of the largest element of the result, is asserted beside it on the
                  well-conditioned class -- the regime that bar is used in; on the covariance classes the result is
                  1e-6 .. 1e-8 of its terms.)
  The factor-ahead tile of the pair factors the UPDATED block, which never reaches memory: its bar is the sum
  C_FACTOR u |L||L^T| + C_UPDATE u (|C2| + |X0||X0|^T) against C2 - X0 X0^T.

Measured on the float64 restatement of the kernels (tests/test_leafref.py): the series inverse stays below 5 u S/|d| on
64 x 64 pow-exp covariance blocks of condition 1e4 .. 6e11, so the bars leave room; a device value beyond one is a finding."""
import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53
LEAF = 64
FACTOR, SOLVE, FACTOR_SOLVE, PAIR = 0, 1, 2, 3
PARKED = ((0, 1), (1, 2), (2, 3), (0, 3))        # the inverse of diagonal 16x16 block j sits in block PARKED[j]
C_FACTOR, C_INV, C_SOLVE, C_UPDATE = 78, 276, 64, 64
UNCHANGED, VALUE, UNSPECIFIED = 0, 1, 2
INPUT_CLASSES = ("well", "cov1", "cov2")         # G G^T + 64 I; pow-exp d = 1 (cond ~ 4e7); pow-exp d = 2 (cond ~ 4e9)


# ------------------------------------------------------------------ layout
def layout(ld, rows, nbatch=0):
    """an arena of NaN for max(nbatch, 1) matrices of rows x ld, a guard band in front, between and behind them
    -> (arena, dict(off, ld, bstride, nbatch))"""
    off, bstride = 34, rows * ld + 70
    arena = np.full(off + max(nbatch, 1) * bstride + 30, np.nan)
    return arena, dict(off=off, ld=ld, bstride=bstride, nbatch=nbatch)


def matrix(arena, lay, rows, b=0):
    """view of matrix b: rows x ld"""
    o = lay["off"] + b * lay["bstride"]
    return arena[o:o + rows * lay["ld"]].reshape(rows, lay["ld"])


def written_by_factor():
    """64 x 64 mask of what a factor launch specifies: the lower triangle and the four parked blocks"""
    i, j = np.indices((LEAF, LEAF))
    m = i >= j
    for r, c in PARKED:
        m |= (i // 16 == r) & (j // 16 == c)
    return m


def classes(size, lay, rows, args, failed=()):
    """class of every arena element after the launch `args` (op, c0, m_below, c0b, fa); failed: matrices whose pivot failed"""
    cls = np.zeros(size, dtype=np.int8)
    op, c0, m, fa, c0b = args["op"], args["c0"], args.get("m_below", 0), args.get("fa", 0), args.get("c0b", -1)
    for b in range(max(lay["nbatch"], 1)):
        M = matrix(cls, lay, rows, b)
        if op in (FACTOR, FACTOR_SOLVE):
            M[c0:c0 + LEAF, c0:c0 + LEAF][written_by_factor()] = VALUE
        if op in (SOLVE, FACTOR_SOLVE):
            M[c0 + LEAF:c0 + LEAF + m, c0:c0 + LEAF] = VALUE
            if c0b >= 0:
                M[c0b + LEAF:c0b + 2 * LEAF, c0b:c0b + LEAF] = VALUE
        if op == PAIR:
            M[c0 + 2 * LEAF:c0 + LEAF + m, c0:c0 + LEAF] = VALUE
            M[c0 + LEAF:c0 + LEAF + m, c0 + LEAF:c0 + 2 * LEAF] = VALUE
            D2 = M[c0 + LEAF:c0 + 2 * LEAF, c0 + LEAF:c0 + 2 * LEAF]
            i, j = np.indices((LEAF, LEAF))
            D2[j > i] = UNSPECIFIED
            if fa:
                D2[written_by_factor()] = VALUE
        if b in failed:
            M[M == VALUE] = UNSPECIFIED
    return cls


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.int64),
                          np.ascontiguousarray(b, dtype=np.float64).view(np.int64))


# ------------------------------------------------------------------ inputs
def problem(cls, seed, m):
    """seeded symmetric positive definite K of side 64 + m: K[:64, :64] is the block a launch factors, K[64:, :64] the panel
    rows under it, K[64:, 64:128] the pair's second block column"""
    rng = np.random.default_rng(seed)
    n = LEAF + m
    if cls == "well":
        G = rng.standard_normal((n, LEAF))
        return G @ G.T + 64.0 * np.eye(n)
    d, length, nugget = {"cov1": (1, 0.3, 1e-6), "cov2": (2, 0.5, 1e-8)}[cls]
    X = rng.random((n, d))
    r2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2)
    return np.exp(-0.5 * r2 / length ** 2) + nugget * np.eye(n)


def fail_pivot(K, rows, how="negative"):
    """K with the pivots of the 1-based rows `rows` (one row or several) of the leading 64 x 64 block made to fail: -1
    (robustly negative; each as if the rows before it had not failed), exactly 0.0 (row 1 only: the pivot is the element)
    or NaN"""
    rows = (rows,) if np.isscalar(rows) else tuple(rows)
    L = np.linalg.cholesky(K[:LEAF, :LEAF])
    K = K.copy()
    for row in rows:
        r = row - 1
        if how == "nan":
            K[r, r] = np.nan
        elif how == "zero":
            assert r == 0
            K[r, r] = 0.0
        else:
            K[r, r] -= L[r, r] ** 2 + 1.0
    return K


def fill(M, c0, K, pair=False):
    """the operands of a launch at c0 from K into matrix view M, everything else stays NaN: the lower triangle of the
    diagonal block, the panel rows, and for the pair columns 64 .. 127 with only the lower triangle of their first block"""
    m = K.shape[0] - LEAF
    i, j = np.indices((LEAF, LEAF))
    D = M[c0:c0 + LEAF, c0:c0 + LEAF]
    D[i >= j] = K[:LEAF, :LEAF][i >= j]
    M[c0 + LEAF:c0 + LEAF + m, c0:c0 + LEAF] = K[LEAF:, :LEAF]
    if pair:
        M[c0 + LEAF:c0 + LEAF + m, c0 + LEAF:c0 + 2 * LEAF] = K[LEAF:, LEAF:2 * LEAF]
        D2 = M[c0 + LEAF:c0 + 2 * LEAF, c0 + LEAF:c0 + 2 * LEAF]
        D2[j > i] = np.nan


def int_problem(seed, m):
    """integer-valued case whose solve and update are exact in fp64 in any order: unit-lower L (strict part in {-1, 0, 1},
    sparse), the exact integer inverses of its diagonal 16 x 16 blocks, integer panel rows B and second block column C2
    -> (block 64 x 64: L below, inverses parked, NaN elsewhere; B m x 64; C2 m x 64; X = B L^-T exactly)"""
    rng = np.random.default_rng(seed)
    i, j = np.indices((LEAF, LEAF))
    L = np.where(i > j, rng.integers(-1, 2, (LEAF, LEAF)) * (rng.random((LEAF, LEAF)) < 0.12), 0).astype(np.float64) + np.eye(LEAF)
    B = rng.integers(-4, 5, (m, LEAF)).astype(np.float64)
    C2 = rng.integers(-8, 9, (m, LEAF)).astype(np.float64)
    blk = np.full((LEAF, LEAF), np.nan)
    blk[i >= j] = L[i >= j]
    for q, (r, c) in enumerate(PARKED):
        inv = tri_inverse_exact(L[16 * q:16 * q + 16, 16 * q:16 * q + 16])
        assert np.array_equal(inv, np.rint(inv))
        blk[16 * r:16 * r + 16, 16 * c:16 * c + 16] = inv.astype(np.float64)
    # every partial sum of any order is bounded by the same computation on absolute values: keep that below 2^50
    W = np.linalg.inv(2.0 * np.eye(LEAF) - np.abs(L))            # sum_k |N|^k >= |L^-1|
    Xabs = np.abs(B) @ W.T
    assert LEAF * Xabs.max() * W.max() < 2.0 ** 50 and LEAF * Xabs.max() ** 2 + 8 < 2.0 ** 50
    X = np.array(solve_exact(L, B), dtype=np.float64)
    assert np.array_equal(X @ L.T, B)
    return blk, B, C2, X


# ------------------------------------------------------------------ exact pieces
def tri_inverse_exact(D):
    """inverse of a lower-triangular block by forward substitution in longdouble"""
    D = np.asarray(D, dtype=LD)
    n = D.shape[0]
    inv = np.zeros((n, n), dtype=LD)
    for c in range(n):
        for r in range(c, n):
            s = (LD(1) if r == c else LD(0)) - D[r, c:r] @ inv[c:r, c]
            inv[r, c] = s / D[r, r]
    return inv


def solve_exact(L, B):
    """X with X L^T = B by substitution in longdouble"""
    L, B = np.asarray(L, dtype=LD), np.asarray(B, dtype=LD)
    X = np.zeros_like(B)
    for c in range(L.shape[0]):
        X[:, c] = (B[:, c] - X[:, :c] @ L[c, :c]) / L[c, c]
    return X


def series_bound(D):
    """S / |d|: (I + |N|)(I + |N|^2)(I + |N|^4)(I + |N|^8) with N = D^-1 strict(L), column q divided by |L_qq|"""
    D = np.asarray(D, dtype=LD)
    d = np.abs(np.diag(D))
    N = np.abs(np.tril(D, -1)) / d[:, None]
    I = np.eye(D.shape[0], dtype=LD)
    N2 = N @ N
    N4 = N2 @ N2
    N8 = N4 @ N4
    return (I + N) @ (I + N2) @ (I + N4) @ (I + N8) / d[None, :]


def ratio(err, bar):
    """max of error / bar; an error that is not a number, or is not zero where the bar is zero, counts as infinite"""
    err, bar = np.asarray(err, dtype=LD), np.asarray(bar, dtype=LD)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, LD(0), err / bar)
    r = np.where(np.isnan(r), LD(np.inf), r)
    return float(r.max())


# ------------------------------------------------------------------ checks (error / bar, < 1 passes)
def check_inverses(blk):
    """the four parked blocks of a returned 64 x 64 block against the exact inverses of ITS diagonal 16 x 16 blocks"""
    worst = 0.0
    for q, (r, c) in enumerate(PARKED):
        D = np.tril(blk[16 * q:16 * q + 16, 16 * q:16 * q + 16])
        P = np.asarray(blk[16 * r:16 * r + 16, 16 * c:16 * c + 16], dtype=LD)
        worst = max(worst, ratio(np.abs(P - tri_inverse_exact(D)), C_INV * U * series_bound(D)))
    return worst


def check_factor(A, blk, extra=None):
    """a returned 64 x 64 block against the matrix A it was factored from (lower triangle)
    -> dict(factor, inverse); extra: added to the factor's bar (the pair's update before the factorisation)"""
    L = np.tril(np.asarray(blk, dtype=LD))
    i, j = np.indices((LEAF, LEAF))
    low = i >= j
    res = np.abs(L @ L.T - np.asarray(A, dtype=LD))
    bar = C_FACTOR * U * (np.abs(L) @ np.abs(L).T)
    if extra is not None:
        bar = bar + extra
    return dict(factor=ratio(res[low], bar[low]), inverse=check_inverses(blk))


def check_solve(blk, B, X):
    """m x 64 returned rows X against the rows B before the launch, step by step from the returned X itself; blk: the
    factored 64 x 64 block the launch read"""
    L = np.tril(np.asarray(blk, dtype=LD))
    B, X = np.asarray(B, dtype=LD), np.asarray(X, dtype=LD)
    worst = 0.0
    for j in range(4):
        s = slice(16 * j, 16 * j + 16)
        inv, bound = tri_inverse_exact(L[s, s]), series_bound(L[s, s])
        acc, aabs = B[:, s].copy(), np.abs(B[:, s])
        for i in range(j):
            t = slice(16 * i, 16 * i + 16)
            acc -= X[:, t] @ L[s, t].T
            aabs += np.abs(X[:, t]) @ np.abs(L[s, t]).T
        bar = C_SOLVE * U * (aabs @ np.abs(inv).T) + C_INV * U * (aabs @ bound.T)
        worst = max(worst, ratio(np.abs(X[:, s] - acc @ inv.T), bar))
    return worst


def update_bar(C2, X1, X0):
    return C_UPDATE * U * (np.abs(np.asarray(C2, dtype=LD)) + np.abs(np.asarray(X1, dtype=LD)) @ np.abs(np.asarray(X0, dtype=LD)).T)


def check_update(C2, X1, X0, out, fa):
    """the pair's columns 64 .. 127 (m x 64, before: C2, after: out) against C2 - X1 X0^T from solved rows X1 (m x 64) and
    X0 = X1[:64]; the first 64 rows: the lower triangle (fa: the factor of the updated block instead, with its inverses)
    -> dict(update, relerr[, factor, inverse])"""
    want = np.asarray(C2, dtype=LD) - np.asarray(X1, dtype=LD) @ np.asarray(X0, dtype=LD).T
    bar = update_bar(C2, X1, X0)
    i, j = np.indices(want.shape)
    spec = (i >= LEAF) if fa else (i >= j)
    err = np.abs(np.asarray(out, dtype=LD) - want)
    with np.errstate(invalid="ignore"):
        res = dict(update=ratio(err[spec], bar[spec]),
                   relerr=float(np.nan_to_num(err[spec], nan=np.inf).max() / np.abs(want[spec]).max()) if spec.any() else 0.0)
    if fa:
        res.update(check_factor(want[:LEAF], out[:LEAF], extra=bar[:LEAF]))
    return res


# ------------------------------------------------------------------ the cases both test files use
SOLVE_M = (1, 2, 15, 16, 17, 63, 64, 65, 127, 130)
PAIR_M = (64, 128, 320)
FAIL_ROWS = (1, 2, 16, 17, 32, 48, 49, 64)


def seed(cls, m):
    return 1000 * (1 + INPUT_CLASSES.index(cls)) + m


def pair_problem_with_failed_tile(cls, m, row, how="negative"):
    """a pair problem whose UPDATED second diagonal block C2 - X0 X0^T fails at 1-based pivot `row`: K as problem(), the
    second diagonal block replaced by X0 X0^T + S with S = fail_pivot(a positive definite block) -> (K, S)"""
    K = problem(cls, seed(cls, m) + 500 + row, m)
    L = np.linalg.cholesky(K[:LEAF, :LEAF])
    X0 = np.array(solve_exact(L, K[LEAF:2 * LEAF, :LEAF]), dtype=np.float64)
    S = fail_pivot(problem("well", 900 + row, 0), row, how)
    K[LEAF:2 * LEAF, LEAF:2 * LEAF] = X0 @ X0.T + S
    return K, S


def big_rows(b, m):
    """standard-normal panel rows of matrix b of the 64-matrix launches"""
    return np.random.default_rng(5000 + b).standard_normal((m, LEAF))
