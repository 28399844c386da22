"""CPU reference for single launches of gemm_nt_kernel (tests/test_gpu_gemm_modes.py, tests/test_gemmref.py).  Test
infrastructure only: plain functions, no device.

A launch is described by the fields of gpemu_gemm_launch_args (include/gpemu.h) as a dict `args`, and works on operands
inside ONE flat float64 array, the arena, as in production, where C sits in the same tall workspace as A and B.

Exact method.  The integer operands are uniform integers in [-8, 8] stored as float64.  With K <= 4096 every product
and every partial sum of C = beta*C + alpha * A B^T is an integer below 2**53 (assert_exact checks the operands that
are really used), so every summation order gives the same fp64 result and the reference (numpy matmul) is the ONLY
correct answer: the GPU tests assert equality, no tolerance.

Zero patterns the skipping modes of the kernel rely on (the contract of gpemu_test_gemm_launch):
  kstart_mode:  A[i][k] = 0 for k < i - kstart_off; the first kstart_off rows are dense: the [Z^T; U] layout of the
                corner product C^-1 = U U^T
  kend_mode:    B[j][k] = 0 for k > j - kend_off while j < k1; rows j >= k1 are dense: the 64 augmented rows behind
                the triangular rows of L^-1 in the prediction product (n = k1 + 64)
Under them the product over the skipped ranges equals the full product over [k0, k1), which is what expected() computes.

Background.  Every element of the arena that is no operand holds 0.5 + (index % 1021): finite, never an integer, so a
stray store cannot pass for data, and a stray read puts a half into an integer result.  Guard bands of GUARD elements
lie before the first and after every operand region.  Leading dimensions and offsets are multiples of 8 elements:
rows start on 64-byte boundaries, as those of every production operand do.

Mask classes of expected():
  BACKGROUND   must be bit-identical to what was uploaded (A and B themselves, padding columns, rows past m, gaps, guards)
  MUST         must equal the reference: [0,m) x [0,n) of each C block; under tri the elements with j <= i
  EITHER       under tri, j > i inside the C rectangle: bit-identical to the value before the launch (idle waves,
               skipped tiles) or equal to the full update (the other waves of a tile on the diagonal)
  UNSPECIFIED  with fa, the strictly upper part of the 64x64 block (0,0), where the inverses of the 16x16 diagonal
               blocks are parked (and the whole block of a matrix whose factorisation failed)
  FACTOR       with fa, the lower triangle of block (0,0): the Cholesky factor of the updated block
"""
import numpy as np

GUARD = 4096
BK = 16
LEAF = 64
BACKGROUND, MUST, EITHER, UNSPECIFIED, FACTOR = 0, 1, 2, 3, 4
CLASS_NAMES = ("background", "must-equal", "either", "unspecified", "factor")

DEFAULTS = dict(offC=0, offA=0, offB=0, ldc=0, lda=0, ldb=0, bsC=0, bsA=0, bsB=0, alpha=1.0, m=0, n=0, k0=0, k1=0, beta=0,
                tri=0, kstart_mode=0, kstart_off=0, kend_mode=0, kend_off=0, nbatch=0, ksplit=0, force_cfg=0, fa=0, fa_c0=0)


def round_up(x, q):
    return -(-x // q) * q


def full_args(args):
    a = dict(DEFAULTS)
    assert set(args) <= set(a), set(args) - set(a)
    a.update(args)
    return a


def nblocks(args):
    a = full_args(args)
    return max(a["nbatch"], a["ksplit"], 1)


# ------------------------------------------------------------------ arena
def background(n):
    return 0.5 + (np.arange(n, dtype=np.int64) % 1021).astype(np.float64)


class Layout:
    """hands out regions of an arena with a guard band before the first and after each of them"""

    def __init__(self):
        self.n = GUARD

    def reserve(self, nelem):
        off = self.n
        self.n += round_up(nelem, 8) + GUARD
        return off

    def arena(self):
        return background(self.n)


def mat(arena, off, ld, rows, cols):
    """writable rows x cols view of the matrix at element offset `off` with leading dimension `ld`"""
    assert off >= 0 and rows >= 1 and cols >= 1 and off + (rows - 1) * ld + cols <= arena.size
    return np.lib.stride_tricks.as_strided(arena[off:], shape=(rows, cols), strides=(ld * arena.itemsize, arena.itemsize))


# ------------------------------------------------------------------ operands
def operand(rng, rows, cols, kind):
    """kind "int": uniform integers in [-8, 8] as float64; "normal": standard normal"""
    if kind == "int":
        return rng.integers(-8, 9, size=(rows, cols)).astype(np.float64)
    assert kind == "normal"
    return rng.standard_normal((rows, cols))


def kstart_operand(rng, rows, cols, off, kind="int"):
    """A[i][k] = 0 (exactly) for k < i - off"""
    A = operand(rng, rows, cols, kind)
    i, k = np.indices(A.shape)
    A[k < i - off] = 0.0
    return A


def kend_operand(rng, rows, cols, off, k1, kind="int"):
    """B[j][k] = 0 (exactly) for k > j - off while j < k1"""
    B = operand(rng, rows, cols, kind)
    j, k = np.indices(B.shape)
    B[(k > j - off) & (j < k1)] = 0.0
    return B


def assert_exact(A, B, C0=None, alpha=1.0, quantum=1.0):
    """the precondition of the exact method: A and B hold integers, C0 multiples of `quantum` (a power of two), and
    max |partial sum| of C0 +- A B^T, whatever the order, stays below 2**53 quanta.  alpha is +-1, or 1/2 on a product
    alone (halving an integer below 2**53 is exact).  -> the bound on the partial sums"""
    assert np.array_equal(A, np.rint(A)) and np.array_equal(B, np.rint(B))
    assert alpha in (1.0, -1.0) or (alpha == 0.5 and C0 is None)
    bound = A.shape[1] * float(np.max(np.abs(A))) * float(np.max(np.abs(B)))
    if C0 is not None:
        assert np.array_equal(C0 / quantum, np.rint(C0 / quantum))
        bound += float(np.max(np.abs(C0)))
    assert bound / quantum < 2.0 ** 53, bound
    return bound


# ------------------------------------------------------------------ split-K
def slice_bounds(k0, k1, ksplit):
    """[lo, hi) of every k-slice: klen = ceil16(ceil((k1 - k0) / ksplit)), slice s = [k0 + s klen, min(k1, k0 + (s+1) klen));
    a slice that starts at or beyond k1 is empty (lo = hi = k1)"""
    klen = round_up(-(-(k1 - k0) // ksplit), BK)
    out = []
    for s in range(ksplit):
        lo = min(k1, k0 + s * klen)
        out.append((lo, min(k1, lo + klen)))
    return out


def element_bounds(args, i, j, s=0):
    """the k-range element (i, j) of block s contracts over when the promised zeros are left out: the slice (or [k0, k1)),
    intersected with k >= i - kstart_off and k <= j - kend_off (rows j >= k1 of B are dense)"""
    a = full_args(args)
    lo, hi = slice_bounds(a["k0"], a["k1"], a["ksplit"])[s] if a["ksplit"] > 1 else (a["k0"], a["k1"])
    if a["kstart_mode"]:
        lo = max(lo, i - a["kstart_off"])
    if a["kend_mode"] and j < a["k1"]:
        hi = min(hi, j - a["kend_off"] + 1)
    return lo, max(lo, hi)


# ------------------------------------------------------------------ the reference
def expected(arena, args, exact=True, quantum=1.0, fa_failed=()):
    """-> (want, mask): the arena after a correct launch of `args` on `arena` and the class of every element (module
    docstring).  Inside the C rectangles `want` holds the full update everywhere, also where the mask says EITHER; the
    FACTOR and UNSPECIFIED elements of `want` hold the updated, not yet factored block.  exact: check the 2**53
    precondition on the operands."""
    a = full_args(args)
    m, n, k0, k1 = a["m"], a["n"], a["k0"], a["k1"]
    assert k0 % BK == 0 and k1 % BK == 0 and k0 < k1 and a["beta"] in (0, 1)
    split = a["ksplit"] > 1
    want = arena.copy()
    mask = np.zeros(arena.size, dtype=np.uint8)
    lower = np.tril(np.ones((m, n), dtype=bool))
    for b in range(nblocks(a)):
        lo, hi = slice_bounds(k0, k1, a["ksplit"])[b] if split else (k0, k1)
        C0 = mat(arena, a["offC"] + b * a["bsC"], a["ldc"], m, n)
        if hi > lo:
            A = mat(arena, a["offA"] + (0 if split else b * a["bsA"]) + lo, a["lda"], m, hi - lo)
            B = mat(arena, a["offB"] + (0 if split else b * a["bsB"]) + lo, a["ldb"], n, hi - lo)
            if exact:
                assert_exact(A, B, C0 if a["beta"] else None, a["alpha"], quantum)
            P = a["alpha"] * (A @ B.T)
        else:
            P = np.zeros((m, n))
        full = C0 + P if a["beta"] else P
        mat(want, a["offC"] + b * a["bsC"], a["ldc"], m, n)[:] = full
        cm = mat(mask, a["offC"] + b * a["bsC"], a["ldc"], m, n)
        cm[:] = MUST
        if a["tri"]:
            cm[~lower] = EITHER
        if a["fa"]:
            blk = cm[:LEAF, :LEAF]
            blk[:] = np.where(lower[:LEAF, :LEAF], UNSPECIFIED if b in fa_failed else FACTOR, UNSPECIFIED)
    return want, mask


def mismatches(got, want, before, mask, args, limit=12):
    """-> (count, lines): the elements of `got` that break their class, each as one line with the class, the matrix of the
    batch (or k-slice) and the (i, j) it has relative to that C block (rows >= m or columns >= n: beside the block)"""
    a = full_args(args)
    same_bits = got.view(np.int64) == before.view(np.int64)
    bad = np.zeros(got.size, dtype=bool)
    bad |= (mask == BACKGROUND) & ~same_bits
    bad |= (mask == MUST) & ~(got == want)
    bad |= (mask == EITHER) & ~(same_bits | (got == want))
    idx = np.flatnonzero(bad)
    lines = []
    for e in idx[:limit]:
        rel = int(e) - a["offC"]
        b = min(max(rel // a["bsC"], 0), nblocks(a) - 1) if a["bsC"] > 0 else 0
        rel -= b * a["bsC"]
        lines.append(f"  {CLASS_NAMES[mask[e]]:11s} arena[{int(e)}] block {b} (i, j) = ({rel // a['ldc']}, {rel % a['ldc']}) "
                     f"got {float(got[e])!r} want {float(want[e])!r} before {float(before[e])!r}")
    return int(idx.size), lines


# ------------------------------------------------------------------ launches (arena + args)
def case_trailing(rng, m, n, K, alpha, beta, kind="int", tri=0, nbatch=0, k0=32, r=3):
    """the trailing update's layout: per matrix ONE row-major block with one leading dimension; A = rows [r, r+m) and
    B = rows [r, r+n) of its columns [k0, k1) (the same storage: A is B, the SYRK form, when m = n), C = rows [r, r+m) of
    the columns [k1, k1+n).  Columns before k0, rows before r and behind the operands hold the background."""
    k1 = k0 + K
    ld = round_up(k1 + n, 8) + 8
    rows = r + max(m, n) + 2
    nb = max(nbatch, 1)
    bs = round_up(rows * ld, 8) + 64
    lay = Layout()
    off = lay.reserve(nb * bs)
    arena = lay.arena()
    for b in range(nb):
        mat(arena, off + b * bs + r * ld + k0, ld, max(m, n), K)[:] = operand(rng, max(m, n), K, kind)
        mat(arena, off + b * bs + r * ld + k1, ld, m, n)[:] = operand(rng, m, n, kind)
    args = dict(offC=off + r * ld + k1, offA=off + r * ld, offB=off + r * ld, ldc=ld, lda=ld, ldb=ld, m=m, n=n, k0=k0, k1=k1,
                alpha=alpha, beta=beta, tri=tri, nbatch=nbatch, bsC=bs, bsA=bs, bsB=bs)
    return arena, args


def case_batch(rng, m, n, K, nbatch, tri, alpha=-1.0, beta=1, kind="int"):
    """nbatch problems with three different strides; every matrix has operands of its own"""
    lda, ldb, ldc = K + 8, K + 16, round_up(n, 8) + 8
    bsA, bsB, bsC = m * lda + 64, n * ldb + 128, m * ldc + 192
    lay = Layout()
    offA, offB, offC = lay.reserve(nbatch * bsA), lay.reserve(nbatch * bsB), lay.reserve(nbatch * bsC)
    arena = lay.arena()
    for b in range(nbatch):
        mat(arena, offA + b * bsA, lda, m, K)[:] = operand(rng, m, K, kind)
        mat(arena, offB + b * bsB, ldb, n, K)[:] = operand(rng, n, K, kind)
        mat(arena, offC + b * bsC, ldc, m, n)[:] = operand(rng, m, n, kind)
    args = dict(offC=offC, offA=offA, offB=offB, ldc=ldc, lda=lda, ldb=ldb, m=m, n=n, k0=0, k1=K, alpha=alpha, beta=beta,
                tri=tri, nbatch=nbatch, bsC=bsC, bsA=bsA, bsB=bsB)
    return arena, args


def case_corner(rng, Np, nbatch, kind="int", off=64):
    """the corner product C^-1 = U U^T: A is B = [Z^T; U], Np + off rows of Np columns, row i zero before column i - off
    (off = 64 in production)"""
    rows, lda, ldc = Np + off, Np + 8, Np + off + 8
    nb = max(nbatch, 1)
    bsA, bsC = rows * lda + 64, rows * ldc + 128
    lay = Layout()
    offA, offC = lay.reserve(nb * bsA), lay.reserve(nb * bsC)
    arena = lay.arena()
    for b in range(nb):
        mat(arena, offA + b * bsA, lda, rows, Np)[:] = kstart_operand(rng, rows, Np, off, kind)
    args = dict(offC=offC, offA=offA, offB=offA, ldc=ldc, lda=lda, ldb=lda, m=rows, n=rows, k0=0, k1=Np, alpha=1.0, beta=0,
                tri=1, kstart_mode=1, kstart_off=off, nbatch=nbatch, bsC=bsC, bsA=bsA, bsB=bsA)
    return arena, args


def case_predict(rng, m, Np, ksplit=0, kind="int", kend_off=0):
    """the prediction product: m query rows against the Np triangular rows of L^-1 (row j zero behind column j - kend_off,
    0 in production) and the 64 dense rows behind them; ldc = Np + 64, and with split-K the slices lie
    round_up(m, 64) * (Np + 64) apart"""
    n, lda, ldb, ldc = Np + 64, Np + 8, Np + 8, Np + 64
    bsC = round_up(m, 64) * ldc
    lay = Layout()
    offA, offB, offC = lay.reserve(m * lda), lay.reserve(n * ldb), lay.reserve(max(ksplit, 1) * bsC)
    arena = lay.arena()
    mat(arena, offA, lda, m, Np)[:] = operand(rng, m, Np, kind)
    mat(arena, offB, ldb, n, Np)[:] = kend_operand(rng, n, Np, kend_off, Np, kind)
    args = dict(offC=offC, offA=offA, offB=offB, ldc=ldc, lda=lda, ldb=ldb, m=m, n=n, k0=0, k1=Np, alpha=1.0, beta=0,
                kend_mode=1, kend_off=kend_off, ksplit=ksplit, bsC=bsC if ksplit > 1 else 0)
    return arena, args


FA_QUANTUM = 2.0 ** -20


def case_factor_ahead(rng, m, K, nbatch, bad_row=None, bad_matrix=None, fa_c0=128):
    """a triangular trailing update (case_trailing, A is B, alpha = -1, beta = 1) whose tile (0,0) leaves as a Cholesky
    factor.  Block (0,0) of every C is S + A0 A0^T with S = G G^T + 64 I, G standard normal, rounded to multiples of
    2**-20: the update is then exact in every order and the updated block is S itself.  bad_row (1-based) of matrix
    bad_matrix gets the diagonal element -1: its leading block stays positive definite, so that row holds the first
    non-positive pivot.  -> (arena, args, [S of every matrix])"""
    arena, args = case_trailing(rng, m, m, K, -1.0, 1, tri=1, nbatch=nbatch)
    args.update(fa=1, fa_c0=fa_c0)
    S = []
    for b in range(max(nbatch, 1)):
        G = rng.standard_normal((LEAF, LEAF))
        Sb = np.rint((G @ G.T + 64.0 * np.eye(LEAF)) / FA_QUANTUM) * FA_QUANTUM
        Sb = np.tril(Sb) + np.tril(Sb, -1).T
        if bad_row is not None and b == bad_matrix:
            Sb[bad_row - 1, bad_row - 1] = -1.0
        A0 = mat(arena, args["offA"] + b * args["bsA"] + args["k0"], args["lda"], LEAF, K)
        mat(arena, args["offC"] + b * args["bsC"], args["ldc"], LEAF, LEAF)[:] = Sb + A0 @ A0.T
        S.append(Sb)
    return arena, args, S
