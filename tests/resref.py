"""Reference for ONE launch of the kernels that read the device-resident factor (skinny_nt_kernel, gemv_tri_kernel,
loo_colsq_kernel, loo_finish_kernel, lgo_gather_kernel, lgo_stage_kernel, lgo_finish_kernel, and the chunk tail of gpemu_lgo)
through gpemu_test_resident_launch: tests/test_gpu_resident_kernels.py on the device, tests/test_resref.py on the CPU.  Test
infrastructure only; plain numpy in numpy.longdouble (x87 extended, 2^-64), no device value is produced here.

The contract these kernels share.  Above its diagonal L^-1 holds exact zeros only inside the diagonal tiles and nothing
specified further out (U = R^-T of leave-group-out likewise left of its diagonal), so the operand builders put NaN on every
element the contract says is not read, and NaN (one fixed payload, NAN_BITS) on every output before the launch.  After it
every element is UNCHANGED (the uploaded bits), VALUE (a specified value with a bar) or UNSPECIFIED, as leafref.classes has
it; a NaN in a VALUE element is a read beside the operands.

The bars.  u = 2^-53; every constant counts roundings along the longest chain that reaches the element (first order in u):

  products    Vp[s][q][n] = sum over k in slice s, k < ke(n), of Kq[q][k] L[n][k]; ke(n) = (n & ~15) + 16 for n < ntri, K
              otherwise.  Integer operands in [-8, 8]: the numpy product is the only right answer.  Mixed operands:
              (n_k + 4) u sum |Kq||L|, n_k the number of k: one rounding per fused accumulation and the merge of the four
              accumulators (the one-query kernel: at most 4 ceil(n_k / 256) fused steps per lane and 6 butterfly additions,
              which is below n_k + 4 from n_k = 16 on; n_k = 0 gives an exact zero).
  loo_colsq   part[c][j] = sum over rows r of chunk c, j <= r < N, of (L^-1)_rj^2: (n + 1) u sum x^2, n <= 64 terms, each a
              fused accumulation.
  loo_finish  P_ii = sum_c part[c][i] - w_i^T Q w_i: (nchunks + 3) u sum |part| + (2 nreg + 3) u |w|^T |Q| |w|.  The four
              quarter sums take at most ceil(len / 4) - 1 roundings, their merge 3, the subtraction 1 (u |P| <= u sum |part|);
              Q w takes nreg fused steps, w^T (Q w) at most ceil(nreg / 4), the merge 3.  var = 1 / P: |dP| / P^2 + 2 u |var|;
              mean = y - gamma / P: |gamma| |dP| / P^2 + 2 u (|gamma / P| + |y|).  Precondition, asserted: w^T Q w <= P_ii.
  lgo_gather  exact: a copy or a zero.
  lgo_stage   T - w_r^T (Q w_c): u |T| + (2 nreg + 2) u |w_r|^T |Q| |w_c| (nreg fused steps twice, one subtraction);
              everything else the kernel writes is 0, 1 or a copy of gamma: exact.
  lgo_finish  var = sum_{pos <= k < b} U[pos][k]^2, e = sum U[pos][k] w[k], mean = y - e: (b - pos + 7) u sum |terms| (the
              terms of the mean: |U||w| and |y|); werr = w[pos], maha and logdet copies: exact; logpdf = -1/2 (maha + logdet +
              b log 2 pi): 7 u (|maha| + |logdet| + b log 2 pi).
  lgo_tail    lgoref.RTOL (1e-8, the project's bar for these outputs) in lgoref.errors' measures against a longdouble Cholesky
              factor of the staged matrix, its inverse, the solved row and the log-determinant; the variance scale kappa is
              the largest variance of the group.  Precondition, asserted: 1-norm condition of the matrix <= 1e3."""
import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53
LEAF = 64
LOO_RC, LOO_SW = 64, 512                  # rows per chunk, columns per strip of loo_colsq_kernel
UNCHANGED, VALUE, UNSPECIFIED = 0, 1, 2
NAN_BITS = 0x7FF8DEAD0000BEEF             # the one NaN of every prefill: UNCHANGED is a comparison of bytes
INFO_NONE = 0x7F7F7F7F
LOG2PI = np.log(8 * np.arctan(LD(1.0)))
COND1_MAX = 1e3

# ------------------------------------------------------------------ the cases of the device test (tests/test_resref.py checks
# the references, the bars and the preconditions on every one of them without a device)
# (nslice, klen) per Np: klen = 80 is one 64-step and one 16-tail, 48 the tail loop only; at Np = 576 the one-query kernel
# makes a second trip of its 256-k stride in which only lanes 0 .. 7 hold a k.  All but (3, 80) are production's rule.
PRODUCT_SPLITS = {192: ((1, 192), (2, 96), (3, 64), (3, 80), (4, 48)), 576: ((2, 288), (3, 192))}
PRODUCT_M = (1, 2, 16)
KINDS = ("int", "mixed")
# N = 513: Np = 576, a second strip owns one chunk and 64 of its columns are pad; 517 / 520: a last chunk of 5 / 8 rows (the
# unroll of 8 with a masked row and with none); 1025: three strips
COLSQ_N = (1, 63, 64, 65, 130, 513, 517, 520, 1025)
# the same N, and 250 / 290 for four / five chunks: len = nchunks - cfirst takes 1, 2, 3, 4, 5, 9, 17; nreg: quarters of the
# 4-way split that are empty or uneven
LOO_FINISH_CASES = tuple(zip(COLSQ_N + (250, 290), (1, 3, 4, 5, 21, 63, 1, 3, 4, 5, 21)))
# (N, sizes, bp): 130 points cannot hold all of 1, 63, 64, 65, 70, 128 -- two selections, both padded to 128 -- 513 can
GATHER_CASES = ((130, (1, 128), 128), (130, (63, 65), 128), (513, (1, 63, 64, 65, 70, 128), 128))
# (N, bp, sizes, nreg, g0)
STAGE_CASES = ((130, 64, (1, 63, 64), 1, 0), (130, 64, (1, 63, 64), 17, 1), (460, 128, (65, 127, 128, 1, 64, 63), 16, 0),
               (460, 128, (65, 127, 128, 1, 64, 63), 33, 2), (460, 128, (65, 127, 128, 1, 64, 63), 63, 3))
# (N, bp, sizes, g0, info words of the chunk): one group of three carries the word 5; bp = 192 with positions >= 128, where
# the walk starts at column 128
FINISH_CASES = ((130, 64, (63, 64, 1), 0, (INFO_NONE, 5, INFO_NONE)), (130, 64, (1, 64, 63), 0, (5, INFO_NONE, INFO_NONE)),
                (650, 192, (129, 130, 191, 192), 1, (INFO_NONE, 5, INFO_NONE)), (650, 192, (191, 192, 129), 0, (INFO_NONE, 5, INFO_NONE)))
TAIL_N, TAIL_BP, TAIL_SIZES = 300, 128, (70, 128, 100)
TAIL_P = (1, 37, 65, 128)                 # the first leaf, inside a leaf, the second 64-column leaf, the last row


def round_up(x, q):
    return -(-x // q) * q


def nans(*shape):
    a = np.empty(shape, dtype=np.float64)
    a.view(np.uint64)[...] = NAN_BITS
    return a


def is_prefill(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64) == NAN_BITS


def values(rng, m, n, kind):
    """kind "int": integers in [-8, 8]; "mixed" (test_gpu_rhs_ride.make_case's): standard normal with every third column
    negative and every fifth row scaled by 1e-150"""
    if kind == "int":
        return rng.integers(-8, 9, size=(m, n)).astype(np.float64)
    assert kind == "mixed"
    v = rng.standard_normal((m, n))
    v[:, ::3] = -np.abs(v[:, ::3])
    v[::5, :] *= 1e-150
    return v


def ratio(err, bar):
    """largest err / bar; an error where the bar is zero must be zero itself; a NaN error is infinite"""
    err, bar = np.atleast_1d(np.asarray(err, dtype=LD)), np.atleast_1d(np.asarray(bar, dtype=LD))
    if np.isnan(err).any():
        return float("inf")
    z = bar == 0
    if np.any(err[z] != 0):
        return float("inf")
    return float(np.max(err[~z] / bar[~z])) if np.any(~z) else 0.0


# ------------------------------------------------------------------ the prediction products
def ke(n, ntri, K):
    return (n & ~15) + 16 if n < ntri else K


def production_klen(Np, nslice):
    """production's rule for the slice length"""
    return round_up(-(-Np // nslice), 16)


def product_case(seed, Np, M, kind, one_query=False):
    """operands of a product launch with K = ntri = Np, ntot = Np + 64 -> dict(kq (16 x ldk), lin (ntot x ld), ...).
    Triangular rows n hold values at k <= n, zeros up to the end of their diagonal 16-block and NaN beyond it; the 64 rows
    below are dense.  Kq rows >= M are zero (the one-query kernel: rows 1 .. 15 NaN); the columns beyond K are NaN."""
    rng = np.random.default_rng(seed)
    K, ntot, ldk, ld = Np, Np + LEAF, Np + 4, Np + 8
    kq, lin = nans(16, ldk), nans(ntot, ld)
    kq[:, :K] = 0.0
    kq[:M, :K] = values(rng, M, K, kind)
    if one_query:
        assert M == 1
        kq[1:] = nans(15, ldk)
    v = values(rng, ntot, K, kind)
    n, k = np.indices((ntot, K))
    tri = n < Np
    lin[:, :K] = np.where(tri & (k > n), 0.0, v)
    lin[:, :K][tri & (k >= (n & ~15) + 16)] = nans(1)[0]
    return dict(kq=kq, lin=lin, K=K, ntri=Np, ntot=ntot, ldk=ldk, ld=ld, M=M)


def product_reference(case, nslice, klen):
    """-> (want, bar): nslice x 16 x ntot in longdouble.  Row q of the one-query case beyond 0 is not meant (NaN operands)."""
    K, ntri, ntot = case["K"], case["ntri"], case["ntot"]
    A = np.asarray(case["kq"][:, :K], dtype=LD)
    B = np.asarray(case["lin"][:, :K], dtype=LD)
    want, bar = np.zeros((nslice, 16, ntot), dtype=LD), np.zeros((nslice, 16, ntot), dtype=LD)
    for s in range(nslice):
        lo = min(K, s * klen)
        for n0 in range(0, ntot, 16):
            hi = min(K, lo + klen, ke(n0, ntri, K))
            if hi <= lo:
                continue
            a, b = A[:, lo:hi], B[n0:n0 + 16, lo:hi]
            want[s, :, n0:n0 + 16] = a @ b.T
            bar[s, :, n0:n0 + 16] = (hi - lo + 4) * U * (np.abs(a) @ np.abs(b).T)
    return want, bar


def product_classes(nslice, vrows, ldv, ntot, one_query):
    cls = np.zeros((nslice, vrows, ldv), dtype=np.int8)
    cls[:, :(1 if one_query else 16), :ntot] = VALUE
    return cls


# ------------------------------------------------------------------ leave-one-out
def nchunks_of(N):
    return -(-N // LOO_RC)


def launched(N, Np):
    """nchunks x Np mask of the (chunk, column) pairs loo_colsq_kernel is launched for: chunk >= 8 * strip"""
    c, j = np.indices((nchunks_of(N), Np))
    return c >= (j // LOO_SW) * (LOO_SW // LOO_RC)


def linv_case(seed, N, extra_rows=0, kind="normal"):
    """LinvAug with rows [0, Np) = a lower triangular N x N block of values and NaN everywhere else: strictly above the
    diagonal (the diagonal tiles included), the pad rows and columns N .. Np, the columns Np .. ld.  extra_rows more rows
    (gamma, W^T) of NaN under it.  -> (lin (Np + extra_rows) x ld, Np, ld)"""
    rng = np.random.default_rng(seed)
    Np = round_up(N, LEAF)
    ld = Np + 6
    lin = nans(Np + extra_rows, ld)
    v = rng.standard_normal((N, N))
    v[:, ::3] *= 1e-3                      # column sums of very different sizes
    r, c = np.indices((N, N))
    lin[:N, :N][r >= c] = v[r >= c]
    return lin, Np, ld


def colsq_reference(lin, N, Np):
    """-> (want, bar, cls): nchunks x Np"""
    nch = nchunks_of(N)
    X = np.zeros((nch * LOO_RC, Np), dtype=LD)
    X[:N, :N] = np.tril(np.asarray(lin[:N, :N], dtype=LD))           # (NaN above the diagonal: tril drops it)
    cnt = np.zeros((nch * LOO_RC, Np), dtype=LD)
    cnt[:N, :N] = np.tril(np.ones((N, N)))
    X2 = (X * X).reshape(nch, LOO_RC, Np)
    want = X2.sum(axis=1)
    n = cnt.reshape(nch, LOO_RC, Np).sum(axis=1)
    bar = (n + 1) * U * want
    return want, bar, np.where(launched(N, Np), VALUE, UNCHANGED).astype(np.int8)


def loo_finish_case(seed, N, nreg):
    """operands of a loo_finish launch: positive partials of mixed size at the launched pairs (NaN at the others), gamma and
    W^T rows under an all-NaN L^-1, beta then Q with Q symmetric positive definite and scaled so that |w|^T |Q| |w| is at
    most half the column's sum of partials -> dict"""
    rng = np.random.default_rng(seed)
    Np, nch = round_up(N, LEAF), nchunks_of(N)
    ld = Np + 6
    part = nans(nch, Np)
    m = launched(N, Np)
    part[m] = (rng.uniform(0.1, 1.0, size=(nch, Np)) * 10.0 ** rng.integers(-3, 3, size=(nch, Np)))[m]
    lin = nans(Np + 1 + nreg, ld)
    gamma, W = rng.standard_normal(N), rng.standard_normal((N, nreg))
    lin[Np, :N] = gamma
    lin[Np + 1:, :N] = W.T
    G = rng.standard_normal((nreg, nreg))
    Q = G @ G.T / nreg + np.eye(nreg)
    psum = np.where(m, part, 0.0).sum(axis=0)[:N]
    scale = np.min(0.5 * psum / np.einsum("ia,ab,ib->i", np.abs(W), np.abs(Q), np.abs(W)))
    Q *= scale * (1.0 - 1e-9)
    betaq = np.concatenate([nans(nreg), Q.ravel()])                   # (beta is not read by the kernel)
    y = rng.standard_normal(N) + 1.0
    return dict(part=part, lin=lin, betaq=betaq, y=y, N=N, Np=Np, ld=ld, nreg=nreg)


def loo_finish_reference(part, gamma, W, Q, y, N, Np):
    """part nchunks x Np (only launched pairs are read), W N x nreg -> dict(mean, var, bar_mean, bar_var, pii, reg)"""
    nch = nchunks_of(N)
    m = launched(N, Np)[:, :N]
    p = np.where(m, np.asarray(part, dtype=LD)[:, :N], LD(0))
    W, Q, gamma, y = (np.asarray(a, dtype=LD) for a in (W, Q, gamma, y))
    nreg = W.shape[1]
    sq = p.sum(axis=0)
    reg = np.einsum("ia,ab,ib->i", W, Q, W)
    areg = np.einsum("ia,ab,ib->i", np.abs(W), np.abs(Q), np.abs(W))
    pii = sq - reg
    assert np.all(reg <= pii), "precondition: w^T Q w <= P_ii"
    dP = (nch + 3) * U * np.abs(p).sum(axis=0) + (2 * nreg + 3) * U * areg
    var, mean = 1 / pii, y - gamma / pii
    return dict(mean=mean, var=var, pii=pii, reg=reg, bar_var=dP / pii ** 2 + 2 * U * np.abs(var),
                bar_mean=np.abs(gamma) * dP / pii ** 2 + 2 * U * (np.abs(gamma / pii) + np.abs(y)))


# ------------------------------------------------------------------ leave-group-out
def group_tables(N, sizes, seed, bp=None):
    """groups of the given sizes, their members interleaved in design order (a seeded permutation; the points left over carry
    the label -1) -> dict(group, colrow, members, moff, bsize, bp, groups), the tables as gpemu_lgo builds them"""
    assert sum(sizes) <= N
    perm = np.random.default_rng(seed).permutation(N)
    group = np.full(N, -1, dtype=np.int32)
    o = 0
    for g, b in enumerate(sizes):
        group[perm[o:o + b]] = g
        o += b
    bp = round_up(max(sizes), LEAF) if bp is None else bp
    groups = [np.flatnonzero(group == g).astype(np.int32) for g in range(len(sizes))]
    colrow = np.full(N, -1, dtype=np.int32)
    for g, B in enumerate(groups):
        colrow[B] = g * bp + np.arange(len(B))
    moff = np.cumsum([0] + [len(B) for B in groups[:-1]]).astype(np.int32)
    return dict(group=group, colrow=colrow, members=np.concatenate(groups), moff=moff, bsize=np.array(sizes, dtype=np.int32), bp=bp,
                groups=groups)


def gather_reference(linv, N, Np, tab, g0, nbc):
    """linv: the N x N block (only j <= k is read) -> Z (nbc * bp) x Np, every element VALUE and exact"""
    bp = tab["bp"]
    Lt = np.tril(np.where(np.tril(np.ones((N, N), dtype=bool)), linv[:N, :N], 0.0))
    Z = np.zeros((nbc * bp, Np))
    for g in range(g0, g0 + nbc):
        B = tab["groups"][g]
        Z[(g - g0) * bp:(g - g0) * bp + len(B), :N] = Lt[:, B].T
    return Z


def tall_rows(bp):
    return 2 * bp + LEAF


def lower_tiles(bp):
    """bp x bp mask of the 64 x 64 tiles at or below the diagonal"""
    r, c = np.indices((bp, bp))
    return c // LEAF <= r // LEAF


def stage_case(seed, N, bp, sizes, nreg, g0):
    """operands of a staging launch for the groups g0 .. of `sizes`: tall matrices with values where both positions are
    members, in the lower tiles, and NaN elsewhere (pad, upper tiles, the rows from bp on); gamma and W^T rows; beta, Q"""
    rng = np.random.default_rng(seed)
    tab = group_tables(N, sizes, seed + 1, bp)
    Np, nbc = round_up(N, LEAF), len(sizes) - g0
    ld, tstride = Np + 2, tall_rows(bp) * bp + 10
    t = nans(nbc * tstride)
    low = lower_tiles(bp)
    for g in range(nbc):
        b = sizes[g0 + g]
        M = t[g * tstride:g * tstride + bp * bp].reshape(bp, bp)
        v = rng.standard_normal((bp, bp))
        r, c = np.indices((bp, bp))
        m = low & (r < b) & (c < b)
        M[m] = v[m]
    lin = nans(Np + 1 + nreg, ld)
    lin[Np, :N] = rng.standard_normal(N)
    lin[Np + 1:, :N] = values(rng, nreg, N, "mixed") if nreg > 1 else rng.standard_normal((1, N))
    Q = rng.standard_normal((nreg, nreg))
    betaq = np.concatenate([nans(nreg), Q.ravel()])
    return dict(t=t, lin=lin, betaq=betaq, tab=tab, N=N, Np=Np, ld=ld, bp=bp, nbc=nbc, g0=g0, nreg=nreg, tstride=tstride)


def stage_reference(case):
    """-> (want, bar, cls) over the whole t region, want and bar in longdouble (bar 0: exact)"""
    bp, nbc, g0, Np, N, nreg, ts = (case[k] for k in ("bp", "nbc", "g0", "Np", "N", "nreg", "tstride"))
    t0 = case["t"]
    want, bar = np.asarray(t0, dtype=LD).copy(), np.zeros(t0.size, dtype=LD)
    cls = np.zeros(t0.size, dtype=np.int8)
    gamma = case["lin"][Np, :N]
    W = np.asarray(case["lin"][Np + 1:, :N].T, dtype=LD)
    Q = np.asarray(case["betaq"][nreg:].reshape(nreg, nreg), dtype=LD)
    low = lower_tiles(bp)
    r, c = np.indices((bp, bp))
    for g in range(nbc):
        B = case["tab"]["groups"][g0 + g]
        b = len(B)
        M = np.where(r == c, LD(1), LD(0))
        E = np.zeros((bp, bp), dtype=LD)
        T = np.asarray(t0[g * ts:g * ts + bp * bp].reshape(bp, bp)[:b, :b], dtype=LD)
        M[:b, :b] = T - W[B] @ (Q @ W[B].T)
        E[:b, :b] = U * np.abs(T) + (2 * nreg + 2) * U * (np.abs(W[B]) @ (np.abs(Q) @ np.abs(W[B]).T))
        sl = slice(g * ts, g * ts + bp * bp)
        want[sl] = np.where(low, M, want[sl].reshape(bp, bp)).ravel()
        bar[sl] = np.where(low, E, 0).ravel()
        cls[sl] = np.where(low, VALUE, UNCHANGED).ravel()
        rest = np.zeros((bp + LEAF, bp), dtype=LD)
        rest[0, :b] = gamma[B]
        rest[LEAF:] = np.eye(bp)
        want[g * ts + bp * bp:g * ts + tall_rows(bp) * bp] = rest.ravel()
        cls[g * ts + bp * bp:g * ts + tall_rows(bp) * bp] = VALUE
    return want, bar, cls


def finish_case(seed, N, bp, sizes, g0, words):
    """operands of a finishing launch for the groups g0 .. of `sizes`: per group the solved row w (values at k < b) and the rows
    of U (values at pos <= k < b, pos < b); NaN everywhere else in the tall matrices.  words: the chunk's info words."""
    rng = np.random.default_rng(seed)
    tab = group_tables(N, sizes, seed + 1, bp)
    nbc = len(sizes) - g0
    tstride = tall_rows(bp) * bp + 10
    t = nans(nbc * tstride)
    for g in range(nbc):
        b = sizes[g0 + g]
        M = t[g * tstride:g * tstride + tall_rows(bp) * bp].reshape(tall_rows(bp), bp)
        M[bp, :b] = rng.standard_normal(b)
        Um = M[bp + LEAF:]
        r, c = np.indices((bp, bp))
        m = (r < b) & (c < b) & (c >= r)
        Um[m] = (rng.standard_normal((bp, bp)) * 10.0 ** rng.integers(-2, 2, size=(bp, 1)))[m]
    res = rng.uniform(0.5, 50.0, size=2 * nbc) * np.where(np.arange(2 * nbc) % 2, -1.0, 1.0)
    y = rng.standard_normal(N) + 1.0
    return dict(t=t, res=res, y=y, tab=tab, N=N, bp=bp, nbc=nbc, g0=g0, tstride=tstride, info=np.array(words, dtype=np.int32),
                ngroups=len(sizes))


def finish_reference(case):
    """-> dict of (want, bar, cls) for mean, var, werr (N each), stat (3 x ngroups) and info_out (want, cls); a group whose
    info word is below INFO_NONE wants NaN everywhere and its word"""
    N, bp, nbc, g0, ts, G = (case[k] for k in ("N", "bp", "nbc", "g0", "tstride", "ngroups"))
    out = {k: [np.zeros(N, dtype=LD), np.zeros(N, dtype=LD), np.zeros(N, dtype=np.int8)] for k in ("mean", "var", "werr")}
    stat = [np.zeros((3, G), dtype=LD), np.zeros((3, G), dtype=LD), np.zeros((3, G), dtype=np.int8)]
    info = [np.zeros(G, dtype=np.int32), np.zeros(G, dtype=np.int8)]
    y = np.asarray(case["y"], dtype=LD)
    for g in range(nbc):
        B = case["tab"]["groups"][g0 + g]
        b = len(B)
        M = np.asarray(case["t"][g * ts:g * ts + tall_rows(bp) * bp].reshape(tall_rows(bp), bp), dtype=LD)
        w, Um = M[bp, :b], np.triu(np.where(np.triu(np.ones((b, b), dtype=bool)), M[bp + LEAF:bp + LEAF + b, :b], LD(0)))
        word = int(case["info"][g])
        bad = word < INFO_NONE
        depth = (b - np.arange(b) + 7) * U
        maha, logdet = LD(case["res"][2 * g]), -LD(case["res"][2 * g + 1])
        vals = dict(var=((Um * Um).sum(axis=1), depth * (Um * Um).sum(axis=1)),
                    mean=(y[B] - Um @ w, depth * (np.abs(Um) @ np.abs(w) + np.abs(y[B]))), werr=(w, np.zeros(b, dtype=LD)))
        for k, (v, e) in vals.items():
            out[k][0][B], out[k][1][B], out[k][2][B] = (LD("nan") if bad else v), e, VALUE
        s = np.array([maha, logdet, -(maha + logdet + b * LOG2PI) / 2], dtype=LD)
        stat[0][:, g0 + g] = LD("nan") if bad else s
        stat[1][:, g0 + g] = [0, 0, 7 * U * (abs(maha) + abs(logdet) + b * LOG2PI)]
        stat[2][:, g0 + g] = VALUE
        info[0][g0 + g], info[1][g0 + g] = (word if bad else 0), VALUE
    out["stat"], out["info_out"] = stat, info
    return out


# ------------------------------------------------------------------ the chunk tail
def cholesky_ld(A):
    """lower Cholesky factor in longdouble; -> (R, p): p = 0, or the 1-based row of the first pivot <= 0"""
    A = np.asarray(A, dtype=LD).copy()
    n = A.shape[0]
    R = np.zeros((n, n), dtype=LD)
    for j in range(n):
        d = A[j, j] - R[j, :j] @ R[j, :j]
        if not d > 0:
            return R, j + 1
        R[j, j] = np.sqrt(d)
        R[j + 1:, j] = (A[j + 1:, j] - R[j + 1:, :j] @ R[j, :j]) / R[j, j]
    return R, 0


def tri_inverse_ld(R):
    """inverse of a lower triangular matrix in longdouble, by columns"""
    n = R.shape[0]
    X = np.zeros((n, n), dtype=LD)
    for i in range(n):
        X[i, i] = 1 / R[i, i]
        X[i, :i] = -(R[i, :i] @ X[:i, :i]) / R[i, i]
    return X


def spd(seed, b):
    """a symmetric positive definite b x b matrix of 1-norm condition well below COND1_MAX"""
    G = np.random.default_rng(seed).standard_normal((b, b))
    A = G @ G.T / b + np.eye(b)
    return 0.5 * (A + A.T)


def make_indefinite(A, p):
    """twice the largest diagonal entry off element (p, p), p 1-based: the leading p - 1 rows stay positive definite and the
    pivot of row p is negative by more than that entry"""
    A = A.copy()
    A[p - 1, p - 1] -= 2.0 * np.max(np.diag(A))
    return A


def tail_case(seed, N, bp, sizes, mats):
    """staged tall matrices as lgo_stage_kernel leaves them, from the caller's b x b matrices `mats` (one per group): the
    matrix in the lower tiles with the identity at the pad, NaN in the tiles above the diagonal, row bp = gamma at the
    members, 63 zero rows, the identity rows"""
    rng = np.random.default_rng(seed)
    tab = group_tables(N, sizes, seed + 1, bp)
    nbc, tstride = len(sizes), tall_rows(bp) * bp
    t = nans(nbc * tstride)
    gamma, y = rng.standard_normal(N), rng.standard_normal(N) + 1.0
    low = lower_tiles(bp)
    for g, (b, A) in enumerate(zip(sizes, mats)):
        M = t[g * tstride:(g + 1) * tstride].reshape(tall_rows(bp), bp)
        P = np.eye(bp)
        P[:b, :b] = A
        M[:bp][low] = P[low]
        M[bp:] = 0.0
        M[bp, :b] = gamma[tab["groups"][g]]
        M[bp + LEAF:] = np.eye(bp)
    return dict(t=t, y=y, gamma=gamma, tab=tab, N=N, bp=bp, nbc=nbc, tstride=tstride, mats=mats, ngroups=nbc)


def tail_reference(case, g):
    """group g of a tail case from the longdouble factor of its matrix -> (dict(mean, var, werr, maha, logdet, logpdf) in
    float64, kappa = the largest variance, cond1), or (None, None, p) when the pivot of row p fails"""
    B = case["tab"]["groups"][g]
    A = np.asarray(case["mats"][g], dtype=LD)
    R, p = cholesky_ld(A)
    if p:
        return None, None, p
    Ri = tri_inverse_ld(R)
    cov = Ri.T @ Ri
    cond1 = float(np.max(np.abs(A).sum(axis=0)) * np.max(np.abs(cov).sum(axis=0)))
    assert cond1 <= COND1_MAX, ("ill-conditioned test input", cond1)
    gam, y = np.asarray(case["gamma"][B], dtype=LD), np.asarray(case["y"][B], dtype=LD)
    w = Ri @ gam
    maha, logdet = w @ w, -2 * np.sum(np.log(np.diag(R)))
    ref = dict(mean=y - cov @ gam, var=np.diag(cov), werr=w, maha=maha, logdet=logdet, logpdf=-(maha + logdet + len(B) * LOG2PI) / 2)
    ref = {k: np.asarray(v, dtype=np.float64) if np.ndim(v) else float(v) for k, v in ref.items()}
    return ref, float(np.max(ref["var"])), cond1
