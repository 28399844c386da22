"""Every prediction regime of gpemu_predict_batch_dev, and ragged sizes at baseline scale, against LAPACK.

Part A.  gpemu_predict_batch_dev (madaiemulator_amd/csrc/hip/gpemu_api.hip, from PRED_SPLIT_MAX on) runs each block of
<= 16 384 queries through one of five kernel chains, chosen from the block's query count and Np (N rounded up to 64):
one query (gemv_tri_kernel), few queries (skinny_nt_kernel), split-K GEMM, unsplit GEMM, and unsplit on 128x128 tiles
(split_rhs_rows).  `dispatch` below restates that choice; REGIMES is its table for every (N, M) the tests run.  Each model
gets one host reference for a pool of queries (`predict_reference`: the oracle's covariance matrix, k-vectors and H,
LAPACK's Cholesky factor and solves), and every device call predicts a prefix of that pool, up the ladder of query counts
and down again on the same context.

Part B.  Likelihood and value+gradient batches at N = 8191 / 8193 (one padding row; 63 padding rows, a lone 64-column
leaf at the end of the outer panel, half-empty 128x128 tile rows) and N = 4097, every element against LAPACK.

Every model asserts its own preconditions before it compares anything: the LAPACK 1-norm condition estimate (dpocon)
<= 5e6, no k-vector entry within 1e-12 (relative) of the 1e-10 clamp (the device's exp may differ from libm's in the
last bit, which must not flip an entry between 0 and non-zero), and queries that are either exact training points or
more than 1e-6 from every one.  The reference half runs without a device; its self-check against the oracle's own
emulate_point is a CPU test."""
import time

import numpy as np
import pytest
import scipy.linalg as sl
from scipy.spatial.distance import cdist

from madaiemulator_amd import abi, synth
from oracle import oracle as O
from test_gpu_batch_elements import factor, grad_chunk_size, lik_errors, likelihood_references, same_bits

RTOL = 1e-8              # the north_star parity bar
XRTOL = 1e-11            # the same query in two regimes (other k-vector form, other summation order)
COND_MAX = 5e6           # test_randomised_parity_sweep's threshold for the plain bar
CLAMP = 1e-10            # makeKVector_fnptr's clamp (emulator.c:588-590)
SEED_C3 = 20261003 + 2   # bench.py's design seed (region A)
FAR = 5                  # pool position of the far query (every coordinate 30)
TRAIN_AT = (0, 15, 16, 63, 64, 1024, 16383, 16384, 16399)     # pool positions of exact training points

LADDER = (1, 2, 5, 15, 16, 17, 63, 64, 65, 129, 700, 1024, 1025, 1500)
SECOND_BLOCK = (16384, 16385, 16400, 16401)


# ------------------------------------------------------------------ the dispatch, restated
def dispatch(N, M):
    """the blocks of one gpemu_predict_batch_dev call -> [(regime, nslice), ...] (gpemu_api.hip, gpemu_predict_batch_dev:
    blocks of cap = min(16384, M rounded up to 64); nslice from the 64x64 tile count; `few` = mb <= 16 and nslice > 1, with
    gemv_tri for mb == 1; otherwise choose_gemm_cfg (kernels_linalg.hip) for one matrix: 128x128 tiles once the product
    has 2 x 1024 of them, and then split_rhs_rows)"""
    Np, Rp = -(-N // 64) * 64, 64
    cap = min(16384, -(-M // 64) * 64)
    out = []
    for q0 in range(0, M, cap):
        mb = min(cap, M - q0)
        mbp = -(-mb // 64) * 64
        tiles = (mbp // 64) * ((Np + Rp + 63) // 64)
        nslice = 1
        if tiles < 1024:
            nslice = max(1, min(min(16, Np // 512), 2048 // tiles))
        if nslice * mbp > 128 * 16:
            nslice = 1                                        # capacity of dV for the partial products
        if mb <= 16 and nslice > 1:
            out.append(("one" if mb == 1 else "few", nslice))
        elif nslice > 1:
            out.append(("splitk", nslice))
        else:
            big = -(-mb // 128) * -(-(Np + Rp) // 128) >= 2 * 1024
            out.append(("big" if big else "unsplit", 1))
    return out


# (N, M) -> the blocks' (regime, nslice).  one: kvec_small_kernel, gemv_tri_kernel<1>, sum_slices_kernel,
# predict_finish_small_kernel; few: the same with skinny_nt_kernel<1>; splitk: Gram or difference k-vectors, gemm_nt_kernel
# with ksplit, sum_slices_kernel, predict_finish_kernel; unsplit: the same without ksplit; big: unsplit on 128x128 tiles for
# the Np triangular columns and 64x64 tiles for the 64 gamma / W^T columns
_R1025 = {1: [("one", 2)], 2: [("few", 2)], 5: [("few", 2)], 15: [("few", 2)], 16: [("few", 2)], 17: [("splitk", 2)],
          63: [("splitk", 2)], 64: [("splitk", 2)], 65: [("splitk", 2)], 129: [("splitk", 2)], 700: [("splitk", 2)],
          1024: [("splitk", 2)], 1025: [("unsplit", 1)], 1500: [("unsplit", 1)]}
_R4097 = {1: [("one", 8)], 2: [("few", 8)], 5: [("few", 8)], 15: [("few", 8)], 16: [("few", 8)], 17: [("splitk", 8)],
          63: [("splitk", 8)], 64: [("splitk", 8)], 65: [("splitk", 8)], 129: [("splitk", 8)], 700: [("splitk", 2)],
          1024: [("unsplit", 1)], 1025: [("unsplit", 1)], 1500: [("unsplit", 1)], 16384: [("big", 1)],
          16385: [("big", 1), ("one", 8)], 16400: [("big", 1), ("few", 8)], 16401: [("big", 1), ("splitk", 8)]}
_R8193 = {1: [("one", 15)], 2: [("few", 15)], 5: [("few", 15)], 15: [("few", 15)], 16: [("few", 15)], 17: [("splitk", 15)],
          63: [("splitk", 15)], 64: [("splitk", 15)], 65: [("splitk", 7)], 129: [("splitk", 5)], 700: [("unsplit", 1)],
          1024: [("unsplit", 1)], 1025: [("unsplit", 1)], 1500: [("unsplit", 1)]}
REGIMES = {**{(1025, M): r for M, r in _R1025.items()}, **{(4097, M): r for M, r in _R4097.items()},
           **{(8193, M): r for M, r in _R8193.items()}}


# ------------------------------------------------------------------ reference half (host only)
ROOT3, ROOT5 = 1.732050808, 2.236067978     # the literal constants of emulator.c:359 / :452, as the oracle uses them


def unclamped_kvectors(kind, X, th, Xq):
    """cov(x_i, x*_q) without the clamp and without the nugget (only to measure the distance to the clamp)"""
    if kind == 1:
        r = np.exp(th[2:2 + X.shape[1]])
        return np.exp(th[0]) * np.exp(-0.5 * cdist(Xq / r, X / r, "sqeuclidean"))
    t = cdist(Xq, X) / np.exp(th[2])
    if kind == 2:
        return th[0] * (1.0 + ROOT3 * t) * np.exp(-ROOT3 * t)
    return th[0] * (1.0 + ROOT5 * t + (5.0 / 3.0) * t * t) * np.exp(-ROOT5 * t)


def check_queries(kind, X, th, Xq, chunk=2048):
    """the preconditions on the queries: exact training point or > 1e-6 from every one; no k-vector entry within 1e-12
    (relative) of the clamp.  -> the smallest relative distance of an entry to the clamp"""
    margin = np.inf
    for a in range(0, Xq.shape[0], chunk):
        Q = Xq[a:a + chunk]
        dmin = cdist(Q, X).min(axis=1)
        exact = dmin == 0.0
        assert np.all(exact | (dmin > 1e-6)), np.flatnonzero(~exact & (dmin <= 1e-6))
        Ku = unclamped_kvectors(kind, X, th, Q)
        margin = min(margin, float(np.min(np.abs(Ku / CLAMP - 1.0))))
    assert margin > 1e-12, margin
    return margin


def predict_reference(kind, order, X, y, th, Xq, keep_factor=False):
    """emulate_point (emulator_struct.c:124-143) at the rows of Xq for any covariance function: mean = h.beta +
    k.C^-1 (y - H beta), var = kappa - k.C^-1 k + q.(H^T C^-1 H)^-1 q, q = h - H^T C^-1 k, kappa = cov(x*, x*) (nugget in).
    C, k and H are the oracle's (O.cov_matrix, O.kvector with its clamp and nugget rule, O.hmatrix); the factor and solves
    are LAPACK's.  Asserts cond_1 <= COND_MAX.  -> dict(mean, var, kappa, cond[, cf])"""
    cf, cond = factor(O.cov_matrix(kind, X, th))
    assert cond <= COND_MAX, (kind, order, cond)
    H = O.hmatrix(order, X)
    AyH = sl.cho_solve(cf, np.column_stack([y, H]), check_finite=False)
    Ay, AH = AyH[:, 0], AyH[:, 1:]
    HAH = H.T @ AH
    beta = np.linalg.solve(HAH, H.T @ Ay)
    gamma = Ay - AH @ beta
    M = Xq.shape[0]
    mean, var = np.empty(M), np.empty(M)
    kappa = O.cov(kind, Xq[0], Xq[0], th)
    for a in range(0, M, 4096):                               # k-vectors in blocks: 16 401 x 4097 doubles would be 0.5 GB
        Q = Xq[a:a + 4096]
        K = np.vstack([O.kvector(kind, X, x, th) for x in Q])
        hq = O.hmatrix(order, Q)
        mean[a:a + 4096] = hq @ beta + K @ gamma
        AK = sl.cho_solve(cf, K.T, check_finite=False)
        q = hq - K @ AH
        var[a:a + 4096] = kappa - np.einsum("qi,iq->q", K, AK) + np.einsum("qa,qa->q", q, np.linalg.solve(HAH, q.T).T)
    out = dict(mean=mean, var=var, kappa=kappa, cond=cond)
    if keep_factor:
        out["cf"] = cf
    return out


def query_pool(X, P, seed):
    """synth.queries with exact training points at TRAIN_AT and one far query (every coordinate 30) at FAR"""
    Q = synth.queries(P, X.shape[1], seed)
    for j, pos in enumerate(TRAIN_AT):
        if pos < P:
            Q[pos] = X[(97 * j + 11) % X.shape[0]]
    Q[FAR] = 30.0
    return Q


def error_scales(ref):
    """per-query scales of the bars: max(1, max |mean|) and kappa for the ordinary queries; the far query's own size for
    the far query, whose mean h.beta and variance kappa + h.(H^T C^-1 H)^-1 h grow with |h| (up to 30^3 per entry)"""
    m, v, kappa = ref["mean"], ref["var"], ref["kappa"]
    ordinary = np.ones(m.size, bool)
    ordinary[FAR] = False
    sm = np.full(m.size, max(1.0, float(np.max(np.abs(m[ordinary])))))
    sv = np.full(m.size, kappa)
    sm[FAR] = max(1.0, abs(m[FAR]))
    sv[FAR] = max(kappa, abs(v[FAR]))
    return sm, sv


def model_reference(kind, order, X, y, th, Q, keep_factor=False):
    margin = check_queries(kind, X, th, Q)
    ref = predict_reference(kind, order, X, y, th, Q, keep_factor)
    ref["margin"] = margin
    ref["sm"], ref["sv"] = error_scales(ref)
    return ref


# ------------------------------------------------------------------ CPU: the reference against the oracle
@pytest.mark.parametrize("d", (3, 8))
@pytest.mark.parametrize("kind", (1, 2, 3))
def test_predict_reference_against_the_oracle_emulator(kind, d):
    """predict_reference (LAPACK) against O.Emulator.emulate (the oracle's own Cholesky, explicit inverse and
    emulate_point) at N = 300, orders 0-3, with training-point and far queries, to 1e-12 of the bars' scales.  The oracle's
    explicit inverse carries about cond * 1e-16: at d = 3 the design is dense enough that the default nugget gives
    cond_1 ~ 5e4, so those models take a larger one (e^-2.5 / 0.05) and assert cond_1 <= 2e4."""
    X, y = synth.design(300, d, 5 + d)
    Q = query_pool(X, 80, 6 + d)
    th = synth.default_thetas(kind, d)
    if d == 3:
        th[1] = -2.5 if kind == 1 else 0.05
    worst = 0.0
    for order in range(4):
        ref = model_reference(kind, order, X, y, th, Q)
        assert ref["cond"] <= 2e4, ref["cond"]
        assert ref["kappa"] == (np.exp(th[0]) + np.exp(th[1]) if kind == 1 else th[0] + th[1])
        mo, vo, st = O.Emulator(kind, order, X, y, th).emulate(Q)
        assert st == 0
        em = np.max(np.abs(ref["mean"] - mo) / ref["sm"])
        ev = np.max(np.abs(ref["var"] - vo) / ref["sv"])
        worst = max(worst, em, ev)
        assert em < 1e-12 and ev < 1e-12, (order, em, ev)
        assert np.all(np.abs(ref["var"][list(p for p in TRAIN_AT if p < 80)]) < 1e-10 * ref["kappa"])   # training points
    print(f"\nkind {kind} d={d}: worst {worst:.1e}")


def test_dispatch_table():
    """REGIMES is what `dispatch` (the code's choice, restated) gives; every regime is in it, at every N"""
    for (N, M), r in REGIMES.items():
        assert dispatch(N, M) == r, (N, M, dispatch(N, M), r)
    for N in (1025, 4097, 8193):
        seen = {b[0] for (n, M), r in REGIMES.items() if n == N for b in r}
        assert {"one", "few", "splitk", "unsplit"} <= seen, (N, seen)
    assert dispatch(4097, 16384) == [("big", 1)]


# ------------------------------------------------------------------ device half, part A
def run_ladder(c, Q, Ms):
    """every M of Ms ascending, then descending, on one context -> (up, down): {M: (mean, var)}"""
    up = {M: c.predict(Q[:M]) for M in Ms}
    down = {M: c.predict(Q[:M]) for M in reversed(Ms)}
    return up, down


def _bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def check_ladder(N, ref, up, down):
    """the bars per call, bits between calls, agreement across regimes -> worst error against the reference"""
    Ms = sorted(up)
    worst = 0.0
    for M in Ms:
        m, v = up[M]
        assert np.all(np.isfinite(m)) and np.all(np.isfinite(v)), M
        em = np.abs(m - ref["mean"][:M]) / ref["sm"][:M]
        ev = np.abs(v - ref["var"][:M]) / ref["sv"][:M]
        worst = max(worst, float(em.max()), float(ev.max()))
        assert em.max() <= RTOL and ev.max() <= RTOL, (N, M, REGIMES[(N, M)], em.max(), int(em.argmax()), ev.max(), int(ev.argmax()))
        assert _bits(up[M], down[M]), (N, M)                   # the same call again, after larger and smaller ones
    # same regime and nslice: the same query gives the same bits whatever M
    for a, b in ((2, 16), (17, 64), (65, 129)):
        if REGIMES[(N, a)] == REGIMES[(N, b)]:
            assert _bits(up[a], (up[b][0][:a], up[b][1][:a])), (N, a, b)
    # across regimes: every call against the largest ladder call (unsplit) on their common queries
    top = max(M for M in Ms if M <= 1500)
    for M in Ms:
        n = min(M, top)
        dm = np.abs(up[M][0][:n] - up[top][0][:n]) / ref["sm"][:n]
        dv = np.abs(up[M][1][:n] - up[top][1][:n]) / ref["sv"][:n]
        assert dm.max() <= XRTOL and dv.max() <= XRTOL, (N, M, REGIMES[(N, M)], dm.max(), dv.max())
    return worst


N1025_MODELS = [(kind, order, 8) for kind in (1, 2, 3) for order in range(4)] + [(1, 3, 16), (1, 2, 31)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,order,d", N1025_MODELS)
def test_n1025_every_regime(kind, order, d):
    """N = 1025 (Np = 1088, nslice 2; the capacity fallback nslice * mbp > 2048 -> unsplit from M = 1025 on): the ladder
    up and down for every covariance function and regression order 0-3 at d = 8, plus pow-exp at d = 16, order 3 (nreg 49)
    and d = 31, order 2 (nreg 63: the last slot of predict_finish_small_kernel's tail[64]; long length scales as in
    test_maximum_dimensions)"""
    t0 = time.time()
    N = 1025
    X, y = synth.design(N, d, 4100 + 10 * kind + order + d)
    th = synth.default_thetas(kind, d)
    if d == 31:
        th[2:] = np.log(2.0)
    Q = query_pool(X, 1500, 77 + d)
    ref = model_reference(kind, order, X, y, th, Q)
    c = abi.Context(0)
    try:
        c.set_model(kind, order, X, y)
        _, rc = c.predict_setup(th)
        assert rc == 0
        up, down = run_ladder(c, Q, LADDER)
    finally:
        c.close()
    worst = check_ladder(N, ref, up, down)
    print(f"\nN={N} kind {kind} order {order} d={d}: worst {worst:.2e} (cond_1 {ref['cond']:.2e}, clamp margin "
          f"{ref['margin']:.1e}), {time.time() - t0:.1f} s")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", (1, 2, 3))
def test_n4097_every_regime_and_second_blocks(kind):
    """N = 4097 (Np = 4160: nslice 8, klen 528 = 33 x 16, so the skinny kernel's 64-k loop leaves a 16-k tail), d = 8,
    order 1, a pool of 16 401 queries: the ladder and 16384 (128x128 tiles: 32 full tile columns and a half one), 16385,
    16400, 16401 (a second block of 1, 16, 17 queries: one-query, few-query, split-K).  The second blocks carry the bits of
    the same queries predicted alone; gpemu_get_cinverse against the LAPACK inverse."""
    t0 = time.time()
    N, d, order = 4097, 8, 1
    X, y = synth.design(N, d, 4097 + kind)
    th = synth.default_thetas(kind, d)
    Q = query_pool(X, 16401, 1234 + kind)
    ref = model_reference(kind, order, X, y, th, Q, keep_factor=True)
    Ainv = sl.cho_solve(ref.pop("cf"), np.eye(N), check_finite=False)
    c = abi.Context(0)
    try:
        c.set_model(kind, order, X, y)
        _, rc = c.predict_setup(th)
        assert rc == 0
        up, down = run_ladder(c, Q, LADDER + SECOND_BLOCK)
        alone = {n: c.predict(Q[16384:16384 + n]) for n in (1, 16, 17)}
        Ai = c.cinverse()
    finally:
        c.close()
    worst = check_ladder(N, ref, up, down)
    for M, n in ((16385, 1), (16400, 16), (16401, 17)):
        tail = (up[M][0][16384:], up[M][1][16384:])
        assert _bits(tail, alone[n]), (M, n)
        assert _bits((up[M][0][:16384], up[M][1][:16384]), up[16384]), M
    ei = float(np.max(np.abs(Ai - Ainv)) / np.max(np.abs(Ainv)))
    assert ei < RTOL and np.array_equal(Ai, Ai.T), ei
    print(f"\nN={N} kind {kind}: worst {worst:.2e}, C^-1 {ei:.2e} (cond_1 {ref['cond']:.2e}, clamp margin {ref['margin']:.1e}), "
          f"{time.time() - t0:.1f} s")


@pytest.mark.gpu
def test_n8193_matern52_every_regime():
    """N = 8193 (Np = 8256: nslice 15, klen 560 = 35 x 16; 63 padding rows), Matern 5/2, order 1, d = 8 on the bench's
    design seed: the ladder up to 1500"""
    t0 = time.time()
    N, d, kind, order = 8193, 8, 3, 1
    X, y = synth.design(N, d, SEED_C3)
    th = synth.default_thetas(kind, d)
    Q = query_pool(X, 1500, 8193)
    ref = model_reference(kind, order, X, y, th, Q)
    c = abi.Context(0)
    try:
        c.set_model(kind, order, X, y)
        _, rc = c.predict_setup(th)
        assert rc == 0
        up, down = run_ladder(c, Q, LADDER)
    finally:
        c.close()
    worst = check_ladder(N, ref, up, down)
    print(f"\nN={N} Matern 5/2: worst {worst:.2e} (cond_1 {ref['cond']:.2e}, clamp margin {ref['margin']:.1e}), "
          f"{time.time() - t0:.1f} s")


# ------------------------------------------------------------------ device half, part B
@pytest.mark.gpu
@pytest.mark.parametrize("N", (8191, 8193))
def test_matern52_ragged_batch_of_16(N):
    """Matern 5/2, d = 8, order 1, a lock-step batch of 16 from 4 thetas (perturbed_thetas, t(b) = b mod 4: no neighbour
    shares one) at N = 8191 (the bench's Np, one padding row) and 8193 (Np = 8256: 63 padding rows, a lone 64-column leaf
    at the end of the outer panel, c_rows = 64 mod 128 in trailing_update): every element against LAPACK; the reversed
    batch gives every element the same bits; a single evaluation equals its element bit for bit"""
    t0 = time.time()
    X, y = synth.design(N, 8, SEED_C3)
    distinct = np.array([synth.perturbed_thetas(3, 8, SEED_C3 + N, i) for i in range(4)])
    refs, conds = likelihood_references(3, 1, X, y, distinct)
    pos = np.arange(16) % 4
    ths = distinct[pos]
    c = abi.Context(0)
    try:
        c.set_model(3, 1, X, y)
        got = c.loglik_batch(ths)
        rev = c.loglik_batch(ths[::-1].copy())
        one = c.loglik(distinct[1])
    finally:
        c.close()
    assert np.all(got["status"] == 0) and np.all(got["info"] == 0) and np.all(rev["status"] == 0) and one["status"] == 0
    worst = 0.0
    for b in range(16):
        e = lik_errors(got, b, refs[pos[b]])
        worst = max(worst, max(e))
        assert max(e) < RTOL, (b, e, conds[pos[b]])
        assert same_bits(got, b, rev, 15 - b), b
    single = {k: [one[k]] for k in ("value", "sigma2", "logdet", "quad", "beta")}
    assert same_bits(got, 1, single, 0)
    print(f"\nN={N} Matern B=16: worst {worst:.2e} (cond_1 up to {max(conds):.2e}), {time.time() - t0:.1f} s")


@pytest.mark.gpu
def test_powexp_n4097_d16_batch_of_64():
    """pow-exp, N = 4097, d = 16, order 1, a batch of 64 (GPEMU_MAX_BATCH) from 8 thetas at t(b) = (b + b // 8) mod 8
    (elements 1, 8, 16, 18 and 32 apart never share one): every element against LAPACK; same theta, same bits"""
    t0 = time.time()
    X, y = synth.design(4097, 16, 20261003 + 3)
    distinct = np.array([synth.perturbed_thetas(1, 16, 4097, i) for i in range(8)])
    refs, conds = likelihood_references(1, 1, X, y, distinct)
    pos = np.array([(b + b // 8) % 8 for b in range(64)])
    c = abi.Context(0)
    try:
        c.set_model(1, 1, X, y)
        got = c.loglik_batch(distinct[pos])
    finally:
        c.close()
    assert np.all(got["status"] == 0) and np.all(got["info"] == 0)
    worst = 0.0
    for b in range(64):
        e = lik_errors(got, b, refs[pos[b]])
        worst = max(worst, max(e))
        assert max(e) < RTOL, (b, e, conds[pos[b]])
        first = int(np.argmax(pos == pos[b]))
        assert same_bits(got, b, got, first), (b, first)
    print(f"\nN=4097 d=16 B=64: worst {worst:.2e} (cond_1 up to {max(conds):.2e}), {time.time() - t0:.1f} s")


@pytest.mark.gpu
def test_powexp_value_gradient_n8193_batch_of_20():
    """gpemu_loglik_grad_batch at N = 8193 (the gradient kernels' gr < N masks leave one valid row in the last tile row),
    d = 8, order 1, B = 20: corners in chunks of 18 + 2.  Two thetas, alternating; literal and exact gradient, every
    element against tests/gradref.py at 1e-8 of max |g|; elements 0 and 18 (same theta, chunks 0 and 1) carry the same bits"""
    import gradref
    t0 = time.time()
    N, d, B = 8193, 8, 20
    X, y = synth.design(N, d, SEED_C3)
    base = synth.default_thetas(1, d)
    alt = base.copy()
    alt[1] = -3.5
    alt[2:] += 0.3 * np.linspace(-1.0, 1.0, d)
    distinct = np.array([base, alt])
    chunk = grad_chunk_size(N, B)
    assert chunk == 18 and -(-B // chunk) == 2
    refs, conds = [], []
    for th in distinct:
        th0 = np.concatenate([[0.0], th[1:]])                 # the gradient path takes theta0 as 0 (maxmultimin.c:311,441)
        conds.append(factor(O.cov_matrix(1, X, th0))[1])
        assert conds[-1] <= COND_MAX, conds[-1]
        refs.append(gradref.value_and_gradients(X, y, 1, th))
    pos = np.arange(B) % 2
    c = abi.Context(0)
    try:
        c.set_model(1, 1, X, y)
        got = {}
        for mode in (0, abi.MODE_EXACT_GRAD):
            c.set_mode(mode)
            got[mode] = c.loglik_grad_batch(distinct[pos])
        c.set_mode(0)
    finally:
        c.close()
    worst = {}
    for mode, key in ((0, "literal"), (abi.MODE_EXACT_GRAD, "exact")):
        g = got[mode]
        assert np.all(g["status"] == 0), key
        w = 0.0
        for b in range(B):
            r = refs[pos[b]]
            e = [float(np.max(np.abs(g["grad"][b] - r[key])) / np.max(np.abs(r[key]))),
                 abs(g["value"][b] - r["value"]) / abs(r["value"]), abs(g["sigma2"][b] - r["sigma2"]) / abs(r["sigma2"]),
                 float(np.max(np.abs(g["beta"][b] - r["beta"])) / np.max(np.abs(r["beta"])))]
            w = max(w, max(e))
            assert max(e) < RTOL, (key, b, e)
        assert all(np.array_equal(g[k][0], g[k][18]) for k in ("value", "sigma2", "beta", "grad")), key
        worst[key] = w
    print(f"\nN={N} B={B} (chunks of {chunk}): worst literal {worst['literal']:.2e} exact {worst['exact']:.2e} "
          f"(cond_1 up to {max(conds):.2e}), {time.time() - t0:.1f} s")
