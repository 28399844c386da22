"""Every element of full-width lock-step batches -- the batch widths and sizes the benchmark times -- against numpy / LAPACK.

The rest of the suite checks a large batch through its first and last element, or through bit equality with a single
evaluation; here every element has a reference of its own.  Nothing in a reference chain comes from the device: the
covariance matrix is built on the host (scipy's difference-form distances in the formulas of emulator.c:101-152 and
438-480, checked on sampled elements against the oracle's covariance function), factored by LAPACK (dpotrf, cho_solve)
and the value, sigma^2, beta, log det and quadratic form are formed as in test_config4_eight_pca_components_n4096_d16;
gradients come from tests/gradref.py or the committed N = 16384 fixture.  Each case asserts its own precondition, the
LAPACK 1-norm condition estimate (dpocon) of every distinct matrix <= 5e6 (the threshold of the randomised sweep), before
it compares at the plain 1e-8 bar.  The reference halves are plain functions (`*_reference`): they run without a device."""
import os
import time

import numpy as np
import pytest
import scipy.linalg as sl
from scipy.linalg import lapack
from scipy.spatial.distance import cdist, pdist

from madaiemulator_amd import abi, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

RTOL = 1e-8              # the north_star parity bar
COND_MAX = 5e6           # test_randomised_parity_sweep's threshold for the plain bar
ROOT5 = 2.236067978      # covariance_fn_matern_five's constant (emulator.c:438-480), as the oracle and the device use it
SEED_C3 = 20261003 + 2   # bench.py's design seed (region A, BASELINE.json configs[2])


# ------------------------------------------------------------------ reference half (host only)
def powexp_matrix(X, th):
    """emulator.c:101-152 for a design without coincident points: e^t0 exp(-1/2 sum_k D_k^2 / e^{2 t_{k+2}}) + e^t1 I"""
    r = np.exp(th[2:2 + X.shape[1]])
    Cm = cdist(X / r, X / r, "sqeuclidean")
    Cm *= -0.5
    np.exp(Cm, out=Cm)
    Cm *= np.exp(th[0])
    Cm[np.diag_indices_from(Cm)] += np.exp(th[1])
    return Cm


def matern52_matrix(dist, th):
    """emulator.c:438-480 (raw amplitude and nugget) on a precomputed distance matrix of a design without
    coincident points: amp (1 + r5 t + 5/3 t^2) e^{-r5 t}, t = |x - x'| / e^{t2}; amp + nugget on the diagonal"""
    t = dist / np.exp(th[2])
    Cm = ROOT5 * t
    np.exp(-Cm, out=Cm)
    Cm *= 1.0 + ROOT5 * t + (5.0 / 3.0) * t * t
    Cm *= th[0]
    Cm[np.diag_indices_from(Cm)] = th[0] + th[1]
    return Cm


def cov_matrix(kind, X, th, dist=None):
    if kind == 1:
        return powexp_matrix(X, th)
    assert kind == 3
    return matern52_matrix(cdist(X, X) if dist is None else dist, th)


def assert_distinct_points(X, sep=1e-6):
    """the matrices above put the nugget on the diagonal only: no two design points may be 'the same point'"""
    assert pdist(X).min() > sep


def check_matrix_against_oracle(kind, X, th, Cm, n=3000, seed=0):
    """sampled elements (random pairs, diagonal, the last row) of a host-built matrix against the oracle's covariance
    function at 1e-13 (+ the rounding exp(-x) inherits from its argument)"""
    N = X.shape[0]
    rng = np.random.default_rng(seed)
    I = np.concatenate([rng.integers(0, N, n), np.arange(0, N, max(1, N // 64)), np.full(64, N - 1)])
    J = np.concatenate([rng.integers(0, N, n), np.arange(0, N, max(1, N // 64)), rng.integers(0, N, 64)])
    ref = np.array([O.cov(kind, X[a], X[b], th) for a, b in zip(I, J)])
    amp = np.exp(th[0]) if kind == 1 else th[0]
    big = np.abs(ref) > 1e-290
    tol = 1e-13 + 1e-15 * np.abs(np.log(np.abs(ref[big]) / amp))
    assert np.all(np.abs(Cm[I, J][big] - ref[big]) / np.abs(ref[big]) < tol)


def factor(Cm):
    """LAPACK dpotrf of Cm (overwritten) and the 1-norm condition estimate dpocon -> (cho_factor tuple, cond_1)"""
    anorm = np.abs(Cm).sum(axis=0).max()
    cf = sl.cho_factor(Cm.T, lower=True, overwrite_a=True, check_finite=False)     # Cm is symmetric: Cm.T is its F-order view
    rcond, info = lapack.dpocon(cf[0], anorm, uplo="L")
    assert info == 0
    return cf, 1.0 / rcond


def likelihood_from_factor(cf, H, y):
    """value (-logL with the reference's 1.83788), sigma^2, beta, log det, quad as test_config4_eight_pca_components_n4096_d16"""
    N = y.size
    logdet = 2.0 * np.log(np.diag(cf[0])).sum()
    AyH = sl.cho_solve(cf, np.column_stack([y, H]), check_finite=False)
    beta = np.linalg.solve(H.T @ AyH[:, 1:], H.T @ AyH[:, 0])
    r = y - H @ beta
    Ar = sl.cho_solve(cf, r, check_finite=False)
    quad = r @ Ar
    return dict(value=-(-0.5 * logdet - N / 2.0 * 1.83788 - 0.5 * quad), sigma2=(y @ Ar) / N, beta=beta, logdet=logdet,
                quad=quad)


def likelihood_references(kind, order, X, y, ths, check_first=True):
    """one LAPACK reference per row of ths; asserts cond_1 <= COND_MAX for each -> (list of dicts, list of cond_1)"""
    assert_distinct_points(X)
    H = O.hmatrix(order, X)
    dist = cdist(X, X) if kind == 3 else None
    refs, conds = [], []
    for i, th in enumerate(ths):
        Cm = cov_matrix(kind, X, th, dist)
        if check_first and i == 0:
            check_matrix_against_oracle(kind, X, th, Cm)      # the host matrix IS the oracle's matrix
        cf, cond = factor(Cm)
        assert cond <= COND_MAX, (i, th, cond)
        refs.append(likelihood_from_factor(cf, H, y))
        conds.append(cond)
        del Cm, cf
    return refs, conds


def lik_errors(got, b, ref):
    """relative errors of element b of a batch result against its reference (value, sigma^2, log det, quad, beta)"""
    e = [abs(got[k][b] - ref[k]) / abs(ref[k]) for k in ("value", "sigma2", "logdet", "quad")]
    e.append(float(np.max(np.abs(got["beta"][b] - ref["beta"])) / np.max(np.abs(ref["beta"]))))
    return e


def same_bits(a, i, b, j, keys=("value", "sigma2", "logdet", "quad", "beta")):
    return all(np.array_equal(np.asarray(a[k][i]), np.asarray(b[k][j])) for k in keys if k in a and k in b)


def grad_chunk_size(N, nb):
    """the number of corners gpemu_loglik_grad_batch keeps in flight (gpemu_api.hip, grad_chunk_size): as many
    (Np + Rp)^2 doubles as fit in 10 GB, Np = N rounded up to 64, Rp = 64"""
    dim = (N + 63) // 64 * 64 + 64
    return max(1, min(nb, int(10.0e9 / (dim * dim * 8.0))))


# ---- case 1: pow-exp, N = 4096, d = 16, B = 64 (the pca8 region's width, GPEMU_MAX_BATCH)
def case1_inputs():
    N, d, B = 4096, 16, 64                                    # B = GPEMU_MAX_BATCH (include/gpemu.h)
    X, y = synth.design(N, d, 20261003 + 3)                    # the configs[3] design
    u = synth.uniform(4242, (B, d + 2))
    ths = np.empty((B, d + 2))
    ths[:, 0] = -1.0 + 2.0 * u[:, 0]                           # amplitude e^[-1, 1]
    ths[:, 1] = -7.0 + 5.0 * u[:, 1]                           # nugget e^[-7, -2]
    ths[:, 2:] = np.log(0.6) + (2.0 * u[:, 2:] - 1.0) * 0.5     # length scales 0.6 e^[-0.5, 0.5]
    return X, y, ths


def case1_reference():
    X, y, ths = case1_inputs()
    refs, conds = likelihood_references(1, 1, X, y, ths)
    return X, y, ths, refs, conds


# ---- case 2: Matern 5/2, N = 8192, d = 8, order 1 -- bench.py's region A model
def case2a_inputs():
    X, y = synth.design(8192, 8, SEED_C3)
    ths = np.array([synth.perturbed_thetas(3, 8, SEED_C3, i) for i in range(16)])   # as bench.py draws them
    return X, y, ths


def case2b_inputs():
    X, y = synth.design(8192, 8, SEED_C3)
    u = synth.uniform(777, (8, 3))
    distinct = np.column_stack([0.5 + u[:, 0], 0.01 + 0.04 * u[:, 1], np.log(0.6) + 0.5 * (u[:, 2] - 0.5)])
    pos = np.array([(b + b // 8) % 8 for b in range(64)])      # offsets 1, 8, 16, 18, 32 never share a theta
    return X, y, distinct, pos


def case2a_reference():
    X, y, ths = case2a_inputs()
    refs, conds = likelihood_references(3, 1, X, y, ths)
    return X, y, ths, refs, conds


def case2b_reference():
    X, y, distinct, pos = case2b_inputs()
    refs, conds = likelihood_references(3, 1, X, y, distinct)
    return X, y, distinct, pos, refs, conds


# ---- case 3: a non-PD element inside a Matern 5/2 batch, N = 4096, d = 8, B = 16
BAD_THETA = np.array([1.0, -0.5, np.log(0.02)])            # amp 1, raw nugget -0.5: diagonal 0.5
NOT_PD_ROWS = (40, 2048, 2112, 2176, 4095)


def case3_inputs(p):
    X, y = synth.design(4096, 8, SEED_C3)
    X = X.copy()
    X[p] = X[p - 1]
    X[p, 0] += 1e-3                                           # row p 1e-3 from row p-1: pivot p + 1 (1-based) goes negative
    goods = np.array([synth.perturbed_thetas(3, 8, 20261003 + p, i) for i in range(16)])
    return X, y, goods


def case3_reference(p, compare=(1, 15)):
    """the bad element's matrix: LAPACK's first failed pivot is p + 1, and it is isolated -- every row's off-diagonal
    1-norm, the (p-1, p) pair left out, is <= 3e-3 against a 0.5 diagonal, so pivots 1 .. p are >= 0.49 (Gershgorin) and
    pivot p + 1 is 0.5 - c^2 / (pivot p) with c = C[p, p-1] close to 1.  References of two good elements."""
    X, y, goods = case3_inputs(p)
    assert_distinct_points(X, sep=5e-4)
    dist = cdist(X, X)
    Cb = matern52_matrix(dist, BAD_THETA)
    check_matrix_against_oracle(3, X, BAD_THETA, Cb, n=500, seed=p)
    c = Cb[p, p - 1]
    off = np.abs(Cb).sum(axis=1) - np.abs(np.diag(Cb))
    off[p] -= abs(c)
    off[p - 1] -= abs(c)
    margins = dict(offdiag=float(off.max()), pair=float(c), pivot=float(0.5 - c * c / 0.5))
    assert margins["offdiag"] <= 3e-3 and margins["pivot"] < -1.0
    _, info = lapack.dpotrf(Cb, lower=1, overwrite_a=1)
    assert info == p + 1
    del Cb
    H = O.hmatrix(1, X)
    refs, conds = {}, []
    for b in compare:
        cf, cond = factor(matern52_matrix(dist, goods[b]))
        assert cond <= COND_MAX, (b, cond)
        refs[b] = likelihood_from_factor(cf, H, y)
        conds.append(cond)
    return X, y, goods, refs, conds, margins


# ---- case 4: value + gradient batches across the corner chunks of gpemu_loglik_grad_batch
def case4a_inputs():
    N, d, B = 8192, 8, 40
    X, y = synth.design(N, d, SEED_C3)
    base = synth.default_thetas(1, d)
    distinct = np.array([base, base, base])
    distinct[1, 1], distinct[2, 1] = -3.5, -4.5
    distinct[1, 2:] += 0.3 * np.linspace(-1.0, 1.0, d)
    distinct[2, 2:] += 0.2 - 0.4 * np.linspace(-1.0, 1.0, d) ** 2
    pos = np.array([(b + b // 18) % 3 for b in range(B)])        # no element shares its theta with b +- 1, b - 18, b - 36
    return X, y, distinct, pos


def case4a_reference():
    import gradref
    X, y, distinct, pos = case4a_inputs()
    assert_distinct_points(X)
    refs, conds = [], []
    for i, th in enumerate(distinct):
        Cm = powexp_matrix(X, np.concatenate([[0.0], th[1:]]))
        if i == 0:
            check_matrix_against_oracle(1, X, np.concatenate([[0.0], th[1:]]), Cm)
        conds.append(factor(Cm)[1])
        del Cm
        assert conds[-1] <= COND_MAX, (i, conds[-1])
        refs.append(gradref.value_and_gradients(X, y, 1, th))
    return X, y, distinct, pos, refs, conds


def case4b_inputs():
    f = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_n16384_c5.npz"))
    kind, order, N, d, seed = (int(v) for v in f["meta"])
    assert (kind, order, N, d, seed) == (1, 0, 16384, 8, 20261003 + 4)
    X, y = synth.design(N, d, seed)
    ths = np.array([synth.perturbed_thetas(1, d, 61, i) for i in range(6)])
    ths[2] = ths[4] = f["thetas"]
    ths[:, 0] = 0.0
    return X, y, ths, f


# ------------------------------------------------------------------ device half
def _ctx_with_env(monkeypatch, env, device=0):
    """a context whose schedule switches come from `env` (copied into the context when it is created)"""
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    c = abi.Context(device)
    for k_ in env:
        monkeypatch.delenv(k_)
    return c


def test_powexp_n4096_d16_batch_of_64_every_element_against_lapack():
    """pca8 width: 64 distinct thetas far beyond perturbed_thetas (amplitude e^[-1,1], nugget e^[-7,-2], every length scale
    0.6 e^[-0.5,0.5]) in one lock-step batch at N = 4096, d = 16, order 1; every element against its LAPACK reference, and
    the same batch reversed gives every element the same bits (an element's result does not depend on its position)."""
    t0 = time.time()
    X, y, ths, refs, conds = case1_reference()
    c = abi.Context(0)
    try:
        c.set_model(1, 1, X, y)
        got = c.loglik_batch(ths)
        rev = c.loglik_batch(ths[::-1].copy())
    finally:
        c.close()
    B = len(ths)
    assert np.all(got["status"] == 0) and np.all(got["info"] == 0) and np.all(rev["status"] == 0)
    worst = 0.0
    for b in range(B):
        e = lik_errors(got, b, refs[b])
        worst = max(worst, max(e))
        assert max(e) < RTOL, (b, e, conds[b])
        assert same_bits(got, b, rev, B - 1 - b), b
    print(f"\ncase 1 N=4096 d=16 B=64: worst {worst:.2e} (cond_1 up to {max(conds):.2e}), {time.time() - t0:.1f} s")


def test_matern52_n8192_bench_thetas_batch_of_16_every_element_against_lapack():
    """region A exactly: bench.py's design, model and theta draws (perturbed_thetas(3, 8, seed, i)), a lock-step batch of
    16 at N = 8192; every element against its LAPACK reference"""
    t0 = time.time()
    X, y, ths, refs, conds = case2a_reference()
    c = abi.Context(0)
    try:
        c.set_model(3, 1, X, y)
        got = c.loglik_batch(ths)
    finally:
        c.close()
    assert np.all(got["status"] == 0) and np.all(got["info"] == 0)
    worst = 0.0
    for b in range(len(ths)):
        e = lik_errors(got, b, refs[b])
        worst = max(worst, max(e))
        assert max(e) < RTOL, (b, e, conds[b])
    print(f"\ncase 2a N=8192 Matern B=16: worst {worst:.2e} (cond_1 up to {max(conds):.2e}), {time.time() - t0:.1f} s")


def test_matern52_n8192_batch_of_64_element_offsets_beyond_2_31():
    """B = 64 at N = 8192: an element's workspace is (8192 + 64) x 8192 doubles, so from element 32 on its offset
    ((long)blockIdx.y * stride) passes 2^31 doubles (35 GB of workspace).  Eight distinct thetas at t(b) = (b + b // 8) mod 8:
    elements 1, 8, 16, 18 and 32 apart never share one.  Every element against its LAPACK reference; elements with the
    same theta carry the same bits."""
    t0 = time.time()
    X, y, distinct, pos, refs, conds = case2b_reference()
    ths = distinct[pos]
    assert (len(ths) - 1) * (8192 + 64) * 8192 > 2 ** 31
    c = abi.Context(0)
    try:
        c.set_model(3, 1, X, y)
        got = c.loglik_batch(ths)
    finally:
        c.close()
    assert np.all(got["status"] == 0) and np.all(got["info"] == 0)
    worst = 0.0
    for b in range(len(ths)):
        e = lik_errors(got, b, refs[pos[b]])
        worst = max(worst, max(e))
        assert max(e) < RTOL, (b, e, conds[pos[b]])
        first = int(np.argmax(pos == pos[b]))
        assert same_bits(got, b, got, first), (b, first)
    print(f"\ncase 2b N=8192 Matern B=64: worst {worst:.2e} (cond_1 up to {max(conds):.2e}), {time.time() - t0:.1f} s")


@pytest.mark.parametrize("p", NOT_PD_ROWS)
def test_not_pd_element_inside_a_batch_reports_its_pivot(monkeypatch, p):
    """One element of a Matern 5/2 batch (N = 4096, d = 8, B = 16) has a first non-positive pivot at exactly p + 1
    (1-based; case3_reference shows it with LAPACK and the margins that isolate it).  Which kernel meets that pivot
    (potrf_rec of a likelihood batch: 2048-column top panels, halved down to 128-column pairs; 64-column leaves):
      p = 40    leaf_factor_kernel at c0 = 0;
      p = 2048  leaf_factor_kernel at the head of the second top panel (the top-level update runs on 128x128 tiles, which
                carry no factor-ahead tile, so the pair at c0 = 2048 factors its first block itself);
      p = 2112  leaf_pair_kernel's factor-ahead tile (the second block of the pair at c0 = 2048);
      p = 2176  the GEMM's factor-ahead tile (the 128-column update inside the 256-column panel at 2048: 64x64 tiles);
      p = 4095  leaf_pair_kernel's factor-ahead tile at the last block of the matrix (the pair at c0 = 3968).
    With GPEMU_FACTOR_AHEAD=0 every block is factored by leaf_factor_kernel; with GPEMU_LEAF_PAIR=0 or
    GPEMU_DIAG_INV_AHEAD=0 the pair blocks of p = 2112 and 4095 are factored by the GEMM's factor-ahead tile.
    The bad element sits at index 0, then at index 11: status GPEMU_ERR_NOT_PD, info p + 1, value and beta NaN; every
    other element has status 0 and the bits of the same batch with the bad theta replaced by a good one; two of them
    against LAPACK."""
    t0 = time.time()
    X, y, goods, refs, conds, margins = case3_reference(p)
    batches = {}
    for at in (0, 11):
        ths = goods.copy()
        ths[at] = BAD_THETA
        batches[at] = ths
    envs = [{}, {"GPEMU_FACTOR_AHEAD": "0"}, {"GPEMU_LEAF_PAIR": "0"}, {"GPEMU_DIAG_INV_AHEAD": "0"}]
    worst = 0.0
    clean = None
    for env in envs:
        c = _ctx_with_env(monkeypatch, env)
        try:
            c.set_model(3, 1, X, y)
            ok = c.loglik_batch(goods)
            got = {at: c.loglik_batch(batches[at]) for at in batches}
        finally:
            c.close()
        assert np.all(ok["status"] == 0) and np.all(ok["info"] == 0), env
        if clean is None:
            clean = ok
            for b, ref in refs.items():
                e = lik_errors(ok, b, ref)
                worst = max(worst, max(e))
                assert max(e) < RTOL, (b, e)
        for at, g in got.items():
            assert g["status"][at] == abi.ERR_NOT_PD and g["info"][at] == p + 1, (env, at, g["status"][at], g["info"][at])
            assert np.isnan(g["value"][at]) and np.all(np.isnan(g["beta"][at])), (env, at)
            for b in range(len(goods)):
                if b == at:
                    continue
                assert g["status"][b] == 0 and g["info"][b] == 0, (env, at, b)
                assert same_bits(g, b, clean, b), (env, at, b)
    print(f"\ncase 3 p={p}: worst {worst:.2e} (cond_1 {max(conds):.2e}; off-diagonal row sums <= {margins['offdiag']:.1e}, "
          f"C[p,p-1] = {margins['pair']:.6f}, pivot ~ {margins['pivot']:.3f}), {time.time() - t0:.1f} s")


def _grad_errors(got, b, ref, key):
    g = ref[key]
    return [float(np.max(np.abs(got["grad"][b] - g)) / np.max(np.abs(g))), abs(got["value"][b] - ref["value"]) / abs(ref["value"]),
            abs(got["sigma2"][b] - ref["sigma2"]) / abs(ref["sigma2"]),
            float(np.max(np.abs(got["beta"][b] - ref["beta"])) / np.max(np.abs(ref["beta"])))]


def _run_grad_modes(c, ths):
    """for the literal and the exact form: the blocking call, and the enqueue / collect_back halves with the batch and its
    reverse in flight together -> {mode: (blocking, collected, collected reverse)}"""
    out = {}
    for mode in (0, abi.MODE_EXACT_GRAD):
        c.set_mode(mode)
        bat = c.loglik_grad_batch(ths)
        c.loglik_grad_batch_enqueue(ths)
        c.loglik_grad_batch_enqueue(ths[::-1].copy())
        early, late = c.loglik_grad_batch_collect_back(1, len(ths)), c.loglik_grad_batch_collect_back(0, len(ths))
        out[mode] = (bat, early, late)
    c.set_mode(0)
    return out


def _same_grad_bits(a, i, b, j):
    return all(np.array_equal(np.asarray(a[k][i]), np.asarray(b[k][j])) for k in ("value", "sigma2", "beta", "grad"))


def test_value_gradient_batch_of_40_spans_three_corner_chunks_n8192():
    """gpemu_loglik_grad_batch at N = 8192, d = 8, pow-exp, order 1, B = 40: the corners C^-1 = U U^T go in chunks of 18
    (18 + 18 + 4), so the chunk offset b0 > 0 of grad_enqueue_chunk moves build_corner's A pointer, the pinned length-theta
    ring, dParams + b0, dRes + b0 * res_len (exact mode) and dGradSum + b0 * GRAD_NP_MAX.  Three thetas at
    t(b) = (b + b // 18) mod 3 (no element shares one with b +- 1, b - 18 or b - 36).  Literal and exact gradient, blocking
    call and enqueue / collect_back, against tests/gradref.py; every element carries the bits of its theta in a one-chunk
    batch.  About 53 GB of device memory (43 GB of workspace with the inverse rows, 9.8 GB of corners)."""
    t0 = time.time()
    X, y, distinct, pos, refs, conds = case4a_reference()
    N, B = X.shape[0], len(pos)
    chunk = grad_chunk_size(N, B)
    assert chunk == 18 and -(-B // chunk) == 3                # the batch really spans three chunks
    rng = np.ptp(X, axis=0)
    assert np.all(0.5 * np.exp(-2.0 * distinct[:, 2:]) * rng ** 2 < 300.0)   # every chunk takes the same (noclamp) kernel
    ths = distinct[pos]
    c = abi.Context(0)
    try:
        c.set_model(1, 1, X, y)
        one = _run_grad_modes(c, distinct)                    # one chunk: the three thetas alone
        big = _run_grad_modes(c, ths)
    finally:
        c.close()
    worst = {}
    for mode, key in ((0, "literal"), (abi.MODE_EXACT_GRAD, "exact")):
        bat, early, late = big[mode]
        assert np.all(bat["status"] == 0) and np.all(one[mode][0]["status"] == 0)
        w = 0.0
        for b in range(B):
            e = _grad_errors(bat, b, refs[pos[b]], key)
            w = max(w, max(e))
            assert max(e) < RTOL, (key, b, e)
            assert _same_grad_bits(bat, b, one[mode][0], pos[b]), (key, b)
            assert _same_grad_bits(bat, b, early, b) and _same_grad_bits(bat, b, late, B - 1 - b), (key, b)
        worst[key] = w
    print(f"\ncase 4a N=8192 B=40 (chunks of {chunk}): worst literal {worst['literal']:.2e} exact {worst['exact']:.2e} "
          f"(cond_1 up to {max(conds):.2e}), {time.time() - t0:.1f} s")


def test_value_gradient_batch_of_6_spans_two_corner_chunks_n16384():
    """N = 16384 (configs[4]): corners of (16384 + 64)^2 doubles go in chunks of 4, a batch of 6 in two.  The committed
    fixture's theta (tests/golden/golden_n16384_c5.npz: numpy / LAPACK value and both gradients) sits at position 2 (first
    chunk) and position 4 (second chunk, b0 = 4), perturbed thetas elsewhere: both elements against the fixture, and
    with the same bits."""
    t0 = time.time()
    X, y, ths, f = case4b_inputs()
    N, B = X.shape[0], len(ths)
    chunk = grad_chunk_size(N, B)
    assert chunk == 4 and -(-B // chunk) == 2
    c = abi.Context(0)
    try:
        c.set_model(1, 0, X, y)
        out = _run_grad_modes(c, ths)
    finally:
        c.close()
    ref = dict(value=float(f["value"]), sigma2=float(f["sigma2"]), beta=f["beta"], literal=f["literal"], exact=f["exact"])
    worst = {}
    for mode, key in ((0, "literal"), (abi.MODE_EXACT_GRAD, "exact")):
        bat, early, late = out[mode]
        assert np.all(bat["status"] == 0) and np.all(np.isfinite(bat["grad"]))
        w = 0.0
        for b in (2, 4):
            e = _grad_errors(bat, b, ref, key)
            w = max(w, max(e))
            assert max(e) < RTOL, (key, b, e)
        assert _same_grad_bits(bat, 2, bat, 4), key
        for b in range(B):
            assert _same_grad_bits(bat, b, early, b) and _same_grad_bits(bat, b, late, B - 1 - b), (key, b)
        worst[key] = w
    print(f"\ncase 4b N=16384 B=6 (chunks of {chunk}): worst literal {worst['literal']:.2e} exact {worst['exact']:.2e}, "
          f"{time.time() - t0:.1f} s")
