"""numpy replica of the ensemble sampler (include/gpemu.h): Philox4x32-10, the uniform U made of two words, the
stretch proposal of one half against the other, the accept step, and a whole run over any Python log-likelihood callable.

The integer part and U are bit-exact everywhere; z and y use +, * and / alone (one rounding each: the kernels form them
without contraction), so they are the device's bits too.  log z, the log prior and log u3 go through a logarithm: the device's
may differ from numpy's in the last place, which the GPU tests' bars allow for.

BARS: what the CPU tests of tests/test_sampleref.py and the GPU end-to-end tests assert against.  Every bar is the replica's own
largest error over 16 seeds OTHER than the asserting test's, times 2, measured by test_sampleref.measure_bars (kept there)."""
import numpy as np

UNIFORM, GAUSS = 0, 1
M32 = np.uint64(0xFFFFFFFF)
HALF_LOG_2PI = 0.91893853320467274178032973640562


def philox4x32(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on broadcastable arrays of 32-bit words -> four uint32 arrays"""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v).astype(np.uint64) & M32 for v in np.broadcast_arrays(c0, c1, c2, c3, k0, k1))
    m0, m1, w0, w1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                        # 32 x 32 bits: inside uint64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & M32, (p0 >> s32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + w0) & M32, (k1 + w1) & M32
    return tuple(v.astype(np.uint32) for v in (c0, c1, c2, c3))


def uniform(a, b):
    """U(a, b) = ((a << 20 | b >> 12) + 0.5) 2^-52, exact in float64"""
    n = (np.asarray(a).astype(np.uint64) << np.uint64(20)) | (np.asarray(b).astype(np.uint64) >> np.uint64(12))
    return (2 * n + 1).astype(np.float64) * 2.0 ** -53


def words(seed, c0, c12, c3):
    c12 = np.asarray(c12, dtype=np.uint64)
    return philox4x32(c0, c12 & M32, c12 >> np.uint64(32), c3, np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32))


def uniforms(seed, walkers, step):
    """(u1, u2, u3) of the walkers at a global step"""
    w = words(seed, walkers, step, 0)
    v = words(seed, walkers, step, 1)
    return uniform(w[0], w[1]), uniform(w[2], w[3]), uniform(v[0], v[1])


def prior_draws(seed, W, lo, hi, kind):
    """the host layer's default starts: counter (k, j, 0, 2) for coordinate j of walker k"""
    lo, hi, kind = np.asarray(lo, float), np.asarray(hi, float), np.asarray(kind)
    k, j = np.meshgrid(np.arange(W), np.arange(lo.size), indexing="ij")
    w = words(seed, k, j, 2)
    u1, u2 = uniform(w[0], w[1]), uniform(w[2], w[3])
    return np.where(kind == GAUSS, lo + hi * (np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)), lo + u1 * (hi - lo))


def prior_terms(y, lo, hi, kind):
    """per-coordinate log prior of the rows of y, the constants as the library tabulates them"""
    lo, hi, kind = np.asarray(lo, float), np.asarray(hi, float), np.asarray(kind)
    g = kind == GAUSS
    with np.errstate(invalid="ignore", divide="ignore"):
        cst = np.where(g, -np.log(np.where(g, hi, 1.0)) - HALF_LOG_2PI, -np.log(np.where(g, 1.0, hi - lo)))
        r = (y - lo) / hi
        return np.where(g, -0.5 * (r * r) + cst, np.where((y >= lo) & (y <= hi), cst, -np.inf))


def log_prior(y, lo, hi, kind):
    """summed over the coordinates in index order from 0.0"""
    t = prior_terms(np.atleast_2d(y), lo, hi, kind)
    s = np.zeros(t.shape[0])
    for c in range(t.shape[1]):
        s = s + t[:, c]
    return s


def propose(x, half, step, seed, a, lo, hi, kind):
    """-> y[W/2, d], aux[W] ((d - 1) log z, then the log prior of y), partner[W/2] (global index), z[W/2]"""
    W, d = x.shape
    h = W // 2
    base, other = half * h, (1 - half) * h
    u1, u2, _ = uniforms(seed, base + np.arange(h), step)
    j = other + np.minimum((u1 * h).astype(np.int64), h - 1)
    s = (a - 1.0) * u2 + 1.0
    z = s * s / a
    xj, xk = x[j], x[base:base + h]
    y = xj + z[:, None] * (xk - xj)
    lz = np.zeros(h) if d == 1 else (d - 1.0) * np.log(z)
    return y, np.concatenate([lz, log_prior(y, lo, hi, kind)]), j, z


def accept_margin(lp, half, step, seed, aux, loglik):
    """-> lp_y, log u3, log r of the active half, in the kernel's operation order"""
    h = lp.size // 2
    base = half * h
    _, _, u3 = uniforms(seed, base + np.arange(h), step)
    with np.errstate(invalid="ignore"):
        lpy = loglik + aux[h:]
        logr = aux[:h] + lpy - lp[base:base + h]
    return lpy, np.log(u3), logr


def accept(x, lp, nacc, half, step, seed, y, aux, loglik):
    """the accept step in place -> the decisions of the active half"""
    h = lp.size // 2
    base = half * h
    lpy, lu, logr = accept_margin(lp, half, step, seed, aux, loglik)
    with np.errstate(invalid="ignore"):
        take = np.isfinite(lpy) & (lu < logr)
    k = base + np.flatnonzero(take)
    x[k] = y[take]
    lp[k] = lpy[take]
    nacc[k] += 1
    return take


def run(loglik, x0, nsteps, lo, hi, kind, burn=0, thin=1, seed=0, first_step=0, a=2.0):
    """loglik(points[M, d]) -> M log likelihoods.  -> dict as abi.calib_sample returns it"""
    x = np.array(x0, dtype=np.float64)
    W, d = x.shape
    lp = loglik(x) + log_prior(x, lo, hi, kind)
    assert np.all(np.isfinite(lp))
    nacc = np.zeros(W, dtype=np.int32)
    tx, tl = [], []
    for g in range(first_step, first_step + nsteps):
        for half in (0, 1):
            y, aux, _, _ = propose(x, half, g, seed, a, lo, hi, kind)
            accept(x, lp, nacc, half, g, seed, y, aux, loglik(y))
        if g >= burn and (g + 1) % thin == 0:
            tx.append(x.copy())
            tl.append(lp.copy())
    return dict(trace_x=np.array(tx).reshape(len(tx), W, d), trace_lp=np.array(tl).reshape(len(tl), W), x_end=x, lp_end=lp,
                naccept=nacc, nrec=len(tx))


def autocorr_time(series):
    """integrated autocorrelation time with Sokal's window: tau(M) = 1 + 2 sum_{t=1..M} rho(t), the smallest M with M >= 5 tau(M)
    (the last M if none).  The autocovariance by direct sums, as the host layer forms it."""
    s = np.asarray(series, dtype=np.float64)
    n = s.size
    c = s - s.mean()
    c0 = float(c @ c)
    if n < 2 or not c0 > 0.0:
        return 1.0
    tau = 1.0
    for M in range(1, n):
        tau += 2.0 * float(c[:n - M] @ c[M:]) / c0
        if M >= 5.0 * tau:
            break
    return tau


# ---------------------------------------------------------------------------- targets of the statistical tests
def gauss_target(d):
    """a correlated Gaussian: sd_i = 0.5 + i / 2, correlation 0.6^|i - j|, mean i - 1"""
    sd = 0.5 + 0.5 * np.arange(d)
    mu = np.arange(d) - 1.0
    i = np.arange(d)
    cov = 0.6 ** np.abs(i[:, None] - i[None, :]) * sd[:, None] * sd[None, :]
    return mu, sd, cov


def gauss_errors(d, seed, W=64, nsteps=2000, burn=500):
    """the replica on gauss_target(d) under a wide box prior -> (error of the mean in units of the true sd, error of the
    covariance in units of sd_i sd_j), the largest over the entries"""
    mu, sd, cov = gauss_target(d)
    P = np.linalg.inv(cov)
    ll = lambda p: -0.5 * np.einsum("qi,ij,qj->q", p - mu, P, p - mu)
    lo, hi, kind = mu - 50.0 * sd, mu + 50.0 * sd, np.zeros(d, dtype=int)
    x0 = prior_draws(seed, W, mu - sd, mu + sd, kind)
    r = run(ll, x0, nsteps, lo, hi, kind, burn=burn, seed=seed)
    s = r["trace_x"].reshape(-1, d)
    return (np.abs(s.mean(axis=0) - mu) / sd).max(), (np.abs(np.cov(s.T).reshape(d, d) - cov) / np.outer(sd, sd)).max()


BOX_LO, BOX_HI = np.array([-1.0, 2.0]), np.array([3.0, 2.5])
BOX_Q = np.array([0.1, 0.25, 0.5, 0.75, 0.9])


def box_errors(seed, W=64, nsteps=2000, burn=500):
    """a flat likelihood under a uniform box prior in d = 2: the marginals' quantiles against the uniform's, in units of the
    box's width, the largest over coordinates and quantiles"""
    kind = np.zeros(2, dtype=int)
    x0 = prior_draws(seed, W, BOX_LO, BOX_HI, kind)
    r = run(lambda p: np.zeros(p.shape[0]), x0, nsteps, BOX_LO, BOX_HI, kind, burn=burn, seed=seed)
    s = r["trace_x"].reshape(-1, 2)
    assert np.all((s >= BOX_LO) & (s <= BOX_HI))
    q = np.quantile(s, BOX_Q, axis=0)
    return (np.abs(q - (BOX_LO + BOX_Q[:, None] * (BOX_HI - BOX_LO))) / (BOX_HI - BOX_LO)).max()


def ar1(phi, n, seed):
    """an AR(1) series with unit innovations from the sampler's own generator (Box-Muller on counters (i, 0, 0, 3))"""
    w = words(seed, np.arange(n), 0, 3)
    e = np.sqrt(-2.0 * np.log(uniform(w[0], w[1]))) * np.cos(2.0 * np.pi * uniform(w[2], w[3]))
    s = np.empty(n)
    s[0] = e[0] / np.sqrt(1.0 - phi * phi)
    for i in range(1, n):
        s[i] = phi * s[i - 1] + e[i]
    return s


AR1_N = 20000


# ---------------------------------------------------------------------------- a posterior tabulated on a regular grid
def grid_moments(pts, logp):
    """mean and sd per coordinate of the density exp(logp) tabulated at pts (n^d rows, the regular grid of n points per
    coordinate in 'ij' order), by the trapezoid rule"""
    d = pts.shape[1]
    n = int(round(pts.shape[0] ** (1.0 / d)))
    w1 = np.ones(n)
    w1[0] = w1[-1] = 0.5
    w = w1 if d == 1 else np.multiply.outer(w1, w1).ravel()
    p = w * np.exp(logp - logp.max())
    p /= p.sum()
    mean = p @ pts
    return mean, np.sqrt(p @ (pts - mean) ** 2)


def grid_loglik(ax, logp):
    """the tabulated log density, interpolated linearly (d = 1) or bilinearly (d = 2) inside the grid's box: a log-likelihood
    callable for run(); outside the box the prior rejects before the value matters"""
    n = ax.size
    if logp.size == n:
        return lambda p: np.interp(p[:, 0], ax, logp)
    T = logp.reshape(n, n)
    step = ax[1] - ax[0]

    def f(p):
        t = np.clip((p - ax[0]) / step, 0.0, n - 1.0)
        i = np.minimum(t.astype(int), n - 2)
        u = t - i
        i0, i1, u0, u1 = i[:, 0], i[:, 1], u[:, 0], u[:, 1]
        return ((1 - u0) * (1 - u1) * T[i0, i1] + u0 * (1 - u1) * T[i0 + 1, i1] + (1 - u0) * u1 * T[i0, i1 + 1] + u0 * u1 * T[i0 + 1, i1 + 1])
    return f


def grid_errors(logp, d, seed, W=64, nsteps=1500, burn=300):
    """the replica on a density tabulated over [0, 1]^d (tests/golden/sample_grid.npz), as the GPU end-to-end test runs the
    device: starts from the box [0.3, 0.6]^d -> (error of the mean in units of the grid's sd, relative error of the sd)"""
    n = int(round(logp.size ** (1.0 / d)))
    ax = np.linspace(0.0, 1.0, n)
    pts = ax[:, None] if d == 1 else np.stack(np.meshgrid(ax, ax, indexing="ij"), axis=-1).reshape(-1, 2)
    mean_g, sd_g = grid_moments(pts, logp)
    kind = np.zeros(d, dtype=int)
    x0 = prior_draws(seed, W, np.full(d, 0.3), np.full(d, 0.6), kind)
    r = run(grid_loglik(ax, logp), x0, nsteps, np.zeros(d), np.ones(d), kind, burn=burn, seed=seed)
    s = r["trace_x"].reshape(-1, d)
    return (np.abs(s.mean(axis=0) - mean_g) / sd_g).max(), (np.abs(s.std(axis=0) - sd_g) / sd_g).max()

# the asserting tests' own seed and the 16 the bars were measured over
TEST_SEED = 2010
BAR_SEEDS = tuple(range(1, 17))

# largest error over BAR_SEEDS times 2 (test_sampleref.measure_bars prints this dict)
BARS = {
    ("ar1", 0.5): 0.22733876234588468, ("ar1", 0.9): 0.5370352850168584,
    "box": 0.04255633622889632,
    ("gauss_mean", 1): 0.08150608815211235, ("gauss_cov", 1): 0.05175548230291094,
    ("gauss_mean", 3): 0.08733970876407146, ("gauss_cov", 3): 0.08595364451818921,
    ("gauss_mean", 5): 0.10756096222056592, ("gauss_cov", 5): 0.11808906573372968,
    # the tabulated posteriors of tests/golden/sample_grid.npz: error of the mean in units of the grid's sd, relative error of the sd
    ("grid_mean", "e2e1"): 0.07029348543077989, ("grid_sd", "e2e1"): 0.021396629473392926,
    ("grid_mean", "e2e2"): 0.21079539967548205, ("grid_sd", "e2e2"): 0.06349167570271287,
}
