"""The ensemble sampler on the device (gpemu_sample_*, gpemu_calib_sample, include/gpemu.h) against the numpy
replica tests/sampleref.py.

Bars of the primitives (the formats' precision, eps = 2^-52): a proposal within 4 eps of max(|x_j|, |z x_k|, |z x_j|); (d - 1)
log z within 8 eps relative (two logarithms of one ulp each, one product); a log prior within 8 eps of the sum of its absolute
terms, -inf exactly where the replica has it.  Accept decisions equal the replica's from the same inputs, a decision whose
margin |log u3 - log r| is below 1e-12 max(1, |log r|) left out -- the seeds here leave out none, which the test asserts.
The run is compared bit for bit with the caller-issued sequence of the public entries, with itself, with a split run and
with a small trace chunk.  End to end: the chain's mean and sd against the posterior tabulated on a grid by the existing
entries, inside sampleref.BARS (the replica's own largest error on the same tabulated density over 16 seeds, times 2)."""
import ctypes as C
import os

import numpy as np
import pytest

import sampleref as R
from madaiemulator_amd import abi, synth

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
GUARD = 64                                   # poisoned doubles (or ints) on either side of a device array
POISON = -7.25e300


@pytest.fixture(scope="module")
def ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.sample_release()
    gpu_ctx.calib_release()


class Guarded:
    """a device array between two poisoned guard regions"""

    def __init__(self, ctx, n, dtype=np.float64):
        self.ctx, self.n, self.dtype = ctx, n, np.dtype(dtype)
        self.poison = np.full(n + 2 * GUARD, POISON if self.dtype == np.float64 else -77, dtype=self.dtype)
        self.base = ctx.dev_alloc(self.poison.nbytes)
        self.ptr = C.c_void_p(self.base.value + GUARD * self.dtype.itemsize)
        ctx.upload(self.base, self.poison)

    def at(self, off):
        return C.c_void_p(self.ptr.value + off * self.dtype.itemsize)

    def put(self, a):
        a = np.ascontiguousarray(a, dtype=self.dtype).ravel()
        assert a.size == self.n
        self.ctx.upload(self.ptr, a)

    def get(self, shape=None):
        return self.ctx.download(self.ptr, (self.n,) if shape is None else shape, dtype=self.dtype)

    def guards_intact(self):
        all_ = self.ctx.download(self.base, (self.n + 2 * GUARD,), dtype=self.dtype)
        return (all_[:GUARD].tobytes() == self.poison[:GUARD].tobytes() and
                all_[GUARD + self.n:].tobytes() == self.poison[GUARD + self.n:].tobytes())

    def free(self):
        self.ctx.dev_free(self.base)


def far_apart_walkers(W, d, seed):
    """walker k near 1000 (k + 1) in every coordinate: a wrong partner moves a proposal by hundreds"""
    return 1000.0 * (1.0 + np.arange(W))[:, None] + np.arange(d)[None, :] + synth.uniform(seed, (W, d))


def prior_through(y, d):
    """a prior that the proposals y straddle: coordinate 0 (and 2) uniform with bounds that ARE proposals' coordinates (points
    exactly on lo and hi), the other even coordinates uniform and wide, the odd ones Gaussian"""
    lo, hi, kind = np.full(d, -1.0e7), np.full(d, 1.0e7), np.zeros(d, dtype=np.int32)
    kind[1::2] = R.GAUSS
    lo[1::2], hi[1::2] = 5.0e3, 2.0e3
    for c in (0, 2):
        if c < d:
            v = np.sort(y[:, c])
            if v.size >= 2 and v[0] < v[-1]:
                lo[c], hi[c] = v[(v.size - 1) // 4], v[max((3 * (v.size - 1)) // 4, (v.size - 1) // 4 + 1)]
                if not lo[c] < hi[c]:
                    lo[c], hi[c] = v[0], v[-1]
            else:
                lo[c], hi[c] = v[0] - 1.0, v[0]
    return lo, hi, kind


# ------------------------------------------------------------------ 1. propose
@pytest.mark.parametrize("d", [1, 2, 8, 33, 64])
@pytest.mark.parametrize("W", [2, 4, 6, 64, 130, 1026])
def test_propose_against_the_replica(ctx, W, d):
    h = W // 2
    x = far_apart_walkers(W, d, 100 * W + d)
    gx, gy, ga = Guarded(ctx, W * d), Guarded(ctx, h * d), Guarded(ctx, W)
    seed = 0x9e3779b97f4a7c15 ^ (W * 131 + d)
    try:
        gx.put(x)
        ninf = non = 0
        for half in (0, 1):
            for a in (2.0, 1.5):
                for step in (0, 2 ** 32 + 5):
                    wide = (np.full(d, -1e9), np.full(d, 1e9), np.zeros(d, dtype=np.int32))
                    y0, _, _, _ = R.propose(x, half, step, seed, a, *wide)
                    lo, hi, kind = prior_through(y0, d)
                    ctx.sample_set_prior(lo, hi, kind)
                    yr, auxr, j, z = R.propose(x, half, step, seed, a, lo, hi, kind)
                    gy.put(np.full(h * d, POISON)); ga.put(np.full(W, POISON))
                    ctx.sample_propose_dev(W, d, half, step, seed, a, gx.ptr, gy.ptr, ga.ptr)
                    y, aux = gy.get((h, d)), ga.get()
                    what = (W, d, half, a, step)
                    xj, xk = x[j], x[half * h:half * h + h]
                    scale = np.maximum(np.abs(xj), np.maximum(np.abs(z[:, None] * xk), np.abs(z[:, None] * xj)))
                    ey = (np.abs(y - yr) / scale).max() / EPS
                    assert ey <= 4.0, (what, ey)
                    if d == 1:
                        assert np.all(aux[:h] == 0.0) and not np.any(np.signbit(aux[:h])), what
                    else:
                        ez = np.abs(aux[:h] - auxr[:h])
                        assert np.all(ez <= 8.0 * EPS * np.abs(auxr[:h])), (what, ez.max())
                    inf = np.isneginf(auxr[h:])
                    assert np.array_equal(np.isneginf(aux[h:]), inf), what
                    tsum = np.abs(np.where(inf[:, None], 0.0, R.prior_terms(yr, lo, hi, kind))).sum(axis=1)
                    ep = np.abs(aux[h:][~inf] - auxr[h:][~inf])              # (a sum of zeros must be 0 itself)
                    assert np.all(ep <= 8.0 * EPS * tsum[~inf]), (what, ep.max())
                    ninf += int(inf.sum()); non += int((~inf).sum())
                    # points exactly on a bound count as inside: the bounds of coordinate 0 are proposals' coordinates
                    on = (yr[:, 0] == lo[0]) | (yr[:, 0] == hi[0])
                    assert on.any(), what
                    only0 = on & np.all((yr[:, 2:3] >= lo[2:3]) & (yr[:, 2:3] <= hi[2:3]), axis=1)
                    assert np.all(np.isfinite(aux[h:][only0])), what
                    assert gy.guards_intact() and ga.guards_intact() and gx.guards_intact(), what
                    assert gx.get((W, d)).tobytes() == x.tobytes(), what
        print(f"W {W} d {d}: {ninf} proposals outside the prior, {non} inside")
        assert non > 0 and (ninf > 0 or h < 4)
    finally:
        for g in (gx, gy, ga):
            g.free()


# ------------------------------------------------------------------ 2. accept
def accept_case(W, d, seed):
    rng = np.random.default_rng(seed)
    h = W // 2
    x, y = rng.standard_normal((W, d)), rng.standard_normal((h, d)) + 10.0
    lp = -np.abs(rng.standard_normal(W)) * 3.0
    aux = np.concatenate([rng.standard_normal(h) * (d > 1), -np.abs(rng.standard_normal(h))])
    ll = -np.abs(rng.standard_normal(h)) * 3.0
    nacc = rng.integers(0, 50, W).astype(np.int32)
    if h >= 8:
        ll[1], ll[3], ll[5] = np.nan, np.inf, -np.inf
        aux[h + 6] = -np.inf
    return x, y, lp, aux, ll, nacc


@pytest.mark.parametrize("W,d", [(2, 1), (6, 2), (16, 1), (64, 64), (130, 8), (1026, 33)])
def test_accept_against_the_replica(ctx, W, d):
    h = W // 2
    ctx.sample_set_prior(np.zeros(d), np.ones(d))
    gx, gy, ga, gl = Guarded(ctx, W * d), Guarded(ctx, h * d), Guarded(ctx, W), Guarded(ctx, h)
    glp, gn = Guarded(ctx, W), Guarded(ctx, W, np.int32)
    try:
        taken = 0
        for half in (0, 1):
            for step in (3, 2 ** 32 + 5):
                seed = 77 + W
                x, y, lp, aux, ll, nacc = accept_case(W, d, 1000 * W + 10 * d + half)
                _, lu, logr = R.accept_margin(lp, half, step, seed, aux, ll)
                with np.errstate(invalid="ignore"):
                    close = np.isfinite(logr) & (np.abs(lu - logr) <= 1e-12 * np.maximum(1.0, np.abs(logr)))   # (a non-finite log r is no close call)
                assert not close.any()                     # the replica leaves no decision out for these seeds
                xr, lpr, nr_ = x.copy(), lp.copy(), nacc.copy()
                take = R.accept(xr, lpr, nr_, half, step, seed, y, aux, ll)
                for g, a in ((gx, x), (gy, y), (ga, aux), (gl, ll), (glp, lp), (gn, nacc)):
                    g.put(a)
                ctx.sample_accept_dev(W, d, half, step, seed, gy.ptr, ga.ptr, gl.ptr, gx.ptr, glp.ptr, gn.ptr)
                xg, lpg, ng = gx.get((W, d)), glp.get(), gn.get()
                what = (W, d, half, step)
                moved = np.any(xg.view(np.uint64) != x.view(np.uint64), axis=1)
                base = half * h
                assert np.array_equal(moved[base:base + h], take), what
                assert xg.tobytes() == xr.tobytes() and lpg.tobytes() == lpr.tobytes() and np.array_equal(ng, nr_), what
                assert xg[base:base + h][take].tobytes() == y[take].tobytes()
                assert lpg[base:base + h][take].tobytes() == (ll + aux[h:])[take].tobytes()
                o = (1 - half) * h                       # the other half keeps its bits
                assert xg[o:o + h].tobytes() == x[o:o + h].tobytes() and lpg[o:o + h].tobytes() == lp[o:o + h].tobytes()
                assert np.array_equal(ng[o:o + h], nacc[o:o + h])
                if h >= 8:                                 # NaN, +inf, -inf log likelihood and a -inf prior reject
                    assert not take[[1, 3, 5, 6]].any()
                for g in (gx, gy, ga, gl, glp, gn):
                    assert g.guards_intact(), what
                assert gy.get().tobytes() == y.tobytes() and ga.get().tobytes() == aux.tobytes()
                taken += int(take.sum())
        assert W < 16 or 0 < taken < 4 * h
    finally:
        for g in (gx, gy, ga, gl, glp, gn):
            g.free()


# ------------------------------------------------------------------ 3. lock-step replay
def test_lock_step_replay(ctx):
    """50 steps of propose / accept over a Gaussian log density computed by the test; every half-step is checked from the
    device's own previous state"""
    W, d, seed, a = 16, 2, 4242, 2.0
    h = W // 2
    mu, sd, cov = R.gauss_target(d)
    P = np.linalg.inv(cov)
    ll = lambda p: -0.5 * np.einsum("qi,ij,qj->q", p - mu, P, p - mu)
    lo, hi, kind = np.array([-3.0, -30.0]), np.array([-0.6, 30.0]), np.zeros(d, dtype=np.int32)     # x_0 <= -0.6 cuts the target
    ctx.sample_set_prior(lo, hi, kind)
    x0 = R.prior_draws(seed, W, mu - sd, np.minimum(mu + sd, hi), kind)
    gx, gy, ga, gl, glp, gn = (Guarded(ctx, W * d), Guarded(ctx, h * d), Guarded(ctx, W), Guarded(ctx, h), Guarded(ctx, W),
                               Guarded(ctx, W, np.int32))
    try:
        gx.put(x0); gn.put(np.zeros(W, dtype=np.int32))
        gl.put(ll(x0[:h])); ctx.sample_logpost_dev(h, d, gx.ptr, gl.ptr, glp.ptr)
        gl.put(ll(x0[h:])); ctx.sample_logpost_dev(h, d, gx.at(h * d), gl.ptr, glp.at(h))
        lp = glp.get()
        want = ll(x0) + R.log_prior(x0, lo, hi, kind)
        assert np.all(np.abs(lp - want) <= 8 * EPS * (np.abs(ll(x0)) + np.abs(R.prior_terms(x0, lo, hi, kind)).sum(axis=1)))
        x, nacc = x0.copy(), np.zeros(W, dtype=np.int32)
        rejected_outside = 0
        for step in range(50):
            for half in (0, 1):
                ctx.sample_propose_dev(W, d, half, step, seed, a, gx.ptr, gy.ptr, ga.ptr)
                y, aux = gy.get((h, d)), ga.get()
                yr, auxr, j, z = R.propose(x, half, step, seed, a, lo, hi, kind)
                assert y.tobytes() == yr.tobytes(), (step, half)      # +, *, / alone: the same bits
                assert np.all(np.abs(aux[:h] - auxr[:h]) <= 8 * EPS * np.abs(auxr[:h]))
                assert np.array_equal(np.isneginf(aux[h:]), np.isneginf(auxr[h:]))
                fin = np.isfinite(auxr[h:])
                assert np.all(np.abs(aux[h:][fin] - auxr[h:][fin]) <= 8 * EPS * np.abs(R.prior_terms(yr, lo, hi, kind)).sum(axis=1)[fin])
                lly = ll(y)
                gl.put(lly)
                # the replica's decision from the device's own y, aux and previous state
                _, lu, logr = R.accept_margin(lp, half, step, seed, aux, lly)
                with np.errstate(invalid="ignore"):
                    assert not np.any(np.isfinite(logr) & (np.abs(lu - logr) <= 1e-12 * np.maximum(1.0, np.abs(logr)))), (step, half)
                take = R.accept(x, lp, nacc, half, step, seed, y, aux, lly)
                rejected_outside += int(np.isneginf(aux[h:]).sum())
                ctx.sample_accept_dev(W, d, half, step, seed, gy.ptr, ga.ptr, gl.ptr, gx.ptr, glp.ptr, gn.ptr)
                assert gx.get((W, d)).tobytes() == x.tobytes() and glp.get().tobytes() == lp.tobytes(), (step, half, take)
                assert np.array_equal(gn.get(), nacc)
        print("accepted", nacc.sum(), "of", 50 * W, "; proposals outside the box:", rejected_outside)
        assert 0.2 * 50 * W < nacc.sum() < 0.95 * 50 * W and rejected_outside > 0
        assert np.all((x >= lo) & (x <= hi))
    finally:
        for g in (gx, gy, ga, gl, glp, gn):
            g.free()


# ------------------------------------------------------------------ 4. the run
class Emulator:
    """nr component contexts with a prediction set-up on a synthetic multi-output model, and the calibration set-up and a uniform
    prior on the design's range on the observation context"""

    def __init__(self, obs, N, d, nr, nt, xs, seed):
        X, y = synth.design(N, d, seed)
        Y = synth.multi_outputs(X, y, nt)
        Z, evals, evecs, ybar = synth.pca_zmatrix(Y, 1.0) if nt > 1 else (((Y - Y.mean(0)) / Y.std(0)), Y.var(0), np.ones((1, 1)), Y.mean(0))
        self.N, self.d, self.nr, self.nt, self.obs = N, d, nr, nt, obs
        self.A = np.ascontiguousarray(evecs[:, :nr] * np.sqrt(evals[:nr]))
        self.ybar = ybar
        self.comps = []
        th = synth.default_thetas(abi.POWEREXP, d)
        for c in range(nr):
            cc = abi.Context(0)
            cc.set_model(abi.POWEREXP, 1, X, np.ascontiguousarray(Z[:, c]))
            _, rc = cc.predict_setup(th)
            assert rc == abi.OK
            self.comps.append(cc)
        # observations: the outputs at the point xs in every coordinate, shifted, with standard deviations a fifth of the outputs'
        # spread (d = 1: y is a sine of period 1 and 0.25 its maximum, so that the posterior has ONE mode: the stretch move
        # cannot carry a walker across a deep valley, and a chain of this length would not equilibrate two)
        xs = np.full((1, d), xs)
        m = np.array([cc.predict(xs)[0][0] for cc in self.comps])
        self.sd = 0.2 * Y.std(axis=0) + 0.05
        self.z = ybar + self.A @ m + 0.3 * self.sd * np.cos(np.arange(nt))
        self.lo, self.hi = np.zeros(d), np.ones(d)
        self.install()

    def install(self):
        rc, info = self.obs.calib_setup(self.ybar, self.A, self.z, sd=self.sd)
        assert rc == abi.OK and info == 0
        self.obs.sample_set_prior(self.lo, self.hi)

    def starts(self, W, seed):
        return R.prior_draws(seed, W, np.full(self.d, 0.3), np.full(self.d, 0.6), np.zeros(self.d, dtype=int))

    def close(self):
        for cc in self.comps:
            cc.close()


EMULATORS = {"small": (96, 2, 2, 5, 0.45), "wide": (130, 5, 3, 7, 0.45), "e2e1": (48, 1, 1, 3, 0.25), "e2e2": (48, 2, 1, 3, 0.45)}
_emus = {}


@pytest.fixture(scope="module")
def emulator(ctx):
    def get(key):
        if key not in _emus:
            _emus[key] = Emulator(ctx, *EMULATORS[key], seed=31 + len(key))
        _emus[key].install()
        return _emus[key]
    yield get
    for e in _emus.values():
        e.close()
    _emus.clear()


RUNS = {"small": dict(W=12, nsteps=40, burn=4, thin=3), "wide": dict(W=66, nsteps=20, burn=0, thin=1)}


def by_public_entries(em, x0, nsteps, burn, thin, seed, first_step=0, a=2.0):
    """the run as a caller issues it: propose, predict_batch_dev per component, calib_eval_dev, accept, a sync between them"""
    obs, comps, d, nr = em.obs, em.comps, em.d, em.nr
    W = x0.shape[0]
    h = W // 2
    bufs = [obs.dev_alloc(8 * n) for n in (W * d, W, h * d, W, nr * h, nr * h, 5 * h)] + [obs.dev_alloc(4 * W), obs.dev_alloc(4 * h)]
    dx, dlp, dy, daux, dm, dv, ds, dn, dw = bufs
    off = lambda p, n: C.c_void_p(p.value + 8 * n)

    def loglik(pts):
        for c, cc in enumerate(comps):
            cc.predict_dev(h, pts, off(dm, c * h), off(dv, c * h))
            cc.sync()
        obs.calib_eval_dev(h, dm, dv, h, ds, dw)
        obs.sync()

    try:
        obs.upload(dx, x0); obs.upload(dn, np.zeros(W, dtype=np.int32))
        for half in (0, 1):
            loglik(off(dx, half * h * d))
            obs.sample_logpost_dev(h, d, off(dx, half * h * d), off(ds, h), off(dlp, half * h))
            obs.sync()
        tx, tl = [], []
        for g in range(first_step, first_step + nsteps):
            for half in (0, 1):
                obs.sample_propose_dev(W, d, half, g, seed, a, dx, dy, daux)
                obs.sync()
                loglik(dy)
                obs.sample_accept_dev(W, d, half, g, seed, dy, daux, off(ds, h), dx, dlp, dn)
                obs.sync()
            if g >= burn and (g + 1) % thin == 0:
                tx.append(obs.download(dx, (W, d))); tl.append(obs.download(dlp, (W,)))
        return dict(trace_x=np.array(tx).reshape(len(tx), W, d), trace_lp=np.array(tl).reshape(len(tl), W),
                    x_end=obs.download(dx, (W, d)), lp_end=obs.download(dlp, (W,)), naccept=obs.download(dn, (W,), dtype=np.int32),
                    nrec=len(tx))
    finally:
        for p in bufs:
            obs.dev_free(p)


def same_bits(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("trace_x", "trace_lp", "x_end", "lp_end", "naccept")) and a["nrec"] == b["nrec"]


@pytest.mark.parametrize("key", ["small", "wide"])
def test_run_equals_the_public_entries_issued_one_by_one(emulator, key):
    em, r = emulator(key), RUNS[key]
    x0 = em.starts(r["W"], 5)
    got = abi.calib_sample(em.comps, em.obs, x0, r["nsteps"], burn=r["burn"], thin=r["thin"], seed=99)
    want = by_public_entries(em, x0, r["nsteps"], r["burn"], r["thin"], 99)
    nrec = sum(1 for g in range(r["nsteps"]) if g >= r["burn"] and (g + 1) % r["thin"] == 0)
    assert got["nrec"] == nrec and got["trace_x"].shape == (nrec, r["W"], em.d)
    assert same_bits(got, want)
    assert np.all(np.isfinite(got["trace_lp"])) and np.all((got["trace_x"] >= 0.0) & (got["trace_x"] <= 1.0))
    acc = got["naccept"].sum() / (r["nsteps"] * r["W"])
    print(key, "acceptance", acc)
    assert 0.05 < acc < 0.95 and got["naccept"].max() <= r["nsteps"]
    assert got["trace_x"][-1].tobytes() != got["trace_x"][0].tobytes()


@pytest.mark.parametrize("key", ["small", "wide"])
def test_run_is_repeatable_and_depends_on_the_seed(emulator, key):
    em, r = emulator(key), RUNS[key]
    x0 = em.starts(r["W"], 5)
    kw = dict(burn=r["burn"], thin=r["thin"])
    a, b = abi.calib_sample(em.comps, em.obs, x0, r["nsteps"], seed=99, **kw), abi.calib_sample(em.comps, em.obs, x0, r["nsteps"], seed=99, **kw)
    c = abi.calib_sample(em.comps, em.obs, x0, r["nsteps"], seed=100, **kw)
    assert same_bits(a, b) and a["trace_x"].tobytes() != c["trace_x"].tobytes()
    # NULL traces are accepted: the same end state
    n = abi.calib_sample(em.comps, em.obs, x0, r["nsteps"], seed=99, trace=False, **kw)
    assert n["trace_x"] is None and n["nrec"] == a["nrec"]
    assert all(n[k].tobytes() == a[k].tobytes() for k in ("x_end", "lp_end", "naccept"))


@pytest.mark.parametrize("key", ["small", "wide"])
def test_split_run_and_small_chunks(emulator, key):
    em, W = emulator(key), RUNS[key]["W"]
    x0 = em.starts(W, 6)
    kw = dict(burn=0, thin=5, seed=7)
    whole = abi.calib_sample(em.comps, em.obs, x0, 40, **kw)
    first = abi.calib_sample(em.comps, em.obs, x0, 25, **kw)
    second = abi.calib_sample(em.comps, em.obs, first["x_end"], 15, first_step=25, **kw)
    assert first["nrec"] == 5 and second["nrec"] == 3 and whole["nrec"] == 8
    assert np.concatenate([first["trace_x"], second["trace_x"]]).tobytes() == whole["trace_x"].tobytes()
    assert np.concatenate([first["trace_lp"], second["trace_lp"]]).tobytes() == whole["trace_lp"].tobytes()
    assert second["x_end"].tobytes() == whole["x_end"].tobytes() and second["lp_end"].tobytes() == whole["lp_end"].tobytes()
    assert np.array_equal(first["naccept"] + second["naccept"], whole["naccept"])
    em.obs.test_sample_chunk(3)
    try:
        chunked = abi.calib_sample(em.comps, em.obs, x0, 40, **kw)
    finally:
        em.obs.test_sample_chunk(0)
    assert same_bits(chunked, whole)


# ------------------------------------------------------------------ 5. end to end against a tabulated posterior
GRID = {"e2e1": 4001, "e2e2": 201}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sample_grid.npz")


def tabulate(em, n):
    """log posterior on the regular grid of n points per coordinate over the prior's box, by predict_batch and calib_eval"""
    ax = np.linspace(0.0, 1.0, n)
    pts = ax[:, None] if em.d == 1 else np.stack(np.meshgrid(ax, ax, indexing="ij"), axis=-1).reshape(-1, 2)
    mv = [cc.predict(pts) for cc in em.comps]
    stat, _ = em.obs.calib_eval(np.array([m for m, _ in mv]), np.array([v for _, v in mv]), M=pts.shape[0])
    return ax, pts, stat[1] + R.log_prior(pts, em.lo, em.hi, np.zeros(em.d, dtype=int))


@pytest.mark.parametrize("key", ["e2e1", "e2e2"])
def test_chain_against_the_tabulated_posterior(emulator, key):
    em = emulator(key)
    ax, pts, logp = tabulate(em, GRID[key])
    out = os.environ.get("GPEMU_SAMPLE_GRID_OUT")             # how tests/golden/sample_grid.npz was written
    if out:
        np.save(os.path.join(out, key + ".npy"), logp)
    stored = np.load(GOLDEN)[key]
    # the bars were measured on the stored table: this device's table must be that density
    assert np.abs(logp - stored).max() <= 1e-9 * np.maximum(1.0, np.abs(stored)).max()
    mean_g, sd_g = R.grid_moments(pts, logp)
    r = abi.calib_sample(em.comps, em.obs, em.starts(64, R.TEST_SEED), 1500, burn=300, seed=R.TEST_SEED)
    s = r["trace_x"].reshape(-1, em.d)
    em_, es = (np.abs(s.mean(axis=0) - mean_g) / sd_g).max(), (np.abs(s.std(axis=0) - sd_g) / sd_g).max()
    print(f"{key}: grid mean {mean_g} sd {sd_g}; chain mean error {em_:.4f}/{R.BARS['grid_mean', key]:.4f} sd units, "
          f"sd error {es:.4f}/{R.BARS['grid_sd', key]:.4f} relative; acceptance {r['naccept'].sum() / (1500 * 64):.3f}")
    assert em_ <= R.BARS["grid_mean", key] and es <= R.BARS["grid_sd", key]


# ------------------------------------------------------------------ 6. error codes
def test_error_codes(ctx, emulator):
    L, h_ = ctx.L, ctx.h
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))
    d = 3
    lo, hi, kind = np.zeros(d), np.ones(d), np.array([0, 1, 0], dtype=np.int32)
    prior = lambda d=d, kind=kind, lo=lo, hi=hi, h=h_: L.gpemu_sample_set_prior(h, d, ip(kind), dp(lo), dp(hi))
    ctx.sample_release()
    W = 8
    bufs = [ctx.dev_alloc(8 * 64 * 8) for _ in range(6)]
    dx, dy, da, dl, dlp, dn = bufs
    prop = lambda W=W, d=d, half=0, a=2.0, x=dx, y=dy, aux=da, h=h_: L.gpemu_sample_propose_dev(h, W, d, half, 0, 1, a, x, y, aux)
    acc = lambda W=W, d=d, half=0, y=dy, aux=da, ll=dl, x=dx, lp=dlp, n=dn, h=h_: \
        L.gpemu_sample_accept_dev(h, W, d, half, 0, 1, y, aux, ll, x, lp, n)
    post = lambda M=4, d=d, x=dx, ll=dl, lp=dlp, h=h_: L.gpemu_sample_logpost_dev(h, M, d, x, ll, lp)
    try:
        ctx.upload(dx, np.zeros(64 * 8)); ctx.upload(dl, np.zeros(64 * 8)); ctx.upload(dlp, np.zeros(64 * 8)); ctx.upload(dn, np.zeros(64 * 8))
        assert prop() == abi.ERR_STATE and acc() == abi.ERR_STATE and post() == abi.ERR_STATE          # no prior
        # the prior's checks
        assert prior(h=None) == abi.ERR_ARG and prior(lo=None) == abi.ERR_ARG and prior(hi=None) == abi.ERR_ARG
        assert prior(d=0) == abi.ERR_ARG and prior(d=65) == abi.ERR_ARG
        assert prior(kind=np.array([0, 2, 0], dtype=np.int32)) == abi.ERR_ARG
        assert prior(hi=np.array([1.0, 1.0, 0.0])) == abi.ERR_ARG                  # lo >= hi on a uniform coordinate
        assert prior(hi=np.array([1.0, 0.0, 1.0])) == abi.ERR_ARG                  # sd <= 0
        assert prior(hi=np.array([1.0, -1.0, 1.0])) == abi.ERR_ARG
        assert prior(lo=np.array([0.0, np.nan, 0.0])) == abi.ERR_ARG and prior(hi=np.array([np.inf, 1.0, 1.0])) == abi.ERR_ARG
        assert prop() == abi.ERR_STATE                                             # a failed call leaves none
        assert prior(lo=np.array([0.0, 5.0, 0.0])) == abi.OK                       # a Gaussian's mean may exceed its sd
        assert prior(kind=None) == abi.OK and prior() == abi.OK
        assert prop() == abi.OK and acc() == abi.OK and post() == abi.OK
        assert prop(d=2) == abi.ERR_STATE and acc(d=2) == abi.ERR_STATE and post(d=2) == abi.ERR_STATE   # a prior of another d
        for f in (prop, acc):
            assert f(h=None) == abi.ERR_ARG and f(W=7) == abi.ERR_ARG and f(W=0) == abi.ERR_ARG and f(W=-2) == abi.ERR_ARG
            assert f(d=0) == abi.ERR_ARG and f(d=65) == abi.ERR_ARG and f(half=2) == abi.ERR_ARG and f(half=-1) == abi.ERR_ARG
            assert f(y=None) == abi.ERR_ARG and f(aux=None) == abi.ERR_ARG and f(x=None) == abi.ERR_ARG
        assert prop(a=1.0) == abi.ERR_ARG and prop(a=0.5) == abi.ERR_ARG and prop(a=np.nan) == abi.ERR_ARG and prop(a=np.inf) == abi.ERR_ARG
        assert acc(ll=None) == abi.ERR_ARG and acc(lp=None) == abi.ERR_ARG and acc(n=None) == abi.ERR_ARG
        assert post(h=None) == abi.ERR_ARG and post(M=0) == abi.ERR_ARG and post(d=0) == abi.ERR_ARG
        assert post(x=None) == abi.ERR_ARG and post(ll=None) == abi.ERR_ARG and post(lp=None) == abi.ERR_ARG
        ctx.sync()
        # the prior survives gpemu_set_model; after the release: GPEMU_ERR_STATE again
        X, y = synth.design(70, 2, 5)
        ctx.set_model(abi.POWEREXP, 1, X, y)
        assert prop() == abi.OK
        ctx.sample_release()
        assert prop() == abi.ERR_STATE
        assert L.gpemu_sample_release(None) == abi.ERR_ARG and L.gpemu_test_sample_chunk(None, 1) == abi.ERR_ARG
        assert L.gpemu_test_sample_chunk(h_, -1) == abi.ERR_ARG
    finally:
        ctx.sync()
        for p in bufs:
            ctx.dev_free(p)

    # the run
    em = emulator("small")
    W, dd = 12, em.d
    x0 = em.starts(W, 5)
    hs = (C.c_void_p * em.nr)(*[c.h for c in em.comps])
    tx, tl = np.empty((40, W, dd)), np.empty((40, W))
    xe, le, na, nrec = np.empty((W, dd)), np.empty(W), np.empty(W, dtype=np.int32), C.c_int(0)

    def run(comp=hs, nr=em.nr, obs=ctx.h, W=W, nsteps=4, burn=0, thin=1, a=2.0, x0=x0, xe=xe, le=le, na=na, nrec=C.byref(nrec), args=True):
        sa = abi.SampleArgs(nwalkers=W, nsteps=nsteps, burn=burn, thin=thin, seed=1, first_step=0, a=a)
        return L.gpemu_calib_sample(comp, nr, obs, C.byref(sa) if args else None, dp(x0), dp(tx), dp(tl), dp(xe), dp(le), ip(na), nrec)

    assert run() == abi.OK and nrec.value == 4
    assert run(comp=None) == abi.ERR_ARG and run(obs=None) == abi.ERR_ARG and run(args=False) == abi.ERR_ARG
    assert run(x0=None) == abi.ERR_ARG and run(xe=None) == abi.ERR_ARG and run(le=None) == abi.ERR_ARG and run(na=None) == abi.ERR_ARG
    assert run(nrec=None) == abi.ERR_ARG
    assert run(nr=0) == abi.ERR_ARG and run(W=11) == abi.ERR_ARG and run(W=0) == abi.ERR_ARG
    assert run(W=4) == abi.ERR_ARG                                                # W/2 < d + 1
    assert run(W=6) == abi.OK                                                     # W/2 = d + 1
    assert run(nsteps=0) == abi.ERR_ARG and run(burn=-1) == abi.ERR_ARG and run(thin=0) == abi.ERR_ARG
    assert run(a=1.0) == abi.ERR_ARG and run(a=np.nan) == abi.ERR_ARG
    bad = x0.copy(); bad[3, 0] = 1.5                                              # outside the prior: a non-finite start
    assert run(x0=bad) == abi.ERR_ARG
    bad = x0.copy(); bad[7, 1] = np.nan
    assert run(x0=bad) == abi.ERR_ARG
    assert run(nr=1) == abi.ERR_STATE                                             # the calibration set-up has nr = 2
    other = emulator("wide")                                                      # (installs its own set-up and prior on ctx)
    mixed = (C.c_void_p * 2)(em.comps[0].h, other.comps[0].h)
    assert run(comp=mixed) in (abi.ERR_ARG,)                                      # components with different d
    em.install()
    fresh = abi.Context(0)
    try:
        nosetup = (C.c_void_p * 2)(em.comps[0].h, fresh.h)
        assert run(comp=nosetup) == abi.ERR_STATE                                 # no prediction set-up
        assert run(obs=fresh.h) == abi.ERR_STATE                                  # no calibration set-up
    finally:
        fresh.close()
    if abi.load().gpemu_device_count() > 1:
        far = abi.Context(1)
        try:
            X, y = synth.design(96, 2, 3)
            far.set_model(abi.POWEREXP, 1, X, y)
            assert far.predict_setup(synth.default_thetas(abi.POWEREXP, 2))[1] == abi.OK
            assert run(comp=(C.c_void_p * 2)(em.comps[0].h, far.h)) == abi.ERR_ARG
        finally:
            far.close()
    ctx.sample_release()
    assert run() == abi.ERR_STATE                                                 # no prior
    ctx.sample_set_prior(np.zeros(3), np.ones(3))
    assert run() == abi.ERR_STATE                                                 # a prior of another d
    em.install()
    ctx.calib_release()
    assert run() == abi.ERR_STATE                                                 # no calibration set-up
    em.install()
    assert run() == abi.OK
