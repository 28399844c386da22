"""K-fold / leave-group-out validation from the resident prediction state (gpemu_lgo, include/gpemu.h).

The device evaluates, for every group B of a call, the block form of gpemu_loo's closed form: P_BB = (C^-1)_BB - W_B Q W_B^T
from the gathered columns of L^-1, its lock-step Cholesky factorisation with inverse rows, cov_B = P_BB^-1,
mean_B = y_B - cov_B gamma_B, the decorrelated errors, their norm, log det cov_B and the joint log density.  It is compared
with what the formula stands for: LAPACK refits on the other N - b points with the joint covariance at x_B (tests/lgoref.py,
which checks itself against the closed form through LAPACK's explicit inverse to 1e-10 first), and on two groups per
configuration with the oracle's own alloc_emulator_struct on the other points (mean and variance).

Bars: the project's parity bar RTOL = 1e-8 in lgoref's six measures.  The oracle's k-vector zeroes covariances below 1e-10;
every comparison with oracle refits asserts first that no off-diagonal element of C is that small."""
import numpy as np
import pytest

import lgoref
import looref
from madaiemulator_amd import abi
from oracle import oracle as O
from test_gpu_loo import setup, small_model

RTOL = lgoref.RTOL
CONFIGS = [(1, 1, 150, 3), (3, 1, 150, 3), (2, 0, 120, 2), (1, 2, 130, 4)]
RAGGED = [1, 2, 17, 33, 64]
EDGES = [1, 63, 64, 65, 129, 191]

pytestmark = pytest.mark.gpu

_refs = {}


def reference(key, kind, order, X, y, th, group):
    """lgoref.reference, computed once per input and shared (never modified)"""
    if key not in _refs:
        _refs[key] = lgoref.reference(kind, order, X, y, th, group)
    return _refs[key]


def check(what, res, ref, group):
    assert res["status"] == abi.OK and not res["info"].any(), (what, res["status"], res["info"])
    out = group < 0
    for k in ("mean", "var", "werr"):
        assert np.array_equal(np.isnan(res[k]), out), (what, k)
    assert np.all(res["var"][~out] > 0)
    e = lgoref.worst([lgoref.errors(g, r, ref["kappa"]) for g, r in zip(lgoref.split(res, ref["groups"]), ref["per_group"])])
    print(f"{what}: {', '.join(f'{k} {v:.2e}' for k, v in e.items())}  (bar {RTOL:.0e}; reference's own {max(ref['ref_err'].values()):.1e})")
    assert all(v < RTOL for v in e.values()), (what, e)


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("mean", "var", "werr", "maha", "logdet", "logpdf", "info"))


def oracle_group(kind, order, X, y, th, B):
    """mean and variance at the members of B from the oracle's own set-up on the other points"""
    keep = np.ones(len(y), dtype=bool)
    keep[B] = False
    e = O.Emulator(kind, order, X[keep], y[keep], th)
    assert e.status == 0
    m, v, _ = e.emulate(X[B])
    return m, v


# ------------------------------------------------------------------ 1. every group against refits
@pytest.mark.parametrize("kind,order,N,d", CONFIGS)
def test_every_group_against_refits(gpu_ctx, kind, order, N, d):
    X, y, th = small_model(kind, order, N, d)
    setup(gpu_ctx, kind, order, X, y, th)
    assert looref.min_offdiag(O.cov_matrix(kind, X, th)) >= looref.CLAMP
    for how, group in (("folds", lgoref.folds(N, 5, seed=7)), ("ragged", lgoref.ragged(N, RAGGED, 11))):
        ref = reference((kind, order, N, d, how), kind, order, X, y, th, group)
        res = gpu_ctx.lgo(group)
        check(f"kind {kind} order {order} N {N} d {d} {how}", res, ref, group)
        for g in (0, len(ref["groups"]) - 1):
            B = ref["groups"][g]
            mo, vo = oracle_group(kind, order, X, y, th, B)
            em, ev = looref.errors(res["mean"][B], res["var"][B], mo, vo, ref["kappa"])
            print(f"  group {g} (b = {len(B)}) against the oracle's refit: mean {em:.2e} var {ev:.2e}")
            assert em < RTOL and ev < RTOL


# ------------------------------------------------------------------ 2. granule edges
@pytest.mark.parametrize("kind", [1, 3])
def test_granule_edges(gpu_ctx, kind):
    """group sizes around the 64-row padding granule and the 128-column pieces of the finishing pass; bp = 192"""
    order, N, d = 1, 513, 3
    X, y, th = small_model(kind, order, N, d)
    group = lgoref.ragged(N, EDGES, 13)
    assert (group >= 0).all()
    ref = reference((kind, "edges"), kind, order, X, y, th, group)
    setup(gpu_ctx, kind, order, X, y, th)
    check(f"kind {kind} N 513 sizes {EDGES}", gpu_ctx.lgo(group), ref, group)


def test_three_folds_of_1000(gpu_ctx):
    """bp = 384: the lock-step batch goes through a 256-column group of the recursion"""
    kind, order, N, d = 1, 1, 1000, 3
    X, y, th = small_model(kind, order, N, d)
    group = lgoref.folds(N, 3, seed=17)
    ref = reference("three folds", kind, order, X, y, th, group)
    setup(gpu_ctx, kind, order, X, y, th)
    check("N 1000 three folds", gpu_ctx.lgo(group), ref, group)


# ------------------------------------------------------------------ 3. chunking
def test_every_point_its_own_group(gpu_ctx):
    """130 groups of one: three chunks (64, 64, 2), bp = 64; equals gpemu_loo and the refits"""
    kind, order, N, d = 1, 1, 130, 3
    X, y, th = small_model(kind, order, N, d)
    group = np.arange(N, dtype=np.int32)
    ref = reference("ones", kind, order, X, y, th, group)
    setup(gpu_ctx, kind, order, X, y, th)
    res = gpu_ctx.lgo(group)
    check("130 groups of one", res, ref, group)
    m, v = gpu_ctx.loo()
    em, ev = looref.errors(res["mean"], res["var"], m, v, ref["kappa"])
    print(f"130 groups of one against gpemu_loo: mean {em:.2e} var {ev:.2e}")
    assert em < RTOL and ev < RTOL
    gpu_ctx.prof_begin(abi.PROF_LGO)
    gpu_ctx.lgo(group)
    p = gpu_ctx.prof_end()
    Np, bp = 192, 64
    want = sum(8.0 * nbc * bp * (Np + (2 * bp + 64) + (bp / 2 + 4)) for nbc in (64, 64, 2))
    assert p["n"] == 9 and p["bytes"] == want, (p, want)


# ------------------------------------------------------------------ 4. unsorted and relabelled groups
def test_relabelled_groups(gpu_ctx):
    kind, order, N, d = 3, 1, 150, 3
    X, y, th = small_model(kind, order, N, d)
    group = lgoref.ragged(N, RAGGED, 11)
    perm = np.array([3, 0, 4, 1, 2], dtype=np.int32)
    relab = np.where(group >= 0, perm[np.maximum(group, 0)], -1).astype(np.int32)
    setup(gpu_ctx, kind, order, X, y, th)
    a, b = gpu_ctx.lgo(group), gpu_ctx.lgo(relab)
    assert a["status"] == abi.OK and b["status"] == abi.OK
    kappa = O.cov(kind, X[0], X[0], th)
    ins = group >= 0
    scale = {"mean": max(1.0, float(np.max(np.abs(a["mean"][ins])))), "var": kappa, "werr": max(1.0, float(np.max(np.abs(a["werr"][ins]))))}
    for k in ("mean", "var", "werr"):
        assert np.array_equal(np.isnan(a[k]), ~ins) and np.array_equal(np.isnan(b[k]), ~ins)
        assert np.max(np.abs(a[k][ins] - b[k][ins])) < RTOL * scale[k], k
    sizes = np.array(RAGGED, dtype=np.float64)
    assert np.max(np.abs(a["maha"] - b["maha"][perm]) / np.maximum(1.0, a["maha"])) < RTOL
    assert np.max(np.abs(a["logdet"] - b["logdet"][perm]) / sizes) < RTOL
    assert np.max(np.abs(a["logpdf"] - b["logpdf"][perm]) / np.maximum(1.0, np.abs(a["logpdf"]))) < RTOL


# ------------------------------------------------------------------ 5. bits
def test_same_bits(gpu_ctx):
    kind, order, N, d = 1, 1, 321, 3
    X, y, th = small_model(kind, order, N, d)
    group = lgoref.ragged(N, [70, 5, 128, 64, 1], 19)
    ng = 5
    setup(gpu_ctx, kind, order, X, y, th)
    Xq = X[:9] + 0.01
    before = (gpu_ctx.predict(Xq), gpu_ctx.loo(), gpu_ctx.cinverse())
    a = gpu_ctx.lgo(group)
    b = gpu_ctx.lgo(group)
    assert a["status"] == abi.OK and same_bits(a, b)
    # the device-pointer entry
    buf = gpu_ctx.dev_alloc((3 * N + 3 * ng) * 8 + ng * 4)
    try:
        base = buf.value
        gpu_ctx.lgo_dev(group, ng, base, base + N * 8, base + 2 * N * 8, base + 3 * N * 8, base + (3 * N + 3 * ng) * 8)
        pts = gpu_ctx.download(buf, (3, N))
        st = gpu_ctx.download(abi.C.c_void_p(base + 3 * N * 8), (3, ng))
        info = gpu_ctx.download(abi.C.c_void_p(base + (3 * N + 3 * ng) * 8), (ng,), dtype=np.int32)
    finally:
        gpu_ctx.dev_free(buf)
    dev = dict(mean=pts[0], var=pts[1], werr=pts[2], maha=st[0], logdet=st[1], logpdf=st[2], info=info)
    assert same_bits(a, dev)
    # nothing another entry reads has changed, before or after the buffers are given back
    for stage in ("after a call", "after lgo_release"):
        after = (gpu_ctx.predict(Xq), gpu_ctx.loo(), gpu_ctx.cinverse())
        for x, z in zip(before, after):
            for p, q in zip(x, z) if isinstance(x, tuple) else [(x, z)]:
                assert np.array_equal(p, q), stage
        gpu_ctx.lgo_release()
    assert same_bits(a, gpu_ctx.lgo(group))


def test_setup_by_batch_same_bits():
    """components set up by gpemu_predict_setup_batch (the later ones own no factorisation workspace) against contexts set up alone"""
    kind, order, N, d = 1, 1, 321, 3
    X, y, th = small_model(kind, order, N, d)
    group = lgoref.folds(N, 4, seed=23)
    ys = [y, np.cos(3.0 * y) + 0.5]
    ths = [th, th + 0.05]
    ctxs = [abi.Context(0) for _ in ys]
    try:
        for c, yc in zip(ctxs, ys):
            c.set_model(kind, order, X, yc)
        _, _, status, rc = abi.predict_setup_batch(ctxs, np.array(ths))
        assert rc == abi.OK and not status.any()
        for c, yc, tc in zip(ctxs, ys, ths):
            alone = abi.Context(0)
            try:
                setup(alone, kind, order, X, yc, tc)
                ra = alone.lgo(group)
            finally:
                alone.close()
            rb = c.lgo(group)
            assert ra["status"] == abi.OK and same_bits(ra, rb)
            ci = c.cinverse()                        # (the later components factor again for it: still works)
            assert np.all(np.isfinite(ci))
    finally:
        for c in ctxs:
            c.close()


# ------------------------------------------------------------------ 6. errors
def _rc(ctx, ng, group, n_out=None, mean=True, var=True, info=True):
    group = None if group is None else np.ascontiguousarray(group, dtype=np.int32)
    n = len(group) if n_out is None else n_out
    m, v, i = np.empty(max(n, 1)), np.empty(max(n, 1)), np.zeros(max(ng, 1, n), dtype=np.int32)
    ip = abi.C.POINTER(abi.C.c_int)
    return ctx.L.gpemu_lgo(ctx.h, ng, None if group is None else group.ctypes.data_as(ip), abi._p(m) if mean else None,
                           abi._p(v) if var else None, None, None, None, None, i.ctypes.data_as(ip) if info else None)


def test_errors(gpu_ctx):
    kind, order, N, d = 1, 1, 90, 3
    nreg = 1 + order * d
    X, y, th = small_model(kind, order, N, d)
    good = lgoref.folds(N, 3)
    fresh = abi.Context(0)
    try:
        fresh.set_model(kind, order, X, y)
        # without a set-up: the pointer and ngroups < 1 checks come first, then the state
        assert _rc(fresh, 3, None, n_out=N) == abi.ERR_ARG
        assert _rc(fresh, 3, good, mean=False) == abi.ERR_ARG
        assert _rc(fresh, 3, good, var=False) == abi.ERR_ARG
        assert _rc(fresh, 3, good, info=False) == abi.ERR_ARG
        assert _rc(fresh, 0, good) == abi.ERR_ARG
        assert fresh.L.gpemu_lgo(None, 3, None, None, None, None, None, None, None, None) == abi.ERR_ARG
        assert _rc(fresh, 3, good) == abi.ERR_STATE
        with pytest.raises(abi.GpemuError) as ei:
            fresh.lgo(good)
        assert ei.value.code == abi.ERR_STATE
        assert fresh.L.gpemu_lgo_dev(fresh.h, 3, good.ctypes.data_as(abi.C.POINTER(abi.C.c_int)), None, None, None, None, None) == abi.ERR_ARG
    finally:
        fresh.close()
    setup(gpu_ctx, kind, order, X, y, th)
    assert _rc(gpu_ctx, 3, good) == abi.OK
    assert _rc(gpu_ctx, N + 1, good) == abi.ERR_ARG                       # more groups than points
    bad = good.copy(); bad[7] = 3
    assert _rc(gpu_ctx, 3, bad) == abi.ERR_ARG                            # a label >= ngroups
    bad = good.copy(); bad[7] = -2
    assert _rc(gpu_ctx, 3, bad) == abi.ERR_ARG                            # a label < -1
    assert _rc(gpu_ctx, 4, good) == abi.ERR_ARG                           # label 3 has no members
    big = np.full(N, -1, dtype=np.int32); big[:N - nreg] = 0
    assert _rc(gpu_ctx, 1, big) == abi.ERR_ARG                            # N - b_max = nreg: no degrees of freedom left
    big[N - nreg - 1] = -1
    assert _rc(gpu_ctx, 1, big) == abi.OK                                 # N - b_max = nreg + 1
    # a pending host-buffer prediction batch stays collectable across a call
    Xq = X[:11] + 0.02
    want = gpu_ctx.predict(Xq)
    gpu_ctx.predict_enqueue(Xq)
    assert gpu_ctx.lgo(good)["status"] == abi.OK
    got = gpu_ctx.predict_collect()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # the prediction state belongs to the old training vector
    gpu_ctx.set_training(y + 1.0)
    with pytest.raises(abi.GpemuError) as ei:
        gpu_ctx.lgo(good)
    assert ei.value.code == abi.ERR_STATE


def test_group_larger_than_16384_is_refused(gpu_ctx):
    """bp > 16384 needs a set-up model of more than 16384 + nreg points: the design of BASELINE configs[2] at N = 16450"""
    from madaiemulator_amd import synth
    kind, order, N, d = 3, 1, 16450, 8
    X, y = synth.design(N, d, 20261003 + 2)
    setup(gpu_ctx, kind, order, X, y, synth.default_thetas(kind, d))
    group = np.full(N, -1, dtype=np.int32)
    group[:16385] = 0                                                      # bp = 16448
    assert _rc(gpu_ctx, 1, group) == abi.ERR_ARG
    assert "16384" in gpu_ctx.L.gpemu_last_error(gpu_ctx.h).decode()
    gpu_ctx.set_model(1, 1, X[:70, :3], y[:70])                            # (the session's context gives the memory back)


# ------------------------------------------------------------------ 7. profiling class
def test_profile_class(gpu_ctx):
    kind, order, N, d = 1, 1, 150, 3
    X, y, th = small_model(kind, order, N, d)
    group = lgoref.ragged(N, RAGGED, 11)
    setup(gpu_ctx, kind, order, X, y, th)
    gpu_ctx.prof_begin(abi.PROF_LGO)
    gpu_ctx.lgo(group)
    p = gpu_ctx.prof_end()
    Np, bp, nbc = 192, 64, 5
    print("PROF_LGO:", p)
    assert p["n"] == 3 and p["ms"] > 0
    assert p["bytes"] == 8.0 * nbc * bp * (Np + (2 * bp + 64) + (bp / 2 + 4))
