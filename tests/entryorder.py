"""The catalogue behind tests/test_entryorder.py and tests/test_gpu_entry_order.py: every entry of include/gpemu.h placed as
a PROBE (an entry with outputs, run with fixed inputs), a DISTURBER (an entry documented to invalidate kept state, or to
leave it alone) or EXEMPT (deliberately outside, with the reason).  The GPU module runs the probes against each other on
long-lived contexts and compares every output, bit for bit, with the same probe on a new context straight after its set-up.

No device is needed to import this module: contexts are made by Rig, which the GPU module alone creates.

A probe is `fn(ctxs, m) -> dict of numpy arrays and return codes`: ctxs the two contexts of a rig (two components on one
design: the second one is what the two-context entries take), m the Model.  All inputs are fixed and come from the reference
modules of the other tests (designtargetref, jointref, lgoref, calibref, sampleref, resref) and madaiemulator_amd.synth.
A probe that the library refuses returns {"rc": code} and nothing else (run_probe).

The models, the smallest with ragged tiles and more than one tile row:
  A  pow-exp, order 1, N = 130, d = 3 (Np = 192, nreg = 4)
  B  Matern 5/2, order 0, N = 65, d = 2        (the closed-form sensitivity and IMSE entries refuse it: GPEMU_ERR_ARG)
  C  pow-exp, order 1, N = 257, d = 8          (only where a model change is the point)
Query and candidate counts: 1, 5, 70, 200 (200 so that a small call follows one that grew every block buffer).

What model B does not exercise: the closed-form sensitivity entries, gpemu_design_gain and gpemu_design_batch refuse a Matern
model (GPEMU_ERR_ARG), so on B those probes compare one refusal with another, and the state they keep (sens_post_N,
design_serial, design_box, batch_mb) is exercised on models A and C alone; the loglik_grad_batch and test_grad_sums disturbers
fall back to a likelihood batch and to nothing on B (the Matern gradient needs two mode flags).  What B does exercise of the
kept state: the joint factor, the transposed copy (linvT_ready), the corner (cinv_ready), the target store, the calibration
table, the sampler, the batch buffers at every size.
"""
import contextlib
import functools

import numpy as np

import calibref
import designtargetref
import jointref
import lgoref
import resref
import sampleref
from madaiemulator_amd import abi, synth

SPEC = dict(A=(abi.POWEREXP, 1, 130, 3), B=(abi.MATERN52, 0, 65, 2), C=(abi.POWEREXP, 1, 257, 8))
SIZES = (1, 5, 70, 200)
NTARGETS = 70
NPICKS = 3
WALKERS, STEPS = 8, 6
THETA2_SHIFT = 0.1                                    # theta_2 of "a new set-up in the middle": every length scale times e^0.1


class Model:
    """the fixed inputs of every probe for one of the models of SPEC"""

    def __init__(self, name):
        self.name = name
        self.kind, self.order, self.N, self.d = SPEC[name]
        kind, N, d = self.kind, self.N, self.d
        self.nreg = 1 + self.order * d
        self.X, y = designtargetref.data(N, d)
        self.Y = synth.multi_outputs(self.X, y, 3)                       # the training vectors of three components; column 0 is y
        th = designtargetref.thetas(kind, d)
        self.ths = [th.copy() for _ in range(3)]                         # a theta vector of its own per component
        for c in range(3):
            self.ths[c][2:] += 0.02 * c
        self.kappa = designtargetref.kappa(kind, th)
        # the box and a mixed measure over it (uniform, Gaussian, uniform ...: the design's centre and 0.3 of its range)
        self.lo, self.hi = designtargetref.box(self.X)
        self.mkind = (np.arange(d) % 2).astype(np.int32)
        g = self.mkind == abi.MEASURE_GAUSS
        self.glo, self.ghi = np.where(g, (self.lo + self.hi) / 2, self.lo), np.where(g, 0.3 * (self.hi - self.lo), self.hi)
        t = np.linspace(0.0, 1.0, 5)
        self.grid = self.lo[:, None] + t[None, :] * (self.hi - self.lo)[:, None]          # d x 5
        # queries (some on design points, some outside the box), candidates (none within a tenth of a length scale of a design
        # point), targets with weights (target 0 on a design point, one weight 0), joint queries (no two alike, none on a
        # design point) with noise, two rows of observations and three of normals
        self.Xq = {M: designtargetref.points(self.X, M, 100 + M) for M in SIZES}
        self.cand = {M: designtargetref.far_candidates(self.X, th, M, 200 + M) for M in SIZES}
        self.Xt, self.wt, _ = designtargetref.targets_and_candidates(self.X, NTARGETS, 5)
        self.Xj = {M: jointref.fresh_queries(self.X, M, 300 + M) for M in SIZES}
        self.noise = {M: jointref.noise_for(self.kappa, M, 400 + M) for M in SIZES}
        self.yobs = {M: synth.normal(500 + M, 2 * M).reshape(2, M) for M in SIZES}
        self.z = {M: synth.normal(600 + M, 3 * M).reshape(3, M) for M in SIZES}
        self.group = lgoref.folds(N, 3, seed=5)
        # the sampler: a box prior over the unit cube the designs are drawn in, walkers started in its middle
        self.prior = (np.zeros(d), np.ones(d))
        # (each half of the walkers must span the space: at least d + 1 of them)
        self.walkers = max(WALKERS, 2 * (d + 1))
        self.x0 = sampleref.prior_draws(7, self.walkers, np.full(d, 0.3), np.full(d, 0.6), np.zeros(d, dtype=int))
        self.other = SPEC["C" if name != "C" else "A"]                   # what gpemu_set_model switches to and back from


@functools.lru_cache(maxsize=None)
def model(name):
    return Model(name)


@functools.lru_cache(maxsize=None)
def calib_case():
    """ONE observation set for every model (the table does not depend on the model): two components, three outputs, diagonal S
    with a relative model error; its `mean` and `var` rows are the inputs of the calib_eval probes"""
    return calibref.make_case("entryorder", 2, 3, max(SIZES), False, True)


# ---------------------------------------------------------------------------------------------------- running a probe
class _RecordingNumpy:
    """numpy as abi.py sees it while a probe runs: np.empty comes back filled with a sentinel, and every array the binding
    allocates for an entry's outputs is kept with a copy, so that after a refused call the test can see that nothing was
    written (the wrappers raise and drop their arrays otherwise).  This relies on abi.py making its output arrays with
    np.empty, np.empty_like, np.zeros or np.full, before the call; a refused probe for which nothing was recorded fails the
    check (untouched)"""
    SENTINEL = -7.25e77

    def __init__(self):
        self.made = []

    def __getattr__(self, k):
        return getattr(np, k)

    def _keep(self, a):
        self.made.append((a, a.copy()))
        return a

    def empty(self, shape, dtype=np.float64):
        return self._keep(np.full(shape, self.SENTINEL if np.dtype(dtype).kind == "f" else -77, dtype=dtype))

    def empty_like(self, a):
        return self.empty(a.shape, a.dtype)

    def full(self, *a, **k):
        return self._keep(np.full(*a, **k))

    def zeros(self, *a, **k):
        return self._keep(np.zeros(*a, **k))

    def untouched(self):
        """(nothing recorded counts as touched: an output the binding makes some other way must not pass unseen)"""
        return bool(self.made) and all(a.tobytes() == c.tobytes() for a, c in self.made)


LAST_ERROR = [None]        # the library's text for the last refused probe (None after a probe that ran)


def run_probe(fn, ctxs, m):
    """-> (outputs, untouched): a refused probe gives {"rc": code}; untouched says whether every array the binding made for the
    call that was refused still holds its prefill.  The refusal's text is kept in LAST_ERROR for the failure messages"""
    rec = _RecordingNumpy()
    abi.np = rec
    LAST_ERROR[0] = None
    try:
        out = fn(ctxs, m)
        out.setdefault("rc", abi.OK)
        return out, None
    except abi.GpemuError as e:
        LAST_ERROR[0] = str(e)
        return dict(rc=e.code), rec.untouched()
    finally:
        abi.np = np


def same(a, b):
    """bit equality of two probe outputs: the same keys, and per key the same type, shape and bytes"""
    if a.keys() != b.keys():
        return False
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            return False
    return True


def first_difference(a, b):
    """a: what the probe gave, b: what was expected"""
    if a.keys() != b.keys():
        why = f' ("{LAST_ERROR[0]}")' if LAST_ERROR[0] else ""
        return f"rc {int(a['rc'])}{why} with keys {sorted(a)} against rc {int(b['rc'])} with keys {sorted(b)}"
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.dtype != y.dtype or x.shape != y.shape:
            return f"{k}: {x.dtype}{x.shape} against {y.dtype}{y.shape}"
        if x.tobytes() != y.tobytes():
            xb, yb = (np.frombuffer(np.ascontiguousarray(v).tobytes(), np.uint8).reshape(max(v.size, 1), -1) for v in (x, y))
            bad = np.flatnonzero(np.any(xb != yb, axis=1))
            i = int(bad[0])
            return f"{k}: {bad.size} of {x.size} elements differ, the first at {i}: {x.ravel()[i]!r} against {y.ravel()[i]!r}"
    return None


# ---------------------------------------------------------------------------------------------------- the probes
class Probe:
    def __init__(self, name, fn, symbols, needs=("setup",), family=None, M=None, after=None, refuses_pending=False, keeps=()):
        self.name, self.fn, self.symbols, self.needs = name, fn, tuple(symbols), frozenset(needs)
        self.family, self.M, self.after, self.refuses_pending, self.keeps = family, M, after, refuses_pending, tuple(keeps)


ALL = {}                 # every probe by name, the sized variants included
PROBES = []              # the names every case runs: one size per family (predict: three)


def _probe(name, symbols, main=True, **kw):
    def deco(fn):
        ALL[name] = Probe(name, fn, symbols, **kw)
        if main:
            PROBES.append(name)
        return fn
    return deco


def _sized(family, symbols, main=(70,), **kw):
    """one probe per size M of SIZES, named family_M; `main` says which of them every case runs"""
    def deco(fn):
        for M in SIZES:
            ALL[f"{family}_{M}"] = Probe(f"{family}_{M}", functools.partial(fn, M=M), symbols if M == main[0] else (), family=family, M=M, **kw)
            if M in main:
                PROBES.append(f"{family}_{M}")
        return fn
    return deco


def _d(**kw):
    return {k: np.asarray(v) for k, v in kw.items() if v is not None}


# -- prediction: the host-buffer entries stage through dXq / dMean / hStage and are enqueue + collect over the _dev entries
@_sized("predict", ["gpemu_predict_batch", "gpemu_predict_batch_enqueue", "gpemu_predict_batch_collect", "gpemu_predict_batch_dev"],
        main=(1, 5, 70), refuses_pending=True)
def p_predict(ctxs, m, M):
    mean, var = ctxs[0].predict(m.Xq[M])
    return _d(mean=mean, var=var)


@_sized("predict_mean", ["gpemu_predict_mean", "gpemu_predict_mean_enqueue", "gpemu_predict_mean_collect", "gpemu_predict_mean_dev"],
        refuses_pending=True)
def p_predict_mean(ctxs, m, M):
    return _d(mean=ctxs[0].predict_mean(m.Xq[M]))


@_sized("predict_mean_grad", ["gpemu_predict_mean_grad", "gpemu_predict_mean_grad_enqueue", "gpemu_predict_mean_grad_collect",
                              "gpemu_predict_mean_grad_dev"], refuses_pending=True)
def p_predict_mean_grad(ctxs, m, M):
    mean, grad = ctxs[0].predict_mean_grad(m.Xq[M])
    return _d(mean=mean, grad=grad)


@_sized("predict_var_grad", ["gpemu_predict_var_grad", "gpemu_predict_var_grad_enqueue", "gpemu_predict_var_grad_collect",
                             "gpemu_predict_var_grad_dev"], refuses_pending=True, keeps=("linvT_ready",))
def p_predict_var_grad(ctxs, m, M):
    mean, var, grad = ctxs[0].predict_var_grad(m.Xq[M])
    return _d(mean=mean, var=var, grad=grad)


@_sized("predict_cov", ["gpemu_predict_cov", "gpemu_predict_cov_dev"], refuses_pending=True)
def p_predict_cov(ctxs, m, M):
    mean, cov = ctxs[0].predict_cov(m.Xq[M])
    return _d(mean=mean, cov=cov)


@_sized("joint", ["gpemu_predict_joint_factor", "gpemu_predict_joint_factor_dev", "gpemu_predict_joint_draw", "gpemu_predict_joint_draw_dev"],
        refuses_pending=True, keeps=("joint_M",))
def p_joint(ctxs, m, M):
    """factor, then draw from the factor it left"""
    r = ctxs[0].predict_joint_factor(m.Xj[M], noise=m.noise[M], yobs=m.yobs[M])
    assert r["status"] == abi.OK, r["info"]
    return _d(draw=ctxs[0].predict_joint_draw(m.z[M]), **r)


@_probe("joint_draw_only", [], after="joint_70", refuses_pending=True)
def p_joint_draw_only(ctxs, m):
    """needs the factor joint_70 left: GPEMU_ERR_STATE without one.  The rows are those of the largest size, so that the call
    stays inside its buffers whatever factor is resident; of each the first 70 values are read"""
    return _d(draw=ctxs[0].predict_joint_draw(m.z[max(SIZES)][::-1]))


# -- validation from the resident factor
@_probe("loo", ["gpemu_loo", "gpemu_loo_dev"])
def p_loo(ctxs, m):
    mean, var = ctxs[0].loo()
    return _d(mean=mean, var=var)


@_probe("lgo", ["gpemu_lgo"])
def p_lgo(ctxs, m):
    return _d(**ctxs[0].lgo(m.group, 3))


@_probe("lgo_ragged", [])
def p_lgo_ragged(ctxs, m):
    """groups of 1, N / 2 and 7 points, the others never left out: for model A another padded size (128) than the folds' (64)"""
    return _d(**ctxs[0].lgo(lgoref.ragged(m.N, (1, m.N // 2, 7), 9), 3))


# -- three device-pointer entries that no host entry runs through (the others are the bodies of their host entries)
@contextlib.contextmanager
def _device(c, *specs):
    """device arrays of the caller's: (count, dtype, initial values or None for an output).  Outputs are prefilled with the
    recorder's sentinel; where the entry refuses they are downloaded through the binding, so that the recorder sees whether
    the refusal wrote into them"""
    ptrs = []
    try:
        for n, dt, init in specs:
            ptrs.append(c.dev_alloc(max(n, 1) * np.dtype(dt).itemsize))
            fill = _RecordingNumpy.SENTINEL if np.dtype(dt).kind == "f" else -77
            c.upload(ptrs[-1], np.full(max(n, 1), fill, dtype=dt) if init is None else np.ascontiguousarray(init, dtype=dt))
        yield ptrs
    except abi.GpemuError:
        for p, (n, dt, init) in zip(ptrs, specs):
            if init is None:
                c.download(p, (max(n, 1),), dt)
        raise
    finally:
        for p in ptrs:
            c.dev_free(p)


@_probe("lgo_dev", ["gpemu_lgo_dev"])
def p_lgo_dev(ctxs, m):
    c, N = ctxs[0], m.N
    with _device(c, (N, np.float64, None), (N, np.float64, None), (N, np.float64, None), (9, np.float64, None), (3, np.int32, None)) as (dm, dv, dw, ds, di):
        c.lgo_dev(m.group, 3, dm, dv, dw, ds, di)
        return _d(mean=c.download(dm, (N,)), var=c.download(dv, (N,)), werr=c.download(dw, (N,)), stat=c.download(ds, (3, 3)),
                  info=c.download(di, (3,), np.int32))


@_probe("target_set_dev", ["gpemu_design_target_set_dev"], keeps=("tgt_S", "tgt_serial"))
def p_target_set_dev(ctxs, m):
    """the targets of target_gain_* from device memory, then a gain over them"""
    c = ctxs[0]
    with _device(c, (m.Xt.size, np.float64, m.Xt), (1, np.float64, None), (NTARGETS, np.float64, None)) as (dx, dt, dv):
        c.design_target_set_dev(NTARGETS, dx, m.wt, dt, dv)
        out = _d(target_var=c.download(dt, (1,)), var_t=c.download(dv, (NTARGETS,)))
    out.update(_d(**c.design_target_gain(m.cand[5])))
    return out


@_probe("calib_gather_dev", ["gpemu_calib_gather_dev"], needs=())
def p_calib_gather_dev(ctxs, m):
    """four listed points of a 5 x 70 table of the caller's, with their worst outputs"""
    c, M, idx = ctxs[0], 70, np.array([3, 0, 69, 17], dtype=np.int32)
    with _device(c, (5 * M, np.float64, synth.uniform(31, (5, M))), (M, np.int32, np.arange(M) % 3), (4, np.int32, idx),
                 (20, np.float64, None), (4, np.int32, None)) as (ds, dw, di, do, dwo):
        c.calib_gather_dev(M, ds, dw, 4, di, do, dwo)
        return _d(out=c.download(do, (4, 5)), worst=c.download(dwo, (4,), np.int32))


# -- the closed-form sensitivity entries, under the uniform measure and under a mixed one (set for the call, then reset)
def _box_of(m, mixed):
    return (m.glo, m.ghi) if mixed else (m.lo, m.hi)


def _under_measure(fn, mixed):
    def run(ctxs, m):
        if not mixed:
            return fn(ctxs, m, m.lo, m.hi)
        for c in ctxs:
            c.sens_set_measure(m.mkind)
        try:
            out = fn(ctxs, m, m.glo, m.ghi)
            out["measure"] = np.concatenate([c.sens_get_measure() for c in ctxs])
            return out
        finally:
            for c in ctxs:
                c.sens_set_measure(None)
    return run


def _sens(name, symbols, **kw):
    """the probe under the uniform measure, and name_mixed under the mixed one"""
    def deco(fn):
        ALL[name] = Probe(name, _under_measure(fn, False), symbols, **kw)
        ALL[name + "_mixed"] = Probe(name + "_mixed", _under_measure(fn, True), [], **kw)
        PROBES.extend([name, name + "_mixed"])
        return fn
    return deco


@_sens("sens_cov", ["gpemu_sens_cov", "gpemu_sens_cov_dev", "gpemu_sens_set_measure", "gpemu_sens_get_measure"])
def p_sens_cov(ctxs, m, lo, hi):
    return _d(**ctxs[0].sens_cov(lo, hi))


@_sens("sens_cov_two", [])
def p_sens_cov_two(ctxs, m, lo, hi):
    return _d(**ctxs[0].sens_cov(lo, hi, other=ctxs[1]))


@_sens("sens_main", ["gpemu_sens_main"])
def p_sens_main(ctxs, m, lo, hi):
    e0, main = ctxs[0].sens_main(lo, hi, m.grid)
    return _d(e0=e0, main=main)


@_sens("sens_post", ["gpemu_sens_post", "gpemu_sens_post_dev", "gpemu_test_sens_post_state"], keeps=("cinv_ready", "sens_post_N"))
def p_sens_post(ctxs, m, lo, hi):
    out = ctxs[0].sens_post(lo, hi)
    P, G, Q = ctxs[0].sens_post_state()
    return _d(P=P, G=G, Q=Q, **out)


@_sens("sens_main_var", ["gpemu_sens_main_var"])
def p_sens_main_var(ctxs, m, lo, hi):
    main, var, ve0 = ctxs[0].sens_main_var(lo, hi, m.grid)
    return _d(main=main, var=var, var_e0=ve0)


@_sens("sens_pairs", ["gpemu_sens_pairs", "gpemu_sens_pairs_dev"])
def p_sens_pairs(ctxs, m, lo, hi):
    return _d(own=ctxs[0].sens_pairs(lo, hi), two=ctxs[0].sens_pairs(lo, hi, other=ctxs[1]))


@_sens("sens_pairs_post", ["gpemu_sens_pairs_post", "gpemu_sens_pairs_post_dev"], keeps=("cinv_ready",))
def p_sens_pairs_post(ctxs, m, lo, hi):
    return _d(s_pair=ctxs[0].sens_pairs_post(lo, hi))


@_sens("sens_joint", ["gpemu_sens_joint"])
def p_sens_joint(ctxs, m, lo, hi):
    e0, joint, inter = ctxs[0].sens_joint(lo, hi, 0, 1, m.grid[0], m.grid[1])
    return _d(e0=e0, joint=joint, inter=inter)


# -- where to put the next run
@_sized("design_gain", ["gpemu_design_gain", "gpemu_design_gain_dev", "gpemu_test_design_state"], keeps=("design_serial", "design_mb"))
def p_design_gain(ctxs, m, M):
    out = ctxs[0].design_gain(m.lo, m.hi, m.cand[M])
    a, b = ctxs[0].design_state(M)
    return _d(a=a, b=b, **out)


@_probe("design_gain_mixed", [], keeps=("design_serial", "design_box"))
def p_design_gain_mixed(ctxs, m):
    """the same candidates under the mixed measure: the kept block [K ; HK] belongs to one box and one set of kinds"""
    return _under_measure(lambda c, mm, lo, hi: _d(**c[0].design_gain(lo, hi, mm.cand[70])), True)(ctxs, m)


@_sized("design_batch", ["gpemu_design_batch", "gpemu_design_batch_dev", "gpemu_test_design_batch_state"], keeps=("batch_mb",))
def p_design_batch(ctxs, m, M):
    nb = min(NPICKS, M)
    out = abi.design_batch(ctxs, m.lo, m.hi, m.cand[M], nb, weight=[1.0, 0.5])
    lam, mu, E = ctxs[1].design_batch_state(M, nb)
    return _d(lam=lam, mu=mu, E=E, **out)


@_sized("target_gain", ["gpemu_design_target_set", "gpemu_design_target_gain", "gpemu_design_target_gain_dev", "gpemu_test_design_target_state"],
        keeps=("tgt_S", "tgt_serial", "tgt_mb"))
def p_target_gain(ctxs, m, M):
    """sets the targets, then the gain of M candidates over them"""
    s = ctxs[0].design_target_set(m.Xt, m.wt)
    ut, rt, qrt = ctxs[0].design_target_state(0, NTARGETS)
    out = ctxs[0].design_target_gain(m.cand[M])
    uq, rq, qrq = ctxs[0].design_target_state(1, M)
    return _d(target_var=s["target_var"], var_t=s["var_t"], ut=ut, rt=rt, qrt=qrt, uq=uq, rq=rq, qrq=qrq, **out)


@_probe("target_gain_only", [], after="target_gain_70")
def p_target_gain_only(ctxs, m):
    """against the targets target_gain_* left resident: GPEMU_ERR_STATE without them"""
    return _d(**ctxs[0].design_target_gain(m.Xq[5]))


# -- calibration: the table is ctxs[0]'s (Rig.install), the components are both contexts
@_sized("calib_eval", ["gpemu_calib_eval", "gpemu_calib_eval_dev"], needs=("calib",))
def p_calib_eval(ctxs, m, M):
    c = calib_case()
    stat, worst = ctxs[0].calib_eval(np.ascontiguousarray(c["mean"][:, :M]), np.ascontiguousarray(c["var"][:, :M]))
    return _d(stat=stat, worst=worst)


@_sized("calib_grad", ["gpemu_calib_grad", "gpemu_calib_grad_dev"], needs=("setup", "calib"), refuses_pending=True)
def p_calib_grad(ctxs, m, M):
    """the gradients of chi2 and of the log density at M queries, from both components' predict_var_grad / predict_mean_grad"""
    pv = [c.predict_var_grad(m.Xq[M]) for c in ctxs]
    gm = [c.predict_mean_grad(m.Xq[M], want_mean=False)[1] for c in ctxs]
    gc, gl = ctxs[0].calib_grad(np.array([p[0] for p in pv]), np.array([p[1] for p in pv]), np.array(gm), np.array([p[2] for p in pv]))
    return _d(gchi2=gc, glogpdf=gl)


@_sized("calib_select", ["gpemu_calib_select", "gpemu_calib_select_dev"], needs=("setup", "calib"), refuses_pending=True)
def p_calib_select(ctxs, m, M):
    """on the outputs of a prediction: both components at M queries, the statistics, the points whose largest I_t stays under 3"""
    pr = [c.predict(m.Xq[M]) for c in ctxs]
    stat, worst = ctxs[0].calib_eval(np.array([p[0] for p in pr]), np.array([p[1] for p in pr]))
    return _d(stat=stat, worst=worst, idx=ctxs[0].calib_select(stat, level=1, cut_I=3.0))


@_probe("calib_sample", ["gpemu_calib_sample", "gpemu_sample_propose_dev", "gpemu_sample_accept_dev", "gpemu_sample_logpost_dev"],
        needs=("setup", "calib", "prior"))
def p_calib_sample(ctxs, m):
    r = abi.calib_sample(ctxs, ctxs[0], m.x0, STEPS, seed=11)
    return _d(**r)


# -- the matrices themselves and the state behind the predictions
@_probe("cinverse", ["gpemu_get_cinverse"], keeps=("cinv_ready",))
def p_cinverse(ctxs, m):
    return _d(cinv=ctxs[0].cinverse())


@_probe("pred_state", ["gpemu_test_pred_state"])
def p_pred_state(ctxs, m):
    beta, gamma = ctxs[0].pred_state()
    return _d(beta=beta, gamma=gamma)


@_probe("cov_matrix", ["gpemu_cov_matrix"], needs=())
def p_cov_matrix(ctxs, m):
    return _d(C=ctxs[0].cov_matrix(m.ths[1]))


@_probe("kvectors", ["gpemu_kvectors"], needs=())
def p_kvectors(ctxs, m):
    return _d(K=ctxs[0].kvectors(m.ths[1], m.Xq[5]))


SIZED_FAMILIES = sorted({p.family for p in ALL.values() if p.family})
REFUSES_PENDING = sorted(n for n, p in ALL.items() if p.refuses_pending)
# model B: a reduced list for the pairs, with every probe that keeps state (Probe.keeps) or follows one (Probe.after), the
# validation entries, and one probe of every buffer family
REDUCED_B = [n for n in PROBES if ALL[n].keeps or ALL[n].after or n in ("predict_1", "predict_70", "predict_mean_70", "predict_cov_70", "loo", "lgo",
                                                                         "lgo_dev", "calib_eval_70", "calib_select_70", "calib_gather_dev", "calib_sample", "pred_state",
                                                                         "kvectors")]

# the buffer families of the sizes case: a probe of the same family to run between two sizes
BETWEEN = dict(predict="predict_var_grad_70", predict_mean="predict_mean_grad_70", predict_mean_grad="predict_mean_70", predict_var_grad="design_gain_70",
               predict_cov="joint_70", joint="predict_cov_70", design_gain="target_gain_70", design_batch="design_gain_70",
               target_gain="design_batch_70", calib_eval="calib_select_70", calib_grad="calib_eval_70", calib_select="calib_grad_70")


# ---------------------------------------------------------------------------------------------------- a rig: contexts with a known history
class Rig:
    """Two contexts on the design of model m -- ctxs[i] trains on column ys[i] of m.Y at thetas m.ths[ys[i]] -- and what the
    header says they hold: `ready` (a prediction set-up on both), `joint` (the resident joint factor's probe, or None),
    `targets`, `calib`, `prior`.  run() runs a probe and follows the state; expected() says what the probe must return."""

    def __init__(self, m, ys=(0, 1), ctxs=None):
        self.m, self.ys = m, tuple(ys)
        self.own = ctxs is None
        self.ctxs = [abi.Context(0), abi.Context(0)] if ctxs is None else list(ctxs)
        self.ready, self.joint, self.targets, self.calib, self.prior, self.shift = False, None, False, False, False, 0.0
        self.broken = False                # set by the GPU module where a check failed: the history is then not what the flags say

    def close(self):
        if self.own:
            for c in self.ctxs:
                c.close()

    def key(self):
        return (self.m.name, self.ys, self.shift)

    def set_model(self, m=None):
        self.m = self.m if m is None else m
        for c, col in zip(self.ctxs, self.ys):
            c.set_model(self.m.kind, self.m.order, self.m.X, self.m.Y[:, col])
        self.ready, self.joint, self.targets = False, None, False

    def set_tables(self):
        c = calib_case()
        rc, info = self.ctxs[0].calib_setup(c["ybar"], c["A"], c["z"], sd=c["sd"], rel=c["rel"])
        assert rc == abi.OK and info == 0
        self.ctxs[0].sample_set_prior(*self.m.prior)
        self.calib = self.prior = True

    def install(self):
        self.set_model()
        self.set_tables()
        return self

    def thetas(self, i):
        th = self.m.ths[self.ys[i]].copy()
        th[2:] += self.shift
        return th

    def setup(self, shift=0.0):
        self.shift = shift
        for i, c in enumerate(self.ctxs):
            beta, rc = c.predict_setup(self.thetas(i))
            assert rc == abi.OK
        self.ready, self.joint = True, None
        return self

    def after_batch_setup(self):
        """the contexts were set up from outside, by abi.predict_setup_batch"""
        self.ready, self.joint, self.shift = True, None, 0.0

    def have(self):
        return {k for k, v in (("setup", self.ready), ("calib", self.calib), ("prior", self.prior)) if v}

    def expected(self, name, fresh):
        """fresh: (rig key, probe name) -> the probe's output on a new rig"""
        p = ALL[name]
        if not p.needs <= self.have():
            return dict(rc=abi.ERR_STATE)
        if name == "joint_draw_only" and self.joint != "joint_70":
            return dict(rc=abi.ERR_STATE)
        if name == "target_gain_only" and not self.targets:
            return dict(rc=abi.ERR_STATE)
        return fresh(self.key(), name)

    def run(self, name):
        assert name != "joint_draw_only" or self.joint in (None, "joint_70"), "the draw-only probe has a reference for joint_70's factor alone"
        out, untouched = run_probe(ALL[name].fn, self.ctxs, self.m)
        if out["rc"] == abi.OK:
            if ALL[name].family == "joint":
                self.joint = name
            if ALL[name].family == "target_gain" or name == "target_set_dev":       # (the same targets either way)
                self.targets = True
        return out, untouched

    def restore(self):
        """whatever a disturber dropped, back: the model, the tables, the set-up"""
        if not (self.calib and self.prior):
            self.set_tables()
        if not self.ready:
            self.setup(self.shift)


def fresh_output(key, name):
    """probe `name` on a new rig of that key straight after the set-up (for a probe with `after`: straight after that probe)"""
    mname, ys, shift = key
    rig = Rig(model(mname), ys).install().setup(shift)
    try:
        if ALL[name].after:
            pre, _ = rig.run(ALL[name].after)
            assert pre["rc"] in (abi.OK, abi.ERR_ARG)
        out, _ = rig.run(name)
        return out
    finally:
        rig.close()


# ---------------------------------------------------------------------------------------------------- the disturbers
class Disturber:
    """fn(rig) runs the entry on every context of the rig.  invalidates: the header says the prediction set-up is gone (every
    probe that needs one must refuse until a new one).  drops: what else is gone, of "joint", "targets", "calib", "prior"."""

    def __init__(self, name, fn, symbols, invalidates=False, drops=()):
        self.name, self.fn, self.symbols, self.invalidates, self.drops = name, fn, tuple(symbols), invalidates, tuple(drops)

    def apply(self, rig):
        self.fn(rig)
        if self.invalidates:
            rig.ready, rig.joint = False, None
        for k in self.drops:
            setattr(rig, k, None if k == "joint" else False)


DISTURBERS = {}


def _disturber(name, symbols, **kw):
    def deco(fn):
        DISTURBERS[name] = Disturber(name, fn, symbols, **kw)
        return fn
    return deco


def _each(fn):
    return lambda rig: [fn(rig, i, c) for i, c in enumerate(rig.ctxs)]


@_disturber("loglik", ["gpemu_loglik", "gpemu_loglik_enqueue", "gpemu_loglik_collect"], invalidates=True)
@_each
def d_loglik(rig, i, c):
    assert c.loglik(rig.thetas(i))["status"] == abi.OK


@_disturber("loglik_batch", ["gpemu_loglik_batch", "gpemu_loglik_batch_enqueue", "gpemu_loglik_batch_collect", "gpemu_loglik_batch_collect_back"],
            invalidates=True)
@_each
def d_loglik_batch(rig, i, c):
    r = c.loglik_batch(np.array([rig.thetas(0), rig.thetas(1), rig.thetas(i)]))
    assert np.all(r["status"] == abi.OK)
    back = c.loglik_batch_collect_back(0, 3)
    assert back["value"].tobytes() == r["value"].tobytes()


@_disturber("loglik_grad_batch", ["gpemu_loglik_grad_batch", "gpemu_loglik_grad_batch_enqueue", "gpemu_loglik_grad_batch_collect",
                                  "gpemu_loglik_grad_batch_collect_back", "gpemu_loglik_grad", "gpemu_grad"], invalidates=True)
@_each
def d_loglik_grad_batch(rig, i, c):
    if rig.m.kind != abi.POWEREXP:                           # (the Matern gradient needs two mode flags: the literal form is pow-exp's)
        c.loglik_batch(np.array([rig.thetas(i)]))
        return
    r = c.loglik_grad_batch(np.array([rig.thetas(i), rig.thetas(1 - i)]))
    assert np.all(r["status"] == abi.OK)
    one = c.loglik_grad(rig.thetas(i))
    g, rc = c.grad(rig.thetas(i))
    assert rc == abi.OK and one["grad"].tobytes() == g.tobytes()


@_disturber("set_training", ["gpemu_set_training"], invalidates=True)
@_each
def d_set_training(rig, i, c):
    c.set_training(rig.m.Y[:, rig.ys[i]])


@_disturber("set_mode", ["gpemu_set_mode"], invalidates=True)
@_each
def d_set_mode(rig, i, c):
    mode = c.get_mode()
    c.set_mode(mode ^ abi.MODE_EXACT_GRAD)
    c.set_mode(mode)


@_disturber("set_mode_same", [])
@_each
def d_set_mode_same(rig, i, c):
    c.set_mode(c.get_mode())


@_disturber("set_model", ["gpemu_set_model"], invalidates=True, drops=("joint", "targets"))
def d_set_model(rig):
    """to another model and back: the calibration table and the prior stay (the prior is the same d again), the targets go"""
    kind, order, N, d = rig.m.other
    X, y = designtargetref.data(N, d)
    for c in rig.ctxs:
        c.set_model(kind, order, X, y)
    rig.set_model()


@_disturber("predict_setup", ["gpemu_predict_setup"], drops=("joint",))
def d_predict_setup(rig):
    rig.setup(rig.shift)


@_disturber("predict_setup_batch", ["gpemu_predict_setup_batch"], drops=("joint",))
def d_predict_setup_batch(rig):
    beta, info, status, rc = abi.predict_setup_batch(rig.ctxs, np.array([rig.thetas(0), rig.thetas(1)]))
    assert rc == abi.OK and not np.any(status)
    rig.ready = True


# the matrix-only entries: buffers of their own
def _spd(n, seed):
    A = synth.uniform(seed, (n, n)) - 0.5
    return A @ A.T + n * np.eye(n)


@_disturber("chol_inverse", ["gpemu_chol_inverse"])
@_each
def d_chol_inverse(rig, i, c):
    assert c.chol_inverse(_spd(130, 3))[3] == abi.OK


@_disturber("symm_apply", ["gpemu_symm_apply", "gpemu_symm_invalidate", "gpemu_symm_pin"])
@_each
def d_symm_apply(rig, i, c):
    A = _spd(70, 4)
    c.symm_apply(A, synth.uniform(5, (3, 70)))
    c.symm_pin(True)
    c.symm_apply(A, synth.uniform(6, (3, 70)))
    c.symm_pin(False)
    c.symm_invalidate()


@_disturber("derivative_gauss", ["gpemu_derivative_gauss"])
@_each
def d_derivative_gauss(rig, i, c):
    c.derivative_gauss(synth.uniform(8, (130,)), 0.5)


@_disturber("trace_product", ["gpemu_trace_product"])
@_each
def d_trace_product(rig, i, c):
    c.trace_product(_spd(70, 9), _spd(70, 10))


@_disturber("warm_start", ["gpemu_warm_start"])
def d_warm_start(rig):
    assert abi.load().gpemu_warm_start(0) == abi.OK


# the releases
@_disturber("predict_joint_release", ["gpemu_predict_joint_release"], drops=("joint",))
@_each
def d_joint_release(rig, i, c):
    c.predict_joint_release()


@_disturber("lgo_release", ["gpemu_lgo_release"])
@_each
def d_lgo_release(rig, i, c):
    c.lgo_release()


@_disturber("sens_release", ["gpemu_sens_release"])
@_each
def d_sens_release(rig, i, c):
    c.sens_release()


@_disturber("design_target_release", ["gpemu_design_target_release"], drops=("targets",))
@_each
def d_target_release(rig, i, c):
    c.design_target_release()


@_disturber("calib_release", ["gpemu_calib_release"], drops=("calib",))
@_each
def d_calib_release(rig, i, c):
    c.calib_release()


@_disturber("sample_release", ["gpemu_sample_release"], drops=("prior",))
@_each
def d_sample_release(rig, i, c):
    c.sample_release()


@_disturber("tables_again", ["gpemu_calib_setup", "gpemu_sample_set_prior"])
def d_tables_again(rig):
    """a second set-up of the same table and the same prior replaces them with the same bits"""
    rig.set_tables()


@_disturber("sample_chunk", ["gpemu_test_sample_chunk"])
def d_sample_chunk(rig):
    """the records a run keeps on the device between two copies: no output depends on it"""
    rig.ctxs[0].test_sample_chunk(3)


# the test hooks: device buffers of their own (the header: "the context's factorisation, prediction state and result ring are
# not touched"), and gpemu_test_staged_matrix, which stages into the context's workspace
@_disturber("test_gemm_nt", ["gpemu_test_gemm_nt"])
@_each
def d_test_gemm_nt(rig, i, c):
    c.test_gemm_nt(synth.uniform(20, (70, 48)), synth.uniform(21, (65, 48)), np.zeros((70, 65)))


@_disturber("test_gemm_launch", ["gpemu_test_gemm_launch"])
@_each
def d_test_gemm_launch(rig, i, c):
    c.test_gemm_launch(synth.uniform(22, (3 * 4096,)), offC=0, offA=4096, offB=8192, ldc=64, lda=64, ldb=64, alpha=1.0, m=64, n=64, k0=0, k1=64)


@_disturber("test_update_launch", ["gpemu_test_update_launch"])
@_each
def d_test_update_launch(rig, i, c):
    c.test_update_launch(0.01 * synth.uniform(23, (192 * 128,)), off=0, ld=128, stride=0, c0=0, k=64, ncols=64, rp=64, inv=0, rhs_live=0, nbatch=1)


@_disturber("test_leaf_launch", ["gpemu_test_leaf_launch"])
@_each
def d_test_leaf_launch(rig, i, c):
    out, info = c.test_leaf_launch(_spd(64, 24), off=0, ld=64, bstride=0, nbatch=1, c0=0, m_below=0, op=abi.LEAF_FACTOR)
    assert info[0] == 0


@_disturber("test_grad_sums", ["gpemu_test_grad_sums"])
@_each
def d_test_grad_sums(rig, i, c):
    m = rig.m
    if m.kind != abi.POWEREXP:                               # (refused for a Matern model without the two mode flags, before anything runs)
        return
    c.test_grad_sums(rig.thetas(i), _spd(m.N, 25), synth.uniform(26, (m.N, 1 + m.nreg)))


@_disturber("test_fill_launch", ["gpemu_test_fill_launch"])
@_each
def d_test_fill_launch(rig, i, c):
    Np = resref.round_up(rig.m.N, 64)
    c.test_fill_launch(abi.FILL_FULL, rig.thetas(i), np.zeros((Np, Np)), form=0)


@_disturber("test_resident_launch", ["gpemu_test_resident_launch"])
@_each
def d_test_resident_launch(rig, i, c):
    lin, Np, ld = resref.linv_case(2, 130)
    c.test_resident_launch(abi.RES_LOO_COLSQ, lin=lin, part=resref.nans(resref.nchunks_of(130), Np), ld=ld, N=130, Np=Np)


@_disturber("test_potrf", ["gpemu_test_potrf"])
@_each
def d_test_potrf(rig, i, c):
    assert c.test_potrf(_spd(130, 27))[1] == 0


@_disturber("test_staged_matrix", ["gpemu_test_staged_matrix"], invalidates=True)
@_each
def d_test_staged_matrix(rig, i, c):
    c.staged_matrix(np.array([rig.thetas(i), rig.thetas(1 - i)]), b=1)


# ---------------------------------------------------------------------------------------------------- deliberately outside
EXEMPT = {
    "gpemu_ctx_create": "the life cycle itself: every rig starts with it",
    "gpemu_ctx_destroy": "the life cycle itself: every rig ends with it",
    "gpemu_last_error": "reads the error text, which no entry reads back",
    "gpemu_version": "a constant string",
    "gpemu_device_count": "asks the runtime, no context",
    "gpemu_device_memory": "asks the runtime, no context",
    "gpemu_ctx_device": "a getter of a field fixed at creation",
    "gpemu_get_mode": "a getter (the set_mode disturbers call it)",
    "gpemu_rccl_allgather": "rccl: more than one device",
    "gpemu_rccl_unique_id": "rccl: more than one device",
    "gpemu_rccl_comm_create": "rccl: more than one device",
    "gpemu_rccl_comm_allgather": "rccl: more than one device",
    "gpemu_rccl_comm_destroy": "rccl: more than one device",
    "gpemu_dev_alloc": "the caller's memory, not the context's",
    "gpemu_dev_free": "the caller's memory, not the context's",
    "gpemu_dev_upload": "the caller's memory, not the context's",
    "gpemu_dev_download": "the caller's memory, not the context's",
    "gpemu_sync": "waits for the stream: every host-buffer probe does",
    "gpemu_prof_begin": "profiling: changes how launches are timed, tests/test_gpu_parity.py covers it",
    "gpemu_prof_end": "profiling: the other half of gpemu_prof_begin",
    "gpemu_trace_dump": "tracing is off unless the environment asks for it at creation",
    "gpemu_test_gemm_bench": "a micro-benchmark: timing, no result to compare",
    "gpemu_test_tile_table": "host-only table function",
    "gpemu_test_row_table": "host-only table function",
    "gpemu_calib_project": "host arithmetic, no device and no context",
    "gpemu_philox4x32": "host arithmetic, no device and no context",
    "gpemu_sample_uniforms": "host arithmetic, no device and no context",
}


def named():
    """symbol -> the catalogue entries that name it"""
    out = {}
    for kind, table in (("probe", ALL), ("disturber", DISTURBERS)):
        for n, e in table.items():
            for s in e.symbols:
                out.setdefault(s, []).append(f"{kind} {n}")
    for s in EXEMPT:
        out.setdefault(s, []).append("EXEMPT")
    return out
