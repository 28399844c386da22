"""The pending-batch state machine of the host-buffer prediction entries (include/gpemu.h): the four kinds -- mean+variance
(gpemu_predict_batch), mean-only (gpemu_predict_mean), mean+gradient (gpemu_predict_mean_grad) and variance-gradient
(gpemu_predict_var_grad) -- each with its _enqueue / _collect halves, its synchronous call and its _dev form.

One batch of any kind is pending per context; only its own kind's collect, with its own size and its required outputs,
takes it; every refusal leaves it pending; gpemu_set_model drops it.  Host state only: what the kernels compute is checked
by the kinds' own test files, so every comparison here is bit for bit (np.array_equal) between two ways of asking the same
library for the same queries, on one small model."""
import numpy as np
import pytest

from madaiemulator_amd import abi
from test_gpu_mean_grad import model
from test_gpu_predict_mean import setup, special_queries

pytestmark = pytest.mark.gpu

KIND, ORDER, N, D = 1, 1, 150, 3
M0 = 40
# kind (the name between gpemu_predict_ and _enqueue / _collect) -> the outputs of its collect in argument order, and
# which of them its collect refuses to go without (mean+variance: both)
OUTPUTS = {"batch": ("mean", "var"), "mean": ("mean",), "mean_grad": ("mean", "grad"), "var_grad": ("mean", "var", "grad")}
REQUIRED = {"batch": ("mean", "var"), "mean": ("mean",), "mean_grad": ("grad",), "var_grad": ("grad",)}
KINDS = tuple(OUTPUTS)
# the same kinds as methods of abi.Context: synchronous call, enqueue, collect, _dev form
METHODS = {"batch": ("predict", "predict_enqueue", "predict_collect", "predict_dev"),
           "mean": ("predict_mean", "predict_mean_enqueue", "predict_mean_collect", "predict_mean_dev"),
           "mean_grad": ("predict_mean_grad", "predict_mean_grad_enqueue", "predict_mean_grad_collect", "predict_mean_grad_dev"),
           "var_grad": ("predict_var_grad", "predict_var_grad_enqueue", "predict_var_grad_collect", "predict_var_grad_dev")}


def named(kind, res):
    """what a Context method of the kind returned, by output name"""
    return dict(zip(OUTPUTS[kind], res if isinstance(res, tuple) else (res,)))


def same(got, want, names=None):
    for n in want if names is None else names:
        assert got[n].shape == want[n].shape and np.array_equal(got[n], want[n]), n


def enqueue(c, kind, Xq):
    """the kind's C enqueue -> return code"""
    Xq = np.ascontiguousarray(Xq, dtype=np.float64)
    return getattr(c.L, f"gpemu_predict_{kind}_enqueue")(c.h, Xq.shape[0], abi._p(Xq))


def collect(c, kind, M, null=()):
    """the kind's C collect for M queries, NULL for the outputs named in `null` -> (return code, outputs by name)"""
    out = {n: np.full((M, D) if n == "grad" else M, np.nan) for n in OUTPUTS[kind]}
    rc = getattr(c.L, f"gpemu_predict_{kind}_collect")(c.h, M, *[None if n in null else abi._p(out[n]) for n in OUTPUTS[kind]])
    return rc, {n: a for n, a in out.items() if n not in null}


@pytest.fixture(scope="module")
def fixed():
    """the model, 1500 queries, one context, and every kind's synchronous results for the first 40 queries"""
    X, y, th = model(KIND, ORDER, N, D)
    Xq = special_queries(X, 1500, D, 31)
    c = abi.Context(0)
    setup(c, KIND, ORDER, X, y, th)
    want = {k: named(k, getattr(c, METHODS[k][0])(Xq[:M0])) for k in KINDS}
    for k in KINDS:
        assert all(np.all(np.isfinite(a)) for a in want[k].values())
    yield dict(X=X, y=y, th=th, Xq=Xq, c=c, want=want)
    c.close()


@pytest.fixture
def c(fixed):
    """the module's context with the model set anew: whatever an earlier test left behind is gone"""
    setup(fixed["c"], KIND, ORDER, fixed["X"], fixed["y"], fixed["th"])
    return fixed["c"]


# ------------------------------------------------------------------ 1. the 4 x 4 matrix
@pytest.mark.parametrize("kind", KINDS)
def test_only_its_own_collect_takes_a_batch(fixed, c, kind):
    Xq = fixed["Xq"][:M0]
    assert enqueue(c, kind, Xq) == abi.OK
    for other in KINDS:
        if other != kind:
            assert collect(c, other, M0)[0] == abi.ERR_STATE, other
            assert enqueue(c, other, Xq) == abi.ERR_STATE, other          # ... and the batch is still there
    for any_kind in KINDS:
        assert enqueue(c, any_kind, Xq) == abi.ERR_STATE, any_kind         # one batch of any kind at a time
    rc, got = collect(c, kind, M0)
    assert rc == abi.OK
    same(got, fixed["want"][kind])
    assert collect(c, kind, M0)[0] == abi.ERR_STATE                        # taken


# ------------------------------------------------------------------ 2. refusals that leave the batch pending
@pytest.mark.parametrize("kind", KINDS)
def test_wrong_size_is_refused(fixed, c, kind):
    assert enqueue(c, kind, fixed["Xq"][:M0]) == abi.OK
    for M in (M0 - 1, M0 + 1):
        assert collect(c, kind, M)[0] == abi.ERR_STATE, M
        for other in KINDS:                                                 # (the size is looked at before the kind)
            assert collect(c, other, M)[0] == abi.ERR_STATE, (other, M)
    rc, got = collect(c, kind, M0)
    assert rc == abi.OK
    same(got, fixed["want"][kind])


@pytest.mark.parametrize("kind", KINDS)
def test_missing_required_output_is_refused(fixed, c, kind):
    assert enqueue(c, kind, fixed["Xq"][:M0]) == abi.OK
    for n in REQUIRED[kind]:
        assert collect(c, kind, M0, null=(n,))[0] == abi.ERR_ARG, n
    assert collect(c, kind, M0, null=OUTPUTS[kind])[0] == abi.ERR_ARG
    for other in KINDS:                                                     # an argument error comes before a state error
        if other != kind:
            assert collect(c, other, M0, null=REQUIRED[other][:1])[0] == abi.ERR_ARG, other
    rc, got = collect(c, kind, M0)
    assert rc == abi.OK
    same(got, fixed["want"][kind])


@pytest.mark.parametrize("kind,null", [("mean_grad", ("mean",)), ("var_grad", ("mean",)), ("var_grad", ("var",)),
                                       ("var_grad", ("mean", "var"))])
def test_optional_outputs(fixed, c, kind, null):
    assert enqueue(c, kind, fixed["Xq"][:M0]) == abi.OK
    rc, got = collect(c, kind, M0, null=null)
    assert rc == abi.OK
    assert set(got) == set(OUTPUTS[kind]) - set(null)
    same(got, fixed["want"][kind], names=got)
    assert collect(c, kind, M0)[0] == abi.ERR_STATE                        # taken


# ------------------------------------------------------------------ 3. nothing pending, no set-up, a new model
def test_collect_with_nothing_enqueued(c):
    for kind in KINDS:
        assert collect(c, kind, M0)[0] == abi.ERR_STATE, kind


def test_enqueue_before_setup(fixed):
    ctx = abi.Context(0)
    try:
        ctx.set_model(KIND, ORDER, fixed["X"], fixed["y"])
        for kind in KINDS:
            assert enqueue(ctx, kind, fixed["Xq"][:M0]) == abi.ERR_STATE, kind
            assert collect(ctx, kind, M0)[0] == abi.ERR_STATE, kind
    finally:
        ctx.close()


@pytest.mark.parametrize("pending", KINDS)
def test_set_model_drops_the_batch(fixed, c, pending):
    Xq = fixed["Xq"][:M0]
    assert enqueue(c, pending, Xq) == abi.OK
    c.set_model(KIND, ORDER, fixed["X"], fixed["y"])
    for kind in KINDS:
        assert collect(c, kind, M0)[0] == abi.ERR_STATE, kind
        assert enqueue(c, kind, Xq) == abi.ERR_STATE, kind                 # no set-up for the new model yet
    _, rc = c.predict_setup(fixed["th"])
    assert rc == abi.OK
    for kind in KINDS:
        assert collect(c, kind, M0)[0] == abi.ERR_STATE, kind              # the set-up brought nothing back
        assert enqueue(c, kind, Xq) == abi.OK, kind
        rc, got = collect(c, kind, M0)
        assert rc == abi.OK
        same(got, fixed["want"][kind])


# ------------------------------------------------------------------ 4. the staging grows, and both forms of the copy back
def test_staging_regrowth_and_both_copy_forms(fixed, c):
    """40, 1500, 40, 1 queries through every kind's two halves on one context whose staging starts empty: 1500 moves the
    staging past the 1024 queries up to which means and variances come back in one copy and regrows the pinned buffers, the
    second 40 and the 1 run in the larger ones.  Each result against the kind's _dev form on uploaded queries, and against
    the first rows of the kind's own 1500-query result (queries are independent; at N = 150 the mean+variance kind never
    splits K, so its single query runs the launches of the 1500 and is compared like the rest)."""
    Xq = fixed["Xq"]
    Mmax = Xq.shape[0]
    offs = {"mean": Mmax * D, "var": Mmax * (D + 1), "grad": Mmax * (D + 2)}        # in doubles, behind the coordinates
    buf = c.dev_alloc(Mmax * (2 * D + 2) * 8)
    big = {}
    try:
        for M in (M0, Mmax, M0, 1):
            c.upload(buf, Xq[:M])
            for kind in KINDS:
                _, enq, col, dev = (getattr(c, m) for m in METHODS[kind])
                enq(Xq[:M])
                got = named(kind, col())
                c.upload(buf.value + offs["mean"] * 8, np.full(Mmax * (D + 2), np.nan))
                dev(M, buf, *[buf.value + offs[n] * 8 for n in OUTPUTS[kind]])
                c.sync()
                same(got, {n: c.download(buf.value + offs[n] * 8, got[n].shape) for n in OUTPUTS[kind]})
                if M == Mmax:
                    big[kind] = got
                elif kind in big:
                    same(got, {n: a[:M] for n, a in big[kind].items()})
                if M == M0:
                    same(got, fixed["want"][kind])
        for kind in KINDS:                       # the first 40 ran before the 1500: against its rows now
            same(fixed["want"][kind], {n: a[:M0] for n, a in big[kind].items()})
    finally:
        c.dev_free(buf)
