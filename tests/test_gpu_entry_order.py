"""Every entry after every other on one context: the state machine around the kernels (include/gpemu.h).

A gpemu_ctx keeps about two dozen pieces of state -- flags, serial numbers, block sizes, a resident joint factor, a target
store, a calibration table, a measure, a prior, a pending batch -- each invalidated by a rule of its own, and about ten scratch
buffers shared between otherwise unrelated entries.  The other GPU modules test each entry against a new set-up; this one
runs the probes of tests/entryorder.py against each other.  The criterion everywhere is bit equality with `fresh`: the same
probe on new contexts straight after their set-up ("the same inputs always give bit-identical outputs": no tolerance).

  1. pairs        P, Q, P on one long-lived rig for every ordered pair of probes (model A in full, model B a reduced list)
  2. sizes        200 -> 5 -> 70 with another entry of the same buffer family in between, and upwards on a new rig
  3. new set-up   other thetas, another training vector, another model and back: the new state's bits, then the old ones again
  4. later components of gpemu_predict_setup_batch: every probe equals the single set-up; the explicit inverse and the
                  posterior sensitivity entries leave the joint factor, the design block, the targets and a pending batch alone
  5. pending      a batch of each of the four kinds enqueued across every probe: refused (the catalogue's list, the header's) or
                  the fresh bits, and the collect returns the bits of an undisturbed batch
  6. disturbers   what the header says invalidates does (GPEMU_ERR_STATE, outputs untouched) and what it says survives does;
                  what it says leaves the context alone leaves every probe's bits
  7. two rigs     models A and B taking turns on one device

`fresh` is always made by gpemu_predict_setup on each new context, for the two-context probes too -- not by
gpemu_predict_setup_batch, on purpose: case 4 then compares every context of a batch set-up with it, which is the header's
"bit for bit" claim itself, and every other case has one reference.

Case 4's joint-draw half fails on the library before this change: ensure_corner went through gpemu_predict_setup on a later
component and dropped the joint factor.  Observed with that library, all four cases of
test_explicit_inverse_on_a_later_component_keeps_the_joint_factor (the rest of case 4 passes there):
  AssertionError: a draw behind cinverse: joint_draw_only on ('A', (1, 2), 0.0): rc 6 ("gpemu error 6: no resident joint
  factor: call gpemu_predict_joint_factor first") with keys ['rc'] against rc 0 with keys ['draw', 'rc']
and the same behind sens_post, sens_pairs_post and sens_post_mixed.

Wall time on one MI355X: 8.9 s for the module's 212 cases (about 13 000 probe calls, 0.7 ms each at N <= 257); the slowest case
is test_pairs_model_a[predict_1] at 0.81 s, the first to run, which also makes the fresh outputs of all probes on new contexts.
"""
import contextlib

import numpy as np
import pytest

import entryorder as E
from madaiemulator_amd import abi

pytestmark = pytest.mark.gpu

_FRESH = {}


def fresh(key, name):
    """probe `name` on new contexts straight after the set-up `key` says (model, training columns, theta shift): computed once"""
    if (key, name) not in _FRESH:
        _FRESH[(key, name)] = E.fresh_output(key, name)
    return _FRESH[(key, name)]


def check(rig, name, where):
    """run the probe on the rig; its output must be what the rig's history says: the fresh bits, or a refusal that wrote nothing"""
    try:
        want = rig.expected(name, fresh)
        refused_first = ("setup" in E.ALL[name].needs and not rig.ready)
        got, untouched = rig.run(name)
        assert E.same(got, want), f"{where}: {name} on {rig.key()}: {E.first_difference(got, want)}"
        if refused_first:
            assert got["rc"] == abi.ERR_STATE and untouched, f"{where}: {name} was refused but wrote into its outputs"
        return got
    except BaseException:
        rig.broken = True                  # (the next test takes a new rig: one failure is reported once)
        raise


@contextlib.contextmanager
def history(rig):
    """what a test does to a rig outside check(): a failure there retires the rig too"""
    try:
        yield rig
    except BaseException:
        rig.broken = True
        raise


def check_all(rig, where, names=None):
    for n in (E.PROBES if names is None else names):
        check(rig, n, where)


@pytest.fixture(scope="module")
def rigs():
    """the long-lived rigs, one per model: every case below adds to their history"""
    made = {}

    def get(name):
        if name in made and made[name].broken:
            made.pop(name).close()
        if name not in made:
            made[name] = E.Rig(E.model(name)).install().setup()
        return made[name]
    yield get
    for r in made.values():
        r.close()


# ---------------------------------------------------------------------------------------------------- 1. pairs
def _pairs(rig, P, names):
    for Q in names:
        check(rig, P, f"{P} before {Q}")
        check(rig, Q, f"{Q} after {P}")
        check(rig, P, f"{P} after {Q}")


@pytest.mark.parametrize("P", E.PROBES)
def test_pairs_model_a(rigs, P):
    _pairs(rigs("A"), P, E.PROBES)


@pytest.mark.parametrize("P", E.REDUCED_B)
def test_pairs_model_b(rigs, P):
    _pairs(rigs("B"), P, E.REDUCED_B)


# ---------------------------------------------------------------------------------------------------- 2. sizes
@pytest.mark.parametrize("mname", ["A", "B"])
@pytest.mark.parametrize("fam", E.SIZED_FAMILIES)
def test_sizes_down_and_up(rigs, fam, mname):
    rig = rigs(mname)
    for M in (200, 5, 70):
        check(rig, f"{fam}_{M}", f"{fam} at {M} going down")
        check(rig, E.BETWEEN[fam], f"{E.BETWEEN[fam]} between the sizes of {fam}")
    new = E.Rig(E.model(mname)).install().setup()
    try:
        for M in (1, 5, 70, 200):
            check(new, f"{fam}_{M}", f"{fam} at {M} going up on a new rig")
            check(new, E.BETWEEN[fam], f"{E.BETWEEN[fam]} between the sizes of {fam}, new rig")
    finally:
        new.close()


# ---------------------------------------------------------------------------------------------------- 3. a new set-up in the middle
@pytest.mark.parametrize("mname", ["A", "B"])
def test_new_thetas_and_back(rigs, mname):
    rig = rigs(mname)
    check_all(rig, "at theta_1")
    rig.setup(E.THETA2_SHIFT)
    check_all(rig, "at theta_2")
    # no probe that depends on the set-up may still show its theta_1 value: the two fresh outputs differ, so equality with
    # the theta_2 one (checked above) excludes it
    k1, k2 = (mname, rig.ys, 0.0), rig.key()
    stale = [n for n in E.PROBES if "setup" in E.ALL[n].needs and fresh(k1, n)["rc"] == abi.OK and E.same(fresh(k1, n), fresh(k2, n))]
    assert not stale, f"theta_2 does not change {stale}: the case cannot see a stale value there"
    rig.setup(0.0)
    check_all(rig, "back at theta_1")


@pytest.mark.parametrize("mname", ["A", "B"])
def test_new_training_vector_and_back(rigs, mname):
    with history(rigs(mname)) as rig:
        m = rig.m
        check(rig, "joint_70", "before set_training")
        check(rig, "target_gain_70", "before set_training")
        rig.ctxs[0].set_training(m.Y[:, 2])
        rig.ys, rig.ready, rig.joint = (2, 1), False, None
        check_all(rig, "after set_training, before the set-up")                 # refused, nothing written; the tables still answer
        rig.setup()
        check_all(rig, "after set_training and a set-up")                        # the targets' coordinates and weights were kept
        k1, k2 = (mname, (0, 1), 0.0), rig.key()
        stale = [n for n in ("predict_70", "predict_mean_70", "loo", "pred_state", "joint_70") if E.same(fresh(k1, n), fresh(k2, n))]
        assert not stale
        rig.ctxs[0].set_training(m.Y[:, 0])
        rig.ys, rig.ready, rig.joint = (0, 1), False, None
        rig.setup()
        check_all(rig, "back on the first training vector")


def test_another_model_and_back(rigs):
    """A -> C -> A through gpemu_set_model: the calibration table survives it (gpemu.h at gpemu_calib_setup); the targets, the
    joint factor and a pending batch do not (gpemu_design_target_*, gpemu_predict_joint_*, gpemu_predict_batch_enqueue)"""
    with history(rigs("A")) as rig:
        a, c = E.model("A"), E.model("C")
        for m in (c, a):
            check(rig, "joint_70", "before set_model")
            check(rig, "target_gain_70", "before set_model")
            rig.ctxs[0].predict_enqueue(rig.m.Xq[5])
            rig.set_model(m)
            rig.prior = False                                                    # (a prior of the other d: the sampler must refuse)
            assert np.array_equal(rig.ctxs[0].sens_get_measure(), np.zeros(m.d, dtype=np.int32))
            with pytest.raises(abi.GpemuError) as e:
                rig.ctxs[0].predict_collect()
            assert e.value.code == abi.ERR_STATE
            check_all(rig, f"model {m.name}, before the set-up")                # calib_eval answers from the table that survived
            rig.setup()
            check_all(rig, f"model {m.name}, set up, the prior still of the other d")
            rig.ctxs[0].sample_set_prior(*m.prior)
            rig.prior = True
            check_all(rig, f"model {m.name}")


# ---------------------------------------------------------------------------------------------------- 4. later components of a batch set-up
@pytest.fixture(scope="module")
def batch():
    """three contexts on model A's design through gpemu_predict_setup_batch; two rigs over the later components, each of them
    once as the first context of a rig"""
    m = E.model("A")
    ctxs = [abi.Context(0) for _ in range(3)]
    ctxs[0].set_model(m.kind, m.order, m.X, m.Y[:, 0])
    r12 = E.Rig(m, (1, 2), ctxs[1:]).install()
    r21 = E.Rig(m, (2, 1), ctxs[:0:-1])
    r21.set_tables()
    r01 = E.Rig(m, (0, 1), ctxs[:2])                  # the first context, in whose workspace the batch is factored
    r01.set_tables()

    def setup():
        beta, info, status, rc = abi.predict_setup_batch(ctxs, np.array(m.ths))
        assert rc == abi.OK and not np.any(status) and not np.any(info)
        for r in (r12, r21, r01):
            r.after_batch_setup()
    yield r12, r21, r01, setup
    for c in ctxs:
        c.close()


def test_later_components_equal_single_setups(batch):
    """the header's "bit for bit" at gpemu_predict_setup_batch, for every entry: fresh is a gpemu_predict_setup of each context"""
    r12, r21, r01, setup = batch
    setup()
    check_all(r12, "ctxs[1] of a batch set-up")
    check_all(r21, "ctxs[2] of a batch set-up")
    check_all(r01, "ctxs[0] of a batch set-up")
    setup()
    check_all(r01, "ctxs[0] of a second batch set-up")
    check_all(r21, "ctxs[2] of a second batch set-up")
    check_all(r12, "ctxs[1] of a second batch set-up")


@pytest.mark.parametrize("X", ["cinverse", "sens_post", "sens_pairs_post", "sens_post_mixed"])
def test_explicit_inverse_on_a_later_component_keeps_the_joint_factor(batch, X):
    """the factor stays "until the next factor call, release, set_model, set_training, set_mode, predict_setup[_batch]": X is
    none of those, on ctxs[0] or on a later component"""
    r12, _, _, setup = batch
    setup()
    check(r12, "joint_70", "the factor")
    check(r12, X, "X behind the factor")
    assert r12.joint == "joint_70"
    check(r12, "joint_draw_only", f"a draw behind {X}")
    check(r12, X, "X again")
    check(r12, "joint_draw_only", f"a draw behind the second {X}")


@pytest.mark.parametrize("X", ["cinverse", "sens_post", "sens_pairs_post"])
def test_explicit_inverse_on_a_later_component_keeps_everything_else(batch, X):
    r12, _, _, setup = batch
    setup()
    kept = ("predict_var_grad_70", "design_gain_70", "target_gain_70", "target_gain_only")
    check_all(r12, f"before {X}", kept)
    undisturbed = {}
    for kind, outs in (("predict", 2), ("predict_var_grad", 3)):
        getattr(r12.ctxs[0], kind + "_enqueue")(r12.m.Xq[70])
        undisturbed[kind] = getattr(r12.ctxs[0], kind + "_collect")()
    setup()
    check_all(r12, f"before {X}, second set-up", kept)
    r12.ctxs[0].predict_var_grad_enqueue(r12.m.Xq[70])
    check(r12, X, "X while a batch is pending")
    got = r12.ctxs[0].predict_var_grad_collect()
    assert all(g.tobytes() == u.tobytes() for g, u in zip(got, undisturbed["predict_var_grad"]))
    check_all(r12, f"after {X}", kept[::-1])
    setup()
    r12.ctxs[0].predict_enqueue(r12.m.Xq[70])
    check(r12, X, "X while a batch is pending, third set-up")
    got = r12.ctxs[0].predict_collect()
    assert all(g.tobytes() == u.tobytes() for g, u in zip(got, undisturbed["predict"]))


# ---------------------------------------------------------------------------------------------------- 5. a pending batch across everything
PENDING = dict(batch=("predict_enqueue", "predict_collect"), mean=("predict_mean_enqueue", "predict_mean_collect"),
               mean_grad=("predict_mean_grad_enqueue", "predict_mean_grad_collect"), var_grad=("predict_var_grad_enqueue", "predict_var_grad_collect"))


def _tuple(x):
    return x if isinstance(x, tuple) else (x,)


@pytest.mark.parametrize("mname", ["A", "B"])
@pytest.mark.parametrize("kind", sorted(PENDING))
def test_a_pending_batch_across_every_probe(rigs, kind, mname):
    with history(rigs(mname)) as rig:
        c, Xq = rig.ctxs[0], rig.m.Xq[70]
        enq, col = (getattr(c, n) for n in PENDING[kind])
        enq(Xq)
        undisturbed = _tuple(col())
        for chunk in (E.PROBES[:len(E.PROBES) // 2], E.PROBES[len(E.PROBES) // 2:], E.PROBES[::-1]):
            enq(Xq)
            for n in chunk:
                if n in E.REFUSES_PENDING:
                    got, untouched = rig.run(n)
                    assert got == dict(rc=abi.ERR_STATE) and untouched, f"{n} while a {kind} batch is pending: {got}"
                else:
                    check(rig, n, f"while a {kind} batch is pending")
            got = _tuple(col())
            assert len(got) == len(undisturbed) and all(g.tobytes() == u.tobytes() for g, u in zip(got, undisturbed)), f"the {kind} batch"
        check_all(rig, "after the collects")


@pytest.mark.parametrize("dname", sorted(set(E.DISTURBERS) - {"set_model"}))
def test_a_pending_batch_across_every_disturber(rigs, dname):
    """gpemu_set_model alone drops a pending batch (gpemu.h at gpemu_predict_batch_enqueue): behind every other disturber the
    collect returns the bits the batch was enqueued for, a new set-up and a lost set-up included; gpemu_predict_setup_batch
    refuses while a batch is pending and changes nothing"""
    d = E.DISTURBERS[dname]
    with history(rigs("A")) as rig:
        if dname == "predict_setup_batch":
            check(rig, "joint_70", "a factor for the refused batch set-up to leave alone")
        c, Xq = rig.ctxs[0], rig.m.Xq[70]
        c.predict_var_grad_enqueue(Xq)
        undisturbed = c.predict_var_grad_collect()
        c.predict_var_grad_enqueue(Xq)
        if dname == "predict_setup_batch":
            with pytest.raises(abi.GpemuError) as e:
                d.fn(rig)
            assert e.value.code == abi.ERR_STATE
            check_all(rig, "behind a refused batch set-up", [n for n in E.PROBES if n not in E.REFUSES_PENDING])
        else:
            d.apply(rig)
        got = c.predict_var_grad_collect()
        assert all(g.tobytes() == u.tobytes() for g, u in zip(got, undisturbed)), f"the batch pending across {dname}"
        rig.restore()
        check_all(rig, f"after a batch pending across {dname}")


def test_a_batch_pending_on_a_later_context_refuses_the_batch_setup_and_touches_none(rigs):
    """the batch is pending on ctxs[1]: gpemu_predict_setup_batch refuses "before any context is touched", ctxs[0], which it
    looked at first, included -- every probe on ctxs[0] still answers, a draw from its resident joint factor among them"""
    with history(rigs("A")) as rig:
        m, (c0, c1) = rig.m, rig.ctxs
        check(rig, "joint_70", "the factor on ctxs[0]")
        check(rig, "target_gain_70", "the targets on ctxs[0]")
        c1.predict_enqueue(m.Xq[70])
        undisturbed = c1.predict_collect()
        c1.predict_enqueue(m.Xq[70])
        for ctxs in (rig.ctxs, [c0, c1, c0]):                                   # (the second: a context listed twice behind a good one)
            with pytest.raises(abi.GpemuError) as e:
                abi.predict_setup_batch(ctxs, np.array([rig.thetas(0), rig.thetas(1), rig.thetas(0)][:len(ctxs)]))
            assert e.value.code in (abi.ERR_STATE, abi.ERR_ARG)
            assert rig.joint == "joint_70" and rig.ready
            # (the probes that take ctxs[1] through its host-buffer entries are refused by its pending batch, as in case 5)
            check_all(rig, "ctxs[0] behind a refused batch set-up", [n for n in E.PROBES if E.ALL[n].family not in ("calib_grad", "calib_select")])
        got = c1.predict_collect()
        assert all(g.tobytes() == u.tobytes() for g, u in zip(got, undisturbed))
        check_all(rig, "after the collect")


# ---------------------------------------------------------------------------------------------------- 6. disturbers
@pytest.mark.parametrize("mname", ["A", "B"])
@pytest.mark.parametrize("dname", sorted(E.DISTURBERS))
def test_disturber(rigs, dname, mname):
    d = E.DISTURBERS[dname]
    with history(rigs(mname)) as rig:
        for n in ("joint_70", "target_gain_70", "predict_var_grad_70", "cinverse", "design_gain_70"):     # something to lose
            check(rig, n, f"before {dname}")
        d.apply(rig)
        check_all(rig, f"straight after {dname}")
        if not (rig.ready and rig.calib and rig.prior):
            rig.restore()
            check_all(rig, f"after {dname} and what it needs to be set up again")
        # the joint factor and the targets again, for whoever comes next
        check(rig, "joint_70", f"after {dname}")
        check(rig, "joint_draw_only", f"after {dname}")


def test_the_measure_survives_where_the_header_says(rigs):
    """gpemu_set_training, gpemu_predict_setup[_batch] and gpemu_sens_release keep the kinds; gpemu_set_model resets them"""
    with history(rigs("A")) as rig:
        m = rig.m
        for c in rig.ctxs:
            c.sens_set_measure(m.mkind)
        try:
            for dname in ("set_training", "predict_setup", "predict_setup_batch", "sens_release", "loglik", "design_target_release"):
                E.DISTURBERS[dname].apply(rig)
                assert all(np.array_equal(c.sens_get_measure(), m.mkind) for c in rig.ctxs), dname
            rig.restore()
            got, _ = E.run_probe(lambda ctxs, mm: dict(E.p_sens_cov(ctxs, mm, mm.glo, mm.ghi)), rig.ctxs, m)
            want = dict(fresh(rig.key(), "sens_cov_mixed"))
            want.pop("measure")
            assert E.same(got, want), E.first_difference(got, want)
            E.DISTURBERS["set_model"].apply(rig)
            assert all(np.array_equal(c.sens_get_measure(), np.zeros(m.d, dtype=np.int32)) for c in rig.ctxs)
        finally:
            for c in rig.ctxs:
                c.sens_set_measure(None)
        rig.restore()
        check_all(rig, "after the measure's round trip")


# ---------------------------------------------------------------------------------------------------- 7. two rigs taking turns
def test_two_models_take_turns(rigs):
    ra, rb = rigs("A"), rigs("B")
    n = len(E.PROBES)
    for i, name in enumerate(E.PROBES):
        check(ra, name, "A, taking turns with B")
        check(rb, E.PROBES[(i + 7) % n], "B, taking turns with A")
    for i, name in enumerate(E.PROBES[::-1]):
        check(rb, name, "B, taking turns with A, backwards")
        check(ra, E.PROBES[(i + 11) % n], "A, taking turns with B, backwards")


def test_two_training_vectors_on_one_design_take_turns(rigs):
    """two rigs of model A whose first contexts hold different training vectors: gpemu_design_batch and the two-context
    sensitivity forms over both, in turns"""
    ra = rigs("A")
    rb = E.Rig(E.model("A"), (2, 1)).install().setup()
    try:
        for i, name in enumerate(E.PROBES):
            check(ra, name, "columns (0, 1)")
            check(rb, E.PROBES[(i + 5) % len(E.PROBES)], "columns (2, 1)")
    finally:
        rb.close()
