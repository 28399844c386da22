"""tests/designbatchref.py checks itself (CPU): the conditional IMSE gains of greedy batches in numpy fp64, pinned
against the same form in mpmath at 50 digits, against tensor quadrature of the conditioned senspostref.cstar^2 (no closed form)
and against the identity they stand for: the running sum of the pick gains is s_all of the design minus s_all of the design
with the picks appended, for every prefix of the picks; and the state the device carries (lambda, mu, E) gives the same
conditional values as the direct V^-1 form.

Settings: those of test_designref.py (N <= 12, d in {1, 2, 3}, orders 0 .. 2, nugget 1e-3, a, b, v from a numpy fit; uniform,
all-Gaussian and mixed measures), its six candidates (one on a design point), four picks.

Bars.  test_designref.py's NP_MP_BAR = 128 * 2^-52 * max(1, max_l 1 / (s_l w_l^2)) bounds the error relative to the sum of the
absolute values of the TERMS; the scales here are the sums of the PARTS, as the GPU tests use them, and test_designref.py
records that for these random models the parts' sum is up to 2150 times smaller than the terms' (a^T K a cancels inside).
CANCEL = 4096 covers that factor: the bar here is CANCEL * NP_MP_BAR, for the refit identity times 8 for the fits' inverses
(as there); the quadrature's floor of 1e-13 there (its own convergence and the fp64 error of cstar, both on the terms' scale)
takes the same factor."""
import numpy as np
import pytest

import designbatchref as DB
import designref as D
import sensref as R
import test_designref as TD

NUGGET = TD.NUGGET
CANCEL = 4096
K = 4
CASES = [(9, 1, 2), (7, 2, 1), (12, 2, 2), (11, 3, 1)]


def inputs(N, d, order, measure):
    X, m, kind, lo, hi, w, Xq = TD.setting(N, d, order, measure)
    a, b, v, _ = D.fit_ab(X, order, m["A"], m["s"], NUGGET, Xq)
    return X, m, kind, lo, hi, w, Xq, a, b, v


@pytest.mark.parametrize("measure", ["design", "gauss", "mixed"])
@pytest.mark.parametrize("N,d,order", CASES)
def test_numpy_against_mpmath_and_quadrature(N, d, order, measure):
    X, m, kind, lo, hi, w, Xq, a, b, v = inputs(N, d, order, measure)
    pc = DB.pieces(R.NP, X, m, lo, hi, kind, Xq, a, b)
    pm = DB.pieces(R.MP(), X, m, lo, hi, kind, Xq, a, b)
    t = CANCEL * TD.bar(m, w)
    e_sig = float(np.max(np.abs(pc[0] - R.MP.tofloat(pm[0])) / pc[2]))
    e_g = float(np.max(np.abs(pc[1] - R.MP.tofloat(pm[1])) / pc[3]))
    assert np.allclose(pc[0], pc[0].T, rtol=0, atol=t * pc[2].max()) and np.allclose(pc[1], pc[1].T, rtol=0, atol=t * pc[3].max())
    # G(q, q) is designref's num, Sigma(q, q) + nugget the variance
    val, scale, _ = D.gain(R.NP, X, m, lo, hi, kind, Xq, a, b, v)
    assert np.all(np.abs(np.diag(pc[1]) - val["num"]) <= t * scale["num"])
    assert np.allclose(np.diag(pc[0]) + NUGGET, v, rtol=1e-9, atol=0)
    g = DB.greedy([pc], [v], NUGGET, K)
    worst, worst_q = 0.0, 0.0
    for j in range(K + 1):
        S = g["S"][0][:j]
        cn, cs = DB.conditional(R.NP, *pc, v, NUGGET, S)
        cm, _ = DB.conditional(R.MP(), *pm, v, NUGGET, S)
        worst = max(worst, DB.scaled_errors(cn, cm, cs))
        qn, qv = DB.quadrature_num(X, m, order, NUGGET, lo, hi, kind, Xq, S)
        worst_q = max(worst_q, float(np.max(np.abs(cn["num"] - qn) / cs["num"])), float(np.max(np.abs(cn["var"] - qv) / cs["var"])))
    print(f"N {N} d {d} order {order} {measure}: Sigma {e_sig:.2e}, G {e_g:.2e}, conditional {worst:.2e}, quadrature {worst_q:.2e} (bar {t:.1e})")
    assert e_sig < t and e_g < t and worst < t
    assert worst_q < max(CANCEL * 1e-13, t)


@pytest.mark.parametrize("measure", ["design", "gauss", "mixed"])
@pytest.mark.parametrize("N,d,order", CASES)
def test_refit_identity_for_every_prefix(N, d, order, measure):
    """sum of the first j pick gains = s_all(design) - s_all(design + the first j picks); the gains are positive and decrease no
    faster than the picks allow: every pick's gain is at most the first pick's"""
    X, m, kind, lo, hi, w, Xq, a, b, v = inputs(N, d, order, measure)
    pc = DB.pieces(R.NP, X, m, lo, hi, kind, Xq, a, b)
    g = DB.greedy([pc], [v], NUGGET, K)
    assert len(set(g["pick"])) == K and g["pick"][0] == int(np.argmax(g["gain_first"]))
    diff, dscale = DB.refit(X, m, order, NUGGET, lo, hi, kind, Xq, g["pick"])
    run, rscale = np.cumsum(g["pick_gain"]), np.cumsum(g["pick_scale"])
    gap = float(np.max(np.abs(run - diff) / (dscale + rscale)))
    t = 8 * CANCEL * TD.bar(m, w)
    print(f"N {N} d {d} order {order} {measure}: picks {g['pick']}, refit gap {gap:.2e} (bar {t:.1e})")
    assert gap < t
    assert np.all(g["pick_gain"] > 0) and np.all(g["pick_gain"][1:] <= g["pick_gain"][0] + t * g["pick_scale"][1:])
    assert np.all(np.isneginf(g["gain_last"][g["pick"]])) and np.all(np.isfinite(np.delete(g["gain_last"], g["pick"])))


@pytest.mark.parametrize("N,d,order", CASES)
def test_the_carried_state_gives_the_direct_form(N, d, order):
    """v - |lambda|^2 and num - 2 lambda . mu + lambda^T E lambda against the direct V^-1 form"""
    X, m, kind, lo, hi, w, Xq, a, b, v = inputs(N, d, order, "design")
    pc = DB.pieces(R.NP, X, m, lo, hi, kind, Xq, a, b)
    g = DB.greedy([pc], [v], NUGGET, K)
    S = g["S"][0]
    (lam, mu, E), (ls, ms, es) = DB.state(*pc, v, NUGGET, S)
    cn, cs = DB.conditional(R.NP, *pc, v, NUGGET, S)
    var = v - (lam * lam).sum(axis=1)
    num = np.diag(pc[1]) - 2 * (lam * mu).sum(axis=1) + np.einsum("qi,ij,qj->q", lam, E, lam)
    t = CANCEL * TD.bar(m, w)
    assert np.all(np.abs(var - cn["var"]) <= t * cs["var"]) and np.all(np.abs(num - cn["num"]) <= t * cs["num"])
    assert np.allclose(np.diag(E), g["pick_gain"], rtol=0, atol=t * g["pick_scale"].max())
    assert np.all(ls > 0) and np.all(ms > 0) and np.all(np.diag(es) > 0)


def test_two_contexts_and_weights():
    """the weighted sum decides: with all weight on one context the picks are that context's own"""
    X, m, kind, lo, hi, w, Xq, a, b, v = inputs(12, 2, 2, "design")
    m2 = dict(m, s=m["s"] * 2.5)
    a2, b2, v2, _ = D.fit_ab(X, 2, m2["A"], m2["s"], NUGGET, Xq)
    p1, p2 = DB.pieces(R.NP, X, m, lo, hi, kind, Xq, a, b), DB.pieces(R.NP, X, m2, lo, hi, kind, Xq, a2, b2)
    own = DB.greedy([p2], [v2], NUGGET, K)
    both = DB.greedy([p1, p2], [v, v2], NUGGET, K, weight=[0.0, 3.0])
    assert np.array_equal(own["pick"], both["pick"]) and np.allclose(both["pick_gain"], 3.0 * own["pick_gain"], rtol=1e-14, atol=0)
    mix = DB.greedy([p1, p2], [v, v2], NUGGET, K, weight=[1.0, 0.5])
    assert np.allclose(mix["pick_gain"], mix["pick_gain_ctx"] @ np.array([1.0, 0.5]), rtol=1e-14, atol=0)


@pytest.mark.parametrize("weight", [None, [1.0, 0.5]])
def test_forced_on_the_reference_own_picks_is_greedy(weight):
    """`forced` takes the picks as an input; given greedy's own picks it returns greedy's numbers bit for bit: every pick's gain and
    scale, per context and weighted, the pick itself as the arg-max among the candidates not yet picked, gain_first and gain_last"""
    X, m, kind, lo, hi, w, Xq, a, b, v = inputs(12, 2, 2, "design")
    m2 = dict(m, s=m["s"] * 2.5)
    a2, b2, v2, _ = D.fit_ab(X, 2, m2["A"], m2["s"], NUGGET, Xq)
    pcs = [DB.pieces(R.NP, X, m, lo, hi, kind, Xq, a, b), DB.pieces(R.NP, X, m2, lo, hi, kind, Xq, a2, b2)]
    vs = [v, v2]
    if weight is None:
        pcs, vs = pcs[:1], vs[:1]
    nb = len(Xq)                                                                              # every candidate: the design point among them
    g = DB.greedy(pcs, vs, NUGGET, nb, weight)
    conditions = [[s in g["S"][c] for s in g["pick"]] for c in range(len(pcs))]
    for j in range(nb + 1):
        f = DB.forced(pcs, vs, NUGGET, g["pick"], j, weight, conditions)
        assert f["S"] == [[s for s in g["S"][c] if s in set(g["pick"][:j])] for c in range(len(pcs))]
        if j == 0:
            assert np.array_equal(f["tot"], g["gain_first"])
        if j == nb:
            assert np.all(np.isneginf(g["gain_last"])) and np.array_equal(f["tot_scale"], g["last_scale"])
            continue
        s = g["pick"][j]
        assert f["tot"][s] == g["pick_gain"][j] and f["tot_scale"][s] == g["pick_scale"][j]
        assert np.array_equal(f["gain"][s], g["pick_gain_ctx"][j]) and np.array_equal(f["gain_scale"][s], g["pick_scale_ctx"][j])
        free = np.ones(nb, dtype=bool)
        free[g["pick"][:j]] = False
        assert s == int(np.argmax(np.where(free, f["tot"], -np.inf)))
        if j:
            (lam, mu, E), _ = f["state"][0]
            (rl, rm, rE), _ = DB.state(*pcs[0], vs[0], NUGGET, f["S"][0])
            assert np.array_equal(lam, rl) and np.array_equal(mu, rm) and np.array_equal(E, rE)
    short = DB.greedy(pcs, vs, NUGGET, 3, weight)                                             # a shorter batch: gain_last of the candidates left
    f = DB.forced(pcs, vs, NUGGET, short["pick"], 3, weight)
    free = np.ones(nb, dtype=bool)
    free[short["pick"]] = False
    assert np.array_equal(f["tot"][free], short["gain_last"][free])


@pytest.mark.parametrize("N,d,order", CASES)
def test_the_carried_recurrence_is_the_direct_form(N, d, order):
    """`carried` (the recurrences the device uses, the base of the leave-out tests) against `state` and `conditional`"""
    X, m, kind, lo, hi, w, Xq, a, b, v = inputs(N, d, order, "design")
    pc = DB.pieces(R.NP, X, m, lo, hi, kind, Xq, a, b)
    S = DB.greedy([pc], [v], NUGGET, K)["S"][0]
    lam, mu, E, vS, numS, gain = DB.carried(pc[0], pc[1], v, NUGGET, S)
    (rl, rm, rE), (ls, ms, es) = DB.state(*pc, v, NUGGET, S)
    cn, cs = DB.conditional(R.NP, *pc, v, NUGGET, S)
    t = CANCEL * TD.bar(m, w)
    assert np.all(np.abs(lam - rl) <= t * ls) and np.all(np.abs(mu - rm) <= t * ms) and np.all(np.abs(E - rE) <= t * es)
    assert np.all(np.abs(vS - cn["var"]) <= t * cs["var"]) and np.all(np.abs(numS - cn["num"]) <= t * cs["num"])
    assert np.all(np.abs(gain - cn["gain"]) <= t * cs["gain"])


def test_two_identical_candidates():
    """of two identical candidates the lower index is picked, and its twin gains next to nothing afterwards"""
    X, m, kind, lo, hi, w, Xq, a, b, v = inputs(11, 3, 1, "design")
    g0 = DB.greedy([DB.pieces(R.NP, X, m, lo, hi, kind, Xq, a, b)], [v], NUGGET, 1)
    Xd = np.vstack([Xq, Xq[g0["pick"][0]][None, :]])
    a, b, v, _ = D.fit_ab(X, 1, m["A"], m["s"], NUGGET, Xd)
    pc = DB.pieces(R.NP, X, m, lo, hi, kind, Xd, a, b)
    g = DB.greedy([pc], [v], NUGGET, 2)
    assert g["pick"][0] == g0["pick"][0]                                                      # the lower index of the two equal gains
    cn, _ = DB.conditional(R.NP, *pc, v, NUGGET, g["S"][0][:1])
    assert 0 <= cn["gain"][-1] < 1e-2 * g["pick_gain"][0]
