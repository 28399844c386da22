"""Greedy batches of K runs (gpemu_design_batch, include/gpemu.h) through the public entries, against
tests/designbatchref.py (numpy fp64; test_designbatchref.py pins it against mpmath, against quadrature of the conditioned c*^2 and
against the refit identity for every prefix of the picks).

What is compared.  As in test_gpu_design.py the reference starts from the device's own a and b (gpemu_test_design_state) and var
(gpemu_design_gain, whose bits the first pass carries); Sigma and G of all pairs of candidates, the conditional gains in the
direct V^-1 form, the greedy picks and the state (lambda, mu, E by a Cholesky factor of V) are the reference's own.  Errors are
relative to the scales designbatchref.py defines (the sums of the absolute values of the parts, extended to the cross terms
and the corrections).

The bars.  Measured on the CPU over exactly the cases of this file (`all_cases()`, a, b and var from a numpy fit) by
`python tests/designbatchref.py --measure`; the device gets FACTOR = 8 times each, as in test_gpu_design.py:
  NP_VS_MP = 2.4e-13  the largest scaled error of the numpy reference against mpmath at 50 digits over the conditional num, var
                      and gain of every candidate (every prefix of the picks up to 8, then every 8th and the last), Sigma and G
                      (the narrow box, in G and the conditional values; 5.7e-14 on N = 64, d = 3, order 2; most cases sit at
                      4e-16 to 5e-14; Sigma alone 3.4e-14 at most)                                          -> TOL = 1.9e-12
  REFIT_NP = 9.6e-18  the largest gap |sum of the first j pick gains - (s_all - s_all')| over the sum of the values' scales,
                      N + j points refitted in numpy, j = 1, 2, nbatch (the narrow box; 1.4e-18 to 7.2e-18 elsewhere)
                                                                                                            -> REFIT_TOL = 7.7e-17
The same run prints every case's smallest MARGIN between the best and the second-best weighted gain over all picks, relative to
the two candidates' scales: every case kept here has margins above 2 TOL (the sum of the two candidates' bars), so the device's
picks must equal the reference's; no pick is left undecided (the kept cases' smallest margins: 4.5e-11 for `wide`, 8.0e-11 for
`three-contexts`, 1.2e-10 and more elsewhere).  Dropped for their margins: see DROPPED."""
import ctypes as C

import numpy as np
import pytest

import designbatchref as DB
import designref as D
import sensref as R
import sensmeasureref as SM
import senspostref as SP
import test_gpu_design as TD
import test_gpu_sens_measure as TM
import test_gpu_sens_post as TP
from madaiemulator_amd import abi, synth

NP_VS_MP = 2.4e-13
REFIT_NP = 9.6e-18
FACTOR = 8
TOL = FACTOR * NP_VS_MP
REFIT_TOL = FACTOR * REFIT_NP
NUGGET = TP.NUGGET

pytestmark = pytest.mark.gpu

# name: (N, d, order, M, nbatch, box or measure, number of contexts)
SHAPES = {
    "one": (1, 1, 0, 1, 1, "design", 1),
    "two": (63, 2, 1, 2, 2, "design", 1),
    "ragged": (64, 3, 2, 63, 3, "design", 1),
    "all-picked-64": (65, 8, 3, 64, 64, "design", 1),
    "all-picked-65": (130, 17, 1, 65, 65, "design", 1),
    "wide": (200, 8, 0, 200, 64, "design", 1),
    "dense": (130, 3, 2, 200, 65, "design", 1),
    "narrow": (130, 3, 1, 65, 3, "narrow", 1),
    "gauss": (65, 2, 1, 64, 3, "gauss", 1),
    "mixed": (130, 3, 2, 64, 3, "mixed", 1),
    "three-contexts": (65, 2, 1, 63, 3, "design", 3),
    "three-contexts-d8": (200, 8, 1, 65, 2, "mixed", 3),
    "duplicate": (64, 3, 1, 64, 3, "design", 1),
    "design-point": (20, 2, 1, 12, 12, "design", 1),
}
# name: why.  130 points in 3 dimensions leave so little variance that after some 50 picks the best two of 200 candidates gain the same
# to 3.3e-13 of their scales: below 2 TOL = 3.8e-12, the pick would be undecided.  (nbatch = 65 stays in `all-picked-65`, M = 200 in `wide`.)
# `design-point`: nugget 0, candidates 8 .. 11 are design points 3, 3, 11, 11 (see case()).  Their var is 0 up to a few ulp of
# either sign and their num likewise: gain is 0 or noise over noise, on a scale of 1 / var.  --measure prints a smallest margin of 0 for it (two of them gain exactly 0):
# no pick among them is decided, so the case cannot be compared pick by pick; test_design_points_with_nugget_0 asserts on the device
# what IS decided there.
DROPPED = {"dense": "smallest margin 3.3e-13 < 2 TOL", "design-point": "smallest margin 0 < 2 TOL"}
WEIGHTS = [1.0, 0.25, 2.5]


# ---------------------------------------------------------------------------------------------------- inputs
def case(name):
    N, d, o, M, nbatch, where, nctx = SHAPES[name]
    X, y = TP.data(N, d)
    if where in ("gauss", "mixed"):
        kind = TM.kinds(where, d)
        lo, hi = TM.measure_of(kind, X)
    else:
        kind = TD.uniform(d)
        lo, hi = R.boxes(X)[where]
    Xq = TD.candidates(X, M, 11)
    th = TP.thetas(d)
    nugget, twin, reg = NUGGET, None, np.arange(M)
    if name == "duplicate":
        # two identical candidate rows, and they are the leading pick: the last row becomes a copy of the candidate that gains most
        # (found here in numpy; the third-best is 6e-8 of the scales behind, so the device's leader is the same)
        m = TP.model_of(th)
        a, b, v, _ = D.fit_ab(X, o, m["A"], m["s"], NUGGET, Xq)
        lead = int(np.argmax(D.gain(R.NP, X, m, lo, hi, kind, Xq, a, b, v)[0]["gain"]))
        other = M - 1 if lead != M - 1 else 0
        Xq[other] = Xq[lead]
        twin = (min(lead, other), max(lead, other))
    if name == "design-point":
        # nugget 0 (exp(-800) is 0.0) on a sparse design with short lengths (C stays well conditioned without a nugget); eight
        # candidates off the design, then design points 3 and 11, each twice
        th = np.array([0.0, -800.0] + [np.log(0.15)] * d)
        nugget, reg = 0.0, np.arange(8)
        Xq[8:] = X[[3, 3, 11, 11]]
    ths = [th + np.concatenate([[0.0, 0.0], 0.12 * c * (-1) ** c * np.ones(d)]) for c in range(nctx)]
    ys = [y, 0.5 * y + X[:, 0], y * y][:nctx]
    return dict(name=name, X=X, ys=ys, ths=ths, o=o, kind=kind, lo=lo, hi=hi, Xq=Xq, nbatch=nbatch, weight=WEIGHTS[:nctx] if nctx > 1 else None,
                nugget=nugget, twin=twin, reg=reg)


def all_cases():
    return [case(n) for n in SHAPES if n not in DROPPED]


def tie(pc, v, twin):
    """two identical candidate rows (identical bits of a and b on the device): the reference's numbers of the second are made copies
    of the first's, so that its tie is as exact as the device's and goes to the lower index there too"""
    if twin is None:
        return pc, v
    i, k = twin
    v = np.array(v, dtype=float)
    v[k] = v[i]
    out = []
    for arr in pc:
        arr = np.array(arr)
        arr[k, :] = arr[i, :]
        arr[:, k] = arr[:, i]
        arr[k, k] = arr[i, i]
        out.append(arr)
    return tuple(out), v


# ---------------------------------------------------------------------------------------------------- the CPU figures
def _prefixes(nb):
    return sorted(set(list(range(0, min(nb, 8) + 1)) + list(range(8, nb + 1, 8)) + [nb]))


def _measure_one(name):
    c = case(name)
    X, o, kind, lo, hi, Xq, nb = c["X"], c["o"], c["kind"], c["lo"], c["hi"], c["Xq"], c["nbatch"]
    nugget = c["nugget"]
    pcs, pms, vs = [], [], []
    e_sig = e_g = 0.0
    for th in c["ths"]:
        m = TP.model_of(th)
        a, b, v, _ = D.fit_ab(X, o, m["A"], m["s"], nugget, Xq)
        pc, pm = DB.pieces(R.NP, X, m, lo, hi, kind, Xq, a, b), DB.pieces(R.MP(), X, m, lo, hi, kind, Xq, a, b)
        e_sig = max(e_sig, float(np.max(np.abs(pc[0] - R.MP.tofloat(pm[0])) / pc[2])))
        e_g = max(e_g, float(np.max(np.abs(pc[1] - R.MP.tofloat(pm[1])) / pc[3])))
        pc, v = tie(pc, v, c["twin"])
        pcs.append(pc), pms.append(pm), vs.append(v)
    with np.errstate(all="ignore"):
        g = DB.greedy(pcs, vs, nugget, nb, c["weight"], c["twin"])
    if nugget == 0.0:
        # V is singular once a design point is in S: nothing conditional can be compared; Sigma, G and the margins stand
        return name, max(e_sig, e_g), e_sig, e_g, float("nan"), float("nan"), float(np.nanmin(g["margin"]))
    e_c = 0.0
    for ci in range(len(pcs)):
        for j in _prefixes(nb):
            S = [s for s in g["S"][ci] if s in set(g["pick"][:j])]
            cn, cs = DB.conditional(R.NP, *pcs[ci], vs[ci], nugget, S)
            cm, _ = DB.conditional(R.MP(), *pms[ci], vs[ci], nugget, S)
            e_c = max(e_c, DB.scaled_errors(cn, cm, cs))
    gap = 0.0
    w = np.ones(len(pcs)) if c["weight"] is None else np.asarray(c["weight"])
    js = sorted(set([1, min(2, nb), nb]))
    run, rscale = np.cumsum(g["pick_gain"]), np.cumsum(g["pick_scale"])
    diff, dscale = np.zeros(nb), np.zeros(nb)
    for ci, th in enumerate(c["ths"]):
        m = TP.model_of(th)
        for j in js:
            dd, ds = DB.refit(X, m, o, nugget, lo, hi, kind, Xq, g["pick"][:j])
            diff[j - 1] += w[ci] * dd[-1]
            dscale[j - 1] += w[ci] * ds[-1]
    for j in js:
        gap = max(gap, abs(run[j - 1] - diff[j - 1]) / (dscale[j - 1] + rscale[j - 1]))
    return name, max(e_sig, e_g, e_c), e_sig, e_g, e_c, gap, float(g["margin"].min())


def measure():
    """the figures NP_VS_MP and REFIT_NP are set from, and the margins the cases are kept by (CPU, minutes)"""
    import multiprocessing as mpc
    import sys
    names = list(SHAPES)                                                                     # (the dropped cases too: their margins are the reason)
    if "--only" in sys.argv:
        names = sys.argv[sys.argv.index("--only") + 1].split(",")
    worst = refit = 0.0
    with mpc.Pool(min(8, mpc.cpu_count())) as pool:
        for name, e, es, eg, ec, gap, margin in pool.imap_unordered(_measure_one, names):
            print(f"{name}: numpy - mpmath {e:.3e} (Sigma {es:.2e}, G {eg:.2e}, conditional {ec:.2e}), refit gap {gap:.3e}, smallest margin {margin:.3e}",
                  flush=True)
            if name in DROPPED:
                print(f"  ({name} is dropped: {DROPPED[name]})")
                continue
            worst, refit = max(worst, e), max(refit, gap)
    print(f"largest scaled error of numpy against mpmath over {len([n for n in names if n not in DROPPED])} kept cases: {worst:.3e}")
    print(f"largest refit gap in numpy: {refit:.3e}")


# ---------------------------------------------------------------------------------------------------- helpers
@pytest.fixture(scope="module")
def ctxs3(gpu_ctx):
    more = [abi.Context(0), abi.Context(0)]
    yield [gpu_ctx] + more
    for c in more:
        c.close()


@pytest.fixture(scope="module")
def refit_ctx():
    ctx = abi.Context(0)
    yield ctx
    ctx.close()


def setup(ctxs, c):
    """the case's contexts fitted; -> (the contexts used, their models)"""
    use = ctxs[:len(c["ths"])]
    return use, [TD.fit(ctx, c["o"], c["X"], y, th, c["kind"]) for ctx, y, th in zip(use, c["ys"], c["ths"])]


BITS = ("pick", "pick_gain", "pick_gain_ctx", "gain_first", "gain_last")


def same(a, b, keys=BITS):
    return all(np.array_equal(a[k], b[k]) for k in keys)


def run_case(ctxs, c, refit_ctx=None):
    """the case through the host entry against the reference on the device's own a, b and var"""
    name, X, o, kind, lo, hi, Xq, nb, weight = (c[k] for k in ("name", "X", "o", "kind", "lo", "hi", "Xq", "nbatch", "weight"))
    use, models = setup(ctxs, c)
    M, twin = len(Xq), c["twin"]
    firsts = [ctx.design_gain(lo, hi, Xq) for ctx in use]
    got = abi.design_batch(use, lo, hi, Xq, nb, weight)
    pcs, vs = [], []
    for ctx, m, f in zip(use, models, firsts):
        a, b = ctx.design_state(M)
        if twin is not None:
            assert np.array_equal(a[twin[0]], a[twin[1]]) and np.array_equal(b[twin[0]], b[twin[1]]) and f["var"][twin[0]] == f["var"][twin[1]]
        pc, v = tie(DB.pieces(R.NP, X, m, lo, hi, kind, Xq, a, b), f["var"], twin)
        pcs.append(pc)
        vs.append(v)
    ref = DB.greedy(pcs, vs, NUGGET, nb, weight, twin)
    if twin is not None:
        # the exact tie goes to the lower index, and what its twin would still gain collapses
        assert got["pick"][0] == twin[0] and got["gain_first"][twin[0]] == got["gain_first"][twin[1]], (name, got["pick"], twin)
        assert twin[1] not in got["pick"] and 0.0 <= got["gain_last"][twin[1]] < 1e-2 * got["pick_gain"][0], (name, got["gain_last"][twin[1]])
    print(f"{name}: picks {got['pick'][:8]} ..., smallest margin {ref['margin'].min():.2e} (2 TOL {2 * TOL:.1e})")
    assert ref["margin"].min() > 2 * TOL, (name, ref["margin"].min())
    assert np.array_equal(got["pick"], ref["pick"]), (name, got["pick"], ref["pick"])
    w = np.ones(len(use)) if weight is None else np.asarray(weight, float)
    e_pick = float(np.max(np.abs(got["pick_gain"] - ref["pick_gain"]) / ref["pick_scale"]))
    e_ctx = float(np.max(np.abs(got["pick_gain_ctx"] - ref["pick_gain_ctx"]) / ref["pick_scale_ctx"]))
    free = np.ones(M, dtype=bool)
    free[ref["pick"]] = False
    assert np.all(np.isneginf(got["gain_last"][~free]))
    e_last = float(np.max(np.abs(got["gain_last"][free] - ref["gain_last"][free]) / ref["last_scale"][free])) if free.any() else 0.0
    print(f"{name}: scaled errors pick_gain {e_pick:.2e}, pick_gain_ctx {e_ctx:.2e}, gain_last {e_last:.2e} (bar {TOL:.1e})")
    assert e_pick < TOL and e_ctx < TOL and e_last < TOL, (name, e_pick, e_ctx, e_last)
    if len(use) == 1:
        assert np.array_equal(got["gain_first"], firsts[0]["gain"]), name
        assert got["pick"][0] == int(np.argmax(firsts[0]["gain"])), name
    # the carried state of every context
    for ci, ctx in enumerate(use):
        lam, mu, E = ctx.design_batch_state(M, nb)
        S = ref["S"][ci]
        col = [int(np.flatnonzero(ref["pick"] == s)[0]) for s in S]
        (rl, rm, rE), (ls, ms, es) = DB.state(*pcs[ci], vs[ci], NUGGET, S)
        e_l = float(np.max(np.abs(lam[:, col] - rl) / ls))
        e_m = float(np.max(np.abs(mu[:, col] - rm) / ms))
        e_E = float(np.max(np.abs(E[np.ix_(col, col)] - rE) / es))
        print(f"{name} context {ci}: scaled errors lambda {e_l:.2e}, mu {e_m:.2e}, E {e_E:.2e} (bar {TOL:.1e})")
        assert e_l < TOL and e_m < TOL and e_E < TOL, (name, ci, e_l, e_m, e_E)
        assert np.array_equal(E, E.T)
    # the refit identity on the device: the running sum of the pick gains against s_all before and after
    if refit_ctx is not None:
        run, rscale = np.cumsum(got["pick_gain"]), np.cumsum(ref["pick_scale"])
        for j in sorted(set([1, min(2, nb), nb])):
            diff = scale = 0.0
            for ci, (ctx, m) in enumerate(zip(use, models)):
                post = ctx.sens_post(lo, hi)
                _, ps = SM.post(kind, R.NP, X, m, *ctx.sens_post_state(), lo, hi)
                X2 = np.vstack([X, Xq[got["pick"][:j]]])
                TD.fit(refit_ctx, o, X2, np.concatenate([c["ys"][ci], 0.5 * np.ones(j)]), c["ths"][ci], kind)
                post2 = refit_ctx.sens_post(lo, hi)
                _, ps2 = SM.post(kind, R.NP, X2, m, *refit_ctx.sens_post_state(), lo, hi)
                diff += w[ci] * (post["s_all"] - post2["s_all"])
                scale += w[ci] * (ps["s_all"] + ps2["s_all"])
            gap = abs(run[j - 1] - diff) / (scale + rscale[j - 1])
            print(f"{name} first {j} picks: sum of gains {run[j - 1]:.6e}, refit {diff:.6e}, gap {gap:.2e} (bar {REFIT_TOL:.1e})")
            assert gap < REFIT_TOL, (name, j, gap)
    return got, ref


# ---------------------------------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize("name", [n for n in SHAPES if n not in DROPPED])
def test_values(ctxs3, refit_ctx, name):
    """tile edges of N, M and nbatch; d = 8, 16 < d; every order; boxes and measures; one and three contexts; the leading pick twice"""
    c = case(name)
    run_case(ctxs3, c, refit_ctx)


def _fma_sub(v, x):
    """v - x * x rounded once"""
    from fractions import Fraction
    return float(Fraction(v) - Fraction(x) * Fraction(x))


def test_design_points_with_nugget_0(gpu_ctx):
    """candidates on design points with nugget 0, every candidate picked.  Their var is 0 up to rounding of either sign, so which of them
    are valid picks is the device's own rounding; asserted is what is decided whatever it is: every output finite; gain 0 where the
    device's own var is <= 0; a pick whose v_S (the device's var less the squares of its own lambda entries, as the update forms it)
    is <= 0 has gain 0, zero columns of lambda and mu and a zero row and column of E, and the picks go on behind it; a valid pick's
    E_jj is its gain; at least one pick takes the v_S <= 0 path; and the candidates off the design are picked in the reference's order
    (a run on a design point without a nugget conditions nothing)."""
    c = case("design-point")
    X, o, kind, lo, hi, Xq, reg = (c[k] for k in ("X", "o", "kind", "lo", "hi", "Xq", "reg"))
    use, (m,) = setup([gpu_ctx], c)
    M = len(Xq)
    first = gpu_ctx.design_gain(lo, hi, Xq)
    got = abi.design_batch(use, lo, hi, Xq, M)
    a, b = gpu_ctx.design_state(M)
    lam, mu, E = gpu_ctx.design_batch_state(M, M)
    print(f"design-point: var of the design points {first['var'][8:]}, their first gains {got['gain_first'][8:]}, picks {got['pick']}")
    for k in ("pick_gain", "pick_gain_ctx", "gain_first"):
        assert np.all(np.isfinite(got[k])), k
    assert np.all(np.isfinite(lam)) and np.all(np.isfinite(mu)) and np.all(np.isfinite(E))
    assert sorted(got["pick"]) == list(range(M)) and np.all(np.isneginf(got["gain_last"]))
    assert np.array_equal(got["gain_first"], first["gain"]) and np.all(first["gain"][first["var"] <= 0.0] == 0.0)
    ninvalid = 0
    for j, s in enumerate(got["pick"]):
        v1 = v2 = first["var"][s]
        for i in range(j):
            v1, v2 = v1 - lam[s, i] * lam[s, i], _fma_sub(v2, lam[s, i])
        invalid = not lam[:, j].any()
        if max(v1, v2) <= 0.0:
            assert invalid, (j, s, v1)
        if min(v1, v2) > 0.0:
            assert not invalid, (j, s, v1)
        if invalid:
            ninvalid += 1
            assert not mu[:, j].any() and not E[j, :].any() and not E[:, j].any() and got["pick_gain"][j] == 0.0, (j, s)
            assert s >= 8, (j, s)
        else:
            assert E[j, j] == got["pick_gain"][j], (j, s)
    print(f"design-point: {ninvalid} of {M} picks on the v_S <= 0 path")
    assert ninvalid >= 1
    pc = DB.pieces(R.NP, X, m, lo, hi, kind, Xq[reg], a[reg], b[reg])
    ref = DB.greedy([pc], [first["var"][reg]], 0.0, len(reg))
    print(f"design-point: the candidates off the design, smallest margin {ref['margin'].min():.2e} (2 TOL {2 * TOL:.1e})")
    assert ref["margin"].min() > 2 * TOL
    mine = [s for s in got["pick"] if s < 8]
    assert mine == list(ref["pick"]), (mine, ref["pick"])
    e = float(np.max(np.abs(got["pick_gain"][got["pick"] < 8] - ref["pick_gain"]) / ref["pick_scale"]))
    print(f"design-point: pick gains of the candidates off the design against the reference without the design points {e:.2e} (bar {TOL:.1e}; not asserted)")


def test_weight_zero_ties_go_to_the_lowest_index(gpu_ctx):
    """all weight 0: every weighted gain is 0 and the picks go on at the lowest index not yet picked, with gain 0 (gains that are 0
    because v_S <= 0: test_design_points_with_nugget_0)"""
    c = case("gauss")
    use, _ = setup([gpu_ctx], c)
    got = abi.design_batch(use, c["lo"], c["hi"], c["Xq"], 5, [0.0])
    assert np.array_equal(got["pick"], np.arange(5)) and np.all(got["pick_gain"] == 0.0)
    assert np.all(got["gain_first"] == 0.0) and np.all(np.isneginf(got["gain_last"][:5])) and np.all(got["gain_last"][5:] == 0.0)


# ---------------------------------------------------------------------------------------------------- 2. bits
def test_same_bits(ctxs3):
    """two calls; a batch of j against the first j picks of a longer one; the host and the _dev entry"""
    c = case("three-contexts")
    use, _ = setup(ctxs3, c)
    lo, hi, Xq, w = c["lo"], c["hi"], c["Xq"], c["weight"]
    M, nc, nb = len(Xq), len(use), 7
    first = abi.design_batch(use, lo, hi, Xq, nb, w)
    states = [ctx.design_batch_state(M, nb) for ctx in use]
    assert same(first, abi.design_batch(use, lo, hi, Xq, nb, w))
    for ctx, st in zip(use, states):
        assert all(np.array_equal(p, q) for p, q in zip(st, ctx.design_batch_state(M, nb)))
    for j in (1, 2, 4):
        short = abi.design_batch(use, lo, hi, Xq, j, w)
        assert all(np.array_equal(short[k], first[k][:j]) for k in ("pick", "pick_gain", "pick_gain_ctx")), j
        assert np.array_equal(short["gain_first"], first["gain_first"])
        for ctx, st in zip(use, states):
            lam, mu, E = ctx.design_batch_state(M, j)
            assert np.array_equal(lam, st[0][:, :j]) and np.array_equal(mu, st[1][:, :j]) and np.array_equal(E, st[2][:j, :j])
    lead = use[0]
    sizes = [Xq.nbytes, nb * 4 + 4, nb * 8, nb * nc * 8, M * 8, M * 8]
    bufs = [lead.dev_alloc(s) for s in sizes]
    try:
        lead.upload(bufs[0], Xq)
        abi.design_batch_dev(use, lo, hi, M, bufs[0], nb, *bufs[1:], weight=w)
        lead.sync()
        dev = dict(pick=lead.download(bufs[1], (nb,), np.int32), pick_gain=lead.download(bufs[2], (nb,)),
                   pick_gain_ctx=lead.download(bufs[3], (nb, nc)), gain_first=lead.download(bufs[4], (M,)),
                   gain_last=lead.download(bufs[5], (M,)))
        assert same(first, dev)
        abi.design_batch_dev(use, lo, hi, M, bufs[0], nb, bufs[1], bufs[2], weight=w)         # the optional outputs may be left out
        lead.sync()
        assert np.array_equal(lead.download(bufs[1], (nb,), np.int32), first["pick"])
    finally:
        for b in bufs:
            lead.dev_free(b)
    # weights of None are weights of 1; the order of the contexts is the order of the sum
    ones = abi.design_batch(use, lo, hi, Xq, 3, [1.0, 1.0, 1.0])
    assert same(ones, abi.design_batch(use, lo, hi, Xq, 3, None))


def test_a_candidate_alone_and_in_a_larger_set(gpu_ctx):
    """the candidates' own numbers do not depend on the set they arrive in: a subset that holds the picks returns their bits"""
    c = case("ragged")
    use, _ = setup([gpu_ctx], c)
    full = abi.design_batch(use, c["lo"], c["hi"], c["Xq"], 3)
    keep = np.sort(np.concatenate([full["pick"], [0, 1, 2, 60]]))
    keep = np.unique(keep)
    sub = abi.design_batch(use, c["lo"], c["hi"], c["Xq"][keep], 3)
    assert np.array_equal(keep[sub["pick"]], full["pick"])
    assert np.array_equal(sub["pick_gain"], full["pick_gain"])
    assert np.array_equal(sub["gain_last"], full["gain_last"][keep]) and np.array_equal(sub["gain_first"], full["gain_first"][keep])


def test_setup_by_batch_same_bits(ctxs3):
    """contexts set up by gpemu_predict_setup_batch against contexts set up alone"""
    c = case("three-contexts")
    use, _ = setup(ctxs3, c)
    alone = abi.design_batch(use, c["lo"], c["hi"], c["Xq"], 3, c["weight"])
    batch = [abi.Context(0) for _ in use]
    try:
        for ctx, y in zip(batch, c["ys"]):
            ctx.set_model(1, c["o"], c["X"], y)
        _, _, status, rc = abi.predict_setup_batch(batch, np.stack(c["ths"]))
        assert rc == abi.OK and np.all(status == abi.OK)
        for ctx in batch:
            ctx.sens_set_measure(c["kind"])
        assert same(alone, abi.design_batch(batch, c["lo"], c["hi"], c["Xq"], 3, c["weight"]))
    finally:
        for ctx in batch:
            ctx.close()


# ---------------------------------------------------------------------------------------------------- 3. neighbours
def test_neighbours_keep_their_bits(gpu_ctx):
    """gpemu_design_gain, gpemu_sens_post and gpemu_predict_var_grad return the bits they returned before; gpemu_sens_release frees
    the state and the next call builds it again"""
    c = case("mixed")
    use, _ = setup([gpu_ctx], c)
    lo, hi, Xq = c["lo"], c["hi"], c["Xq"]
    gain, post, vg = gpu_ctx.design_gain(lo, hi, Xq), gpu_ctx.sens_post(lo, hi), gpu_ctx.predict_var_grad(Xq)
    first = abi.design_batch(use, lo, hi, Xq, 3)
    gain2, post2, vg2 = gpu_ctx.design_gain(lo, hi, Xq), gpu_ctx.sens_post(lo, hi), gpu_ctx.predict_var_grad(Xq)
    assert TD.same(gain, gain2) and TP.same_bits(post, post2) and all(np.array_equal(p, q) for p, q in zip(vg, vg2))
    gpu_ctx.sens_release()
    with pytest.raises(abi.GpemuError) as ei:
        gpu_ctx.design_batch_state(len(Xq), 3)
    assert ei.value.code == abi.ERR_STATE
    assert same(first, abi.design_batch(use, lo, hi, Xq, 3))


# ---------------------------------------------------------------------------------------------------- 4. errors
def test_errors(ctxs3, refit_ctx):
    c = case("three-contexts")
    use, _ = setup(ctxs3, c)
    L, p = use[0].L, abi._p
    lo, hi, Xq = (np.ascontiguousarray(v, dtype=np.float64) for v in (c["lo"], c["hi"], c["Xq"]))
    M, nb, n = len(Xq), 3, len(use)
    pick, pg = np.zeros(nb, dtype=np.int32), np.empty(nb)
    pk = pick.ctypes.data_as(C.c_void_p)
    w = np.array(c["weight"])

    def call(hs, nctx=None, weight=w, lo_=lo, hi_=hi, M_=M, xq=Xq, nb_=nb, pick_=pk, pg_=pg):
        arr = None if hs is None else (C.c_void_p * len(hs))(*hs)
        return L.gpemu_design_batch(arr, len(hs) if nctx is None and hs is not None else (nctx or 0), abi._po(weight), abi._po(lo_), abi._po(hi_),
                                    M_, abi._po(xq), nb_, pick_, abi._po(pg_), None, None, None)

    good = [ctx.h for ctx in use]
    refit_ctx.set_model(1, c["o"], c["X"], c["ys"][0])                                        # a model, no set-up
    for hs in (good, [good[0], refit_ctx.h, good[2]]):                                        # whatever the state
        assert call(None, nctx=3) == abi.ERR_ARG
        assert call(hs, nctx=0) == abi.ERR_ARG
        assert call([hs[0], None, hs[2]]) == abi.ERR_ARG
        assert call(hs, lo_=None) == abi.ERR_ARG and call(hs, hi_=None) == abi.ERR_ARG and call(hs, xq=None) == abi.ERR_ARG
        assert call(hs, pick_=None) == abi.ERR_ARG and call(hs, pg_=None) == abi.ERR_ARG
        assert call(hs, M_=0) == abi.ERR_ARG and call(hs, M_=16385) == abi.ERR_ARG
        assert call(hs, nb_=0) == abi.ERR_ARG and call(hs, nb_=M + 1) == abi.ERR_ARG and call(hs, nb_=-1) == abi.ERR_ARG
    arr = (C.c_void_p * n)(*good)
    assert L.gpemu_design_batch_dev(arr, n, None, p(lo), p(hi), M, None, nb, None, None, None, None, None) == abi.ERR_ARG
    big = np.zeros((300, Xq.shape[1]))
    assert call(good, M_=300, xq=big, nb_=257, pick_=np.zeros(257, dtype=np.int32).ctypes.data_as(C.c_void_p), pg_=np.empty(257)) == abi.ERR_ARG
    # no prediction set-up on one of the contexts: before the Matern model of another is looked at
    assert call([good[0], refit_ctx.h, good[2]]) == abi.ERR_STATE
    refit_ctx.set_model(3, c["o"], c["X"], c["ys"][0])
    _, rc = refit_ctx.predict_setup(synth.default_thetas(3, c["X"].shape[1]))
    assert rc == abi.OK
    use[2].set_model(1, c["o"], c["X"], c["ys"][2])
    assert call([good[0], refit_ctx.h, good[2]]) == abi.ERR_STATE
    TD.fit(use[2], c["o"], c["X"], c["ys"][2], c["ths"][2], c["kind"])
    # a Matern model, a bad box, weights, differing designs, a context twice
    assert call([good[0], refit_ctx.h, good[2]]) == abi.ERR_ARG
    bad = hi.copy()
    bad[1] = lo[1]
    assert call(good, hi_=bad) == abi.ERR_ARG
    for wv in (-1.0, np.nan, np.inf):
        assert call(good, weight=np.array([1.0, wv, 1.0])) == abi.ERR_ARG
    X2 = c["X"].copy()
    X2[0, 0] += 0.01
    TD.fit(refit_ctx, c["o"], X2, c["ys"][0], c["ths"][0], c["kind"])
    assert call([good[0], refit_ctx.h, good[2]]) == abi.ERR_ARG
    assert call([good[0], good[1], good[0]]) == abi.ERR_ARG
    use[1].sens_set_measure([0, 1])
    assert call(good) == abi.ERR_ARG                                                          # differing measures
    for ctx in use:
        ctx.sens_set_measure([0, 1])
    for sd in (0.0, -1.0, np.nan):
        bad = hi.copy()
        bad[1] = sd
        assert call(good, hi_=bad) == abi.ERR_ARG
    for ctx in use:
        ctx.sens_set_measure(None)
    # and the entry works after all that; the state of another size is refused
    assert call(good) == abi.OK and len(set(pick)) == nb
    lam = np.empty((M, nb))
    assert L.gpemu_test_design_batch_state(good[0], M, nb + 1, p(lam), p(lam), p(lam)) == abi.ERR_STATE
    assert L.gpemu_test_design_batch_state(good[0], M, nb, None, p(lam), p(lam)) == abi.ERR_ARG
