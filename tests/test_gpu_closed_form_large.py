"""The closed-form sensitivity, design-gain and greedy-batch entries PAST ONE 256-WIDE TRIP of their kernels (DESIGN.md 4.14, 4.15,
4.16, 4.17, 4.20, 4.22).  Almost every kernel of kernels_sens.hip and kernels_design.hip is 256 threads striding over the design
points, the padded columns Np, the tile partials or the candidates; the other GPU files stop at N = 200, Np = 256, 256 tiles,
M = 200 and nbatch = 65.  The shapes here are the smallest that cross each of those lines:

  n257          N 257, d 3, order 2   Np = 320: one element in the second trip of every N-sum and in the second column block
  n321-d8       N 321, d 8, order 1   Np = 384, the unrolled d <= 8 form
  n1025-full    N 1025, d 2, order 1  289 full-square tiles: sens_finish_kernel, sens_pair_finish_kernel at t > 255
  n1409-lower   N 1409, d 2, order 1  276 lower tiles: the post finishes and sens_lower_tile at t > 255
  nreg63        N 130, d 31, order 2  nreg = 63 (the limit), the rolled d > 16 form
  d64           N 130, d 64, order 0  d = GPEMU_MAX_PARAMS
  design-n257   N 257, d 8, order 1   every design kernel at Np > 256; M = 300: design_argmax_kernel's second trip
  design-n321   N 321, d 3, order 2   the same at Np = 384
  long batches  design-n257, M 300, nbatch 256: design_gather_kernel and design_update_kernel at j >= 64, 128, 192, 255

The band of gpemu_sens_main_var is cut into blocks of 16 384 rows (PRED_BATCH_MAX, gpemu_api.hip): no ngrid below 300 spans two
blocks, so ngrid = 300 stays (901 and 2401 rows: sens_tvec_kernel and sens_band_finish_kernel past 256 rows).

What is compared, as in the files whose helpers this one uses (test_gpu_sens*.py, test_gpu_design*.py): the reference starts from
the device's own beta, gamma, P, G, Q, a, b and var; everything downstream is the reference's, and every value is compared
through the references' scaled_errors on the existing scales.

Long batches cannot be compared pick by pick (the reference's margins fall under the bar long before pick 128), so they are
checked CONDITIONALLY ON THE DEVICE'S OWN PICKS: designbatchref.forced takes the picks as an input and evaluates, non-incrementally,
every candidate's conditional gain given a prefix of them; see test_long_batch.  Where a v_S rounds to <= 0 the reference applies
the device's rule itself (gain 0, designbatchref.conditional), so nothing is skipped for a small v_S.

That each case CAN fail -- that the part past its line is worth more than 100 bars -- is asserted on the CPU by
tests/test_closed_form_large_ref.py.

The bars.  Measured on the CPU over exactly the cases of this file by `python tests/test_gpu_closed_form_large.py --measure`
(beta, gamma, P, G, Q, a, b and var from a numpy fit; mpmath at 50 digits); the device gets FACTOR = 8 times each, as in every
closed-form GPU file: it sums in another order and its erf differs from libm's by a few ulp.
  measured, numpy against mpmath -> bar (the device's largest error over this file):
    plug-in (sens_cov, sens_main)          3.98e-12 -> 3.2e-11  (1.7e-12)      pairs, surface (sens_pairs, sens_joint)  9.88e-13 -> 7.9e-12  (1.3e-12)
    posterior (sens_post, the band)        8.46e-17 -> 6.8e-16  (1.0e-16)      pairs (sens_pairs_post)                  8.76e-18 -> 7.0e-17  (2.4e-17)
    design gain                            5.78e-14 -> 4.6e-13  (2.9e-14)      conditional gains and state              1.46e-13 -> 1.2e-12  (2.2e-13)
Where each figure comes from, the pick margins and what the 50-digit repeat left out for its cost: beside MEASURED below.
Slowest test: the 256 picks of three contexts, 6.3 s, 6.1 s of them the reference's 20 prefixes."""
import os
import sys
import time

if __name__ == "__main__":                       # (`--measure`: the package is one directory up)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import pytest

import designbatchref as DB
import designref as D
import sensmeasureref as M
import senspairref as SPR
import senspostref as SP
import sensref as R
import test_gpu_design as TD
import test_gpu_sens as TS
import test_gpu_sens_measure as TM
import test_gpu_sens_post as TP
from madaiemulator_amd import abi

# family: the largest scaled error of numpy against mpmath at 50 digits over the cases of this file (`--measure`), and where.
# The pairs have figures of their own: on one figure with the entries above them they would be held to a bar 4 and 10 times wider.
MEASURED = {
    "plug": 3.98e-12,        # sens_cov, sens_main: nreg63 (d64 1.0e-12, n257 gauss with two contexts 1.2e-12; n1025-full 4.5e-13; one context at n321-d8 6e-14)
    "post": 8.46e-17,        # sens_post, the band: d64 (n321-d8 5.8e-17, n257 5.7e-17, both in the band at ngrid 300; nreg63 1.7e-17, n1409-lower
                             # 3.7e-18).  All 2401 rows of the band against long double (class LD below); at 50 digits the columns BAND_MP_COLUMNS
                             # of the 300 (on them alone: 4.9e-17, against either reference)
    "pairs_plug": 9.88e-13,  # sens_pairs, sens_joint: n257 gauss with two contexts (n321-d8 6.1e-13, n1025-full 2.8e-13)
    "pairs_post": 8.76e-18,  # sens_pairs_post: n257 uniform (n321-d8 4.1e-18, n1409-lower 3.1e-18)
    "design": 5.78e-14,      # design_gain: design-n257 uniform, M 257 (M 300 5.5e-14, mixed 2.4e-14; design-n321 2.9e-14; nreg63, d64 4.4e-15; M 1 7e-16)
    "cond": 1.46e-13,        # Sigma, G, the conditional gains of every candidate, lambda, mu and E: design-n321, three contexts, eight picks
                             # (design-n257 with 256 picks, at every prefix of PREFIXES: 1.3e-13; nreg63 9.2e-15, d64 3.9e-15)
}
# smallest pick margins of the cases compared pick by pick (`--measure`, numpy fits; the device's own a, b and var give the same to
# the digits shown): design-n257 1.1e-9 (one context), 8.8e-11 (three); design-n321 1.1e-10, 4.1e-11; nreg63 4.5e-6; d64 2.2e-8 --
# all above 2 bars = 2.3e-12, with the candidates of seed CAND_SEED = 11: no case needed another seed.
# The mpmath repeat took 50 digits everywhere (n1409-lower 16 minutes of one core, the 256-pick case 65 minutes per context).

FACTOR = 8
TOL = {k: FACTOR * v for k, v in MEASURED.items()}
NUGGET = TP.NUGGET
WEIGHTS = [1.0, 0.25, 2.5]
CAND_SEED = 11

pytestmark = pytest.mark.gpu

SHAPES = {"n257": (257, 3, 2), "n321-d8": (321, 8, 1), "n1025-full": (1025, 2, 1), "n1409-lower": (1409, 2, 1), "nreg63": (130, 31, 2),
          "d64": (130, 64, 0), "design-n257": (257, 8, 1), "design-n321": (321, 3, 2)}
ENTRY_CASES = ("n257", "n321-d8")
LIMIT_CASES = ("nreg63", "d64")
DESIGN_CASES = ("design-n257", "design-n321")
MEASURES = ("uniform", "gauss", "mixed")
BAND_NGRIDS = (5, 300)
DESIGN_MS = (1, 257, 300)
BATCH_M, BATCH_PICKS, LIMIT_M, LIMIT_PICKS = 300, 8, 65, 3
LONG_CASE, LONG_M, LONG_NBATCH = "design-n257", 300, 256
PREFIXES = list(range(9)) + [63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256]
PAIR_KEYS = ("cov_pair", "joint", "inter", "e0_joint")


# ---------------------------------------------------------------------------------------------------- inputs
def kind_of(mn, d):
    return TD.uniform(d) if mn == "uniform" else TM.kinds(mn, d)


def box_of(mn, kind, X):
    return R.boxes(X)["design"] if mn == "uniform" else TM.measure_of(kind, X)


def plug_inputs(name):
    """-> X, [(y, th) of the context, (y, th) of a second one with other lengths], order.  d > 17: test_gpu_sens_post.py's lengths,
    which grow with d (test_gpu_sens.py's 0.6 would leave k = exp(-40) between neighbours at d = 64)"""
    N, d, o = SHAPES[name]
    if d > 17:
        X, y = TP.data(N, d)
        th = TP.thetas(d)
        return X, [(y, th), (np.cos(2.0 * y) + 0.3 * X[:, 0], th + np.concatenate([[0.0, 0.0], 0.2 * np.ones(d)]))], o
    X, y = TS.data(N, d)
    return X, [(y, TS.thetas(d)), (TS.data(N, d, 1)[1], TS.thetas(d, 0.2))], o


def post_inputs(name):
    N, d, o = SHAPES[name]
    X, y = TP.data(N, d)
    return X, y, TP.thetas(d), o


def band_grids(kind, X, lo, hi):
    glo, ghi = TM.span(kind, lo, hi)
    return [TP.band_grid(X, glo, ghi, ng) for ng in BAND_NGRIDS]


def design_inputs(name, mn, M_, nctx=1):
    """as test_gpu_design_batch.case: the candidates of seed CAND_SEED, contexts that differ in their lengths and training values"""
    N, d, o = SHAPES[name]
    X, y = TP.data(N, d)
    kind = kind_of(mn, d)
    lo, hi = box_of(mn, kind, X)
    th = TP.thetas(d)
    ths = [th + np.concatenate([[0.0, 0.0], 0.12 * c * (-1) ** c * np.ones(d)]) for c in range(nctx)]
    ys = [y, 0.5 * y + X[:, 0], y * y][:nctx]
    return dict(name=f"{name}-{mn}-M{M_}-c{nctx}", X=X, ys=ys, ths=ths, o=o, kind=kind, lo=lo, hi=hi, Xq=TD.candidates(X, M_, CAND_SEED),
                weight=WEIGHTS[:nctx] if nctx > 1 else None)


# ---------------------------------------------------------------------------------------------------- helpers
WORST = {}


def check(what, fam, got, ref, scale, keys):
    e = R.scaled_errors(got, ref, scale, keys)
    WORST[fam] = max(WORST.get(fam, 0.0), e)
    print(f"{what}: scaled error {e:.2e} (bar {TOL[fam]:.1e}, {fam})")
    for k in keys:
        assert np.all(np.isfinite(got[k])), (what, k)
    assert e < TOL[fam], (what, fam, e)
    return e


def check_arrays(what, fam, pairs):
    """pairs: [(got, ref, scale)] arrays"""
    e = max(float(np.max(np.abs(np.asarray(g) - r) / s)) for g, r, s in pairs)
    WORST[fam] = max(WORST.get(fam, 0.0), e)
    print(f"{what}: scaled error {e:.2e} (bar {TOL[fam]:.1e}, {fam})")
    assert all(np.all(np.isfinite(g)) for g, _, _ in pairs) and e < TOL[fam], (what, fam, e)
    return e


@pytest.fixture(scope="module")
def ctxs3(gpu_ctx):
    more = [abi.Context(0), abi.Context(0)]
    yield [gpu_ctx] + more
    for c in more:
        c.close()


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for fam, e in sorted(WORST.items()):
        print(f"largest scaled error of the device over this file, {fam}: {e:.2e} (bar {TOL[fam]:.1e})")


def split(keys):
    return tuple(k for k in keys if k not in PAIR_KEYS and k != "s_pair"), tuple(k for k in keys if k in PAIR_KEYS or k == "s_pair")


# ---------------------------------------------------------------------------------------------------- 1. every entry past N = 256
@pytest.mark.parametrize("mn", MEASURES)
@pytest.mark.parametrize("name", ENTRY_CASES)
def test_plug_entries(ctxs3, name, mn):
    """gpemu_sens_cov (one context and two), _main, _pairs, _joint: sens_kernel_mean, sens_poly_kernel, sens_main_kernel and
    sens_joint_kernel make a second trip over the design points, sens_prep_kernel and sens_pair_prep_kernel a second column block"""
    ctx, second = ctxs3[:2]
    X, fits, o = plug_inputs(name)
    kind = kind_of(mn, X.shape[1])
    lo, hi = box_of(mn, kind, X)
    ma, mb = TS.fit(ctx, o, X, *fits[0]), TS.fit(second, o, X, *fits[1])
    ctx.sens_set_measure(kind)
    second.sens_set_measure(kind)
    for other, m2, what in ((None, ma, f"{name} {mn}"), (second, mb, f"{name} {mn} cross")):
        got = TM.plug_entries(ctx, kind, X, lo, hi, other, dev=False)
        ref, scale, keys = TM.plug_reference(R.NP, kind, X, ma, m2, lo, hi)
        own, pair = split(keys)
        check(what, "plug", got, ref, scale, own)
        check(what + " pairs", "pairs_plug", got, ref, scale, pair)
        if other is None:
            TM.plug_ordered(what, got, scale, TOL["plug"] + TOL["pairs_plug"])


@pytest.mark.parametrize("mn", MEASURES)
@pytest.mark.parametrize("name", ENTRY_CASES)
def test_post_entries(gpu_ctx, name, mn):
    """gpemu_sens_post, _pairs_post and the band with 5 and with 300 values per coordinate (d ngrid + 1 = 901 and 2401 rows:
    sens_tvec_kernel, sens_band_finish_kernel); sens_post_finish_kernel and sens_pair_post_finish_kernel at i > 255"""
    X, y, th, o = post_inputs(name)
    kind = kind_of(mn, X.shape[1])
    lo, hi = box_of(mn, kind, X)
    m = TP.fit(gpu_ctx, o, X, y, th)
    gpu_ctx.sens_set_measure(kind)
    got = TM.post_entries(gpu_ctx, kind, X, lo, hi, dev=False)
    P, G, Q = gpu_ctx.sens_post_state()
    beta, gamma = gpu_ctx.pred_state()
    ref, scale, keys = TM.post_reference(R.NP, kind, X, m, P, G, Q, beta, gamma, lo, hi)
    own, pair = split(keys)
    check(f"{name} {mn}", "post", got, ref, scale, own)
    check(f"{name} {mn} pairs", "pairs_post", got, ref, scale, pair)
    for grid in band_grids(kind, X, lo, hi):
        main, var, ve0 = gpu_ctx.sens_main_var(lo, hi, grid)
        bref, bscale = M.band(kind, R.NP, X, m, P, G, Q, beta, gamma, lo, hi, grid)
        check(f"{name} {mn} band ngrid {grid.shape[1]}", "post", dict(main=main, var=var, var_e0=ve0), bref, bscale, ("var", "var_e0", "main"))
        assert abs(ve0 - got["s_none"]) <= 2 * TOL["post"] * (scale["s_none"] + bscale["var_e0"])


# ---------------------------------------------------------------------------------------------------- 2. more than 256 tiles
def test_n1025_full_square_tiles(ctxs3):
    """289 tiles of the full square: sens_finish_kernel and sens_pair_finish_kernel add partials 256 .. 288 in a second trip;
    one context, and two with different lengths (s != t)"""
    ctx, second = ctxs3[:2]
    X, fits, o = plug_inputs("n1025-full")
    lo, hi = R.boxes(X)["design"]
    ma, mb = TS.fit(ctx, o, X, *fits[0]), TS.fit(second, o, X, *fits[1])
    for other, m2, what in ((None, ma, "n1025-full"), (second, mb, "n1025-full cross")):
        got = ctx.sens_cov(lo, hi, other)
        ref, scale = R.covariances(R.NP, X, ma, m2, lo, hi)
        check(what, "plug", got, ref, scale, R.KEYS)
        pref, pscale = SPR.pair_covariances(R.NP, X, ma, m2, lo, hi)
        check(what + " pairs", "pairs_plug", dict(cov_pair=ctx.sens_pairs(lo, hi, other)), pref, pscale, ("cov_pair",))


def test_n1409_lower_tiles(gpu_ctx):
    """276 lower tiles: sens_lower_tile at t > 255 (sens_pmat_kernel and both weighted sweeps), the post finishes' second trip"""
    X, y, th, o = post_inputs("n1409-lower")
    lo, hi = R.boxes(X)["design"]
    m = TP.fit(gpu_ctx, o, X, y, th)
    got = gpu_ctx.sens_post(lo, hi)
    P, G, Q = gpu_ctx.sens_post_state()
    ref, scale = SP.post(R.NP, X, m, P, G, Q, lo, hi)
    check("n1409-lower", "post", got, ref, scale, SP.KEYS)
    TP.ordered("n1409-lower", got, scale)
    pref, pscale = SPR.pair_post(R.NP, X, m, P, G, Q, lo, hi)
    check("n1409-lower pairs", "pairs_post", dict(s_pair=gpu_ctx.sens_pairs_post(lo, hi)), pref, pscale, ("s_pair",))


# ---------------------------------------------------------------------------------------------------- 3. design gain, short batches
def gain_case(ctx, c):
    """gpemu_design_gain against designref on the device's own a, b and var -> (got, scale)"""
    m = TD.fit(ctx, c["o"], c["X"], c["ys"][0], c["ths"][0], c["kind"])
    Mq = len(c["Xq"])
    got = ctx.design_gain(c["lo"], c["hi"], c["Xq"])
    a, b = ctx.design_state(Mq)
    ref, scale, _ = D.gain(R.NP, c["X"], m, c["lo"], c["hi"], c["kind"], c["Xq"], a, b, got["var"])
    assert np.all(np.isfinite(got["var"])) and np.all(got["var"] > 0)
    check(c["name"], "design", got, ref, scale, D.KEYS)
    return got, scale


@pytest.mark.parametrize("mn", ["uniform", "mixed"])
@pytest.mark.parametrize("name", DESIGN_CASES)
def test_design_gain(gpu_ctx, name, mn):
    """gain, num and var at Np > 256 (design_kmat_kernel, _hk_, _kvec_, _cross_, _finish_ past four tile columns) with one candidate,
    257 and 300; var against the prediction's variance where the k-vector clamp holds nothing back (test_gpu_design.properties)"""
    for Mq in DESIGN_MS:
        c = design_inputs(name, mn, Mq)
        got, scale = gain_case(gpu_ctx, c)
        if Mq == DESIGN_MS[-1]:
            TD.properties(gpu_ctx, (c["name"], c["X"], c["ys"][0], c["ths"][0], c["o"], c["kind"], c["lo"], c["hi"], c["Xq"]), got, scale)


def batch_case(ctxs, c, nbatch):
    """gpemu_design_batch pick by pick against designbatchref.greedy, as test_gpu_design_batch.run_case, at this file's bar"""
    name, X, o, kind, lo, hi, Xq, weight = (c[k] for k in ("name", "X", "o", "kind", "lo", "hi", "Xq", "weight"))
    use = ctxs[:len(c["ths"])]
    models = [TD.fit(ctx, o, X, y, th, kind) for ctx, y, th in zip(use, c["ys"], c["ths"])]
    Mq, tol = len(Xq), TOL["cond"]
    firsts = [ctx.design_gain(lo, hi, Xq) for ctx in use]
    got = abi.design_batch(use, lo, hi, Xq, nbatch, weight)
    pcs, vs = [], []
    for ctx, m, f in zip(use, models, firsts):
        a, b = ctx.design_state(Mq)
        pcs.append(DB.pieces(R.NP, X, m, lo, hi, kind, Xq, a, b))
        vs.append(f["var"])
    ref = DB.greedy(pcs, vs, NUGGET, nbatch, weight)
    print(f"{name}: picks {got['pick'][:8]} ..., smallest margin {ref['margin'].min():.2e} (2 bars {2 * tol:.1e})")
    assert ref["margin"].min() > 2 * tol, (name, ref["margin"].min())
    assert np.array_equal(got["pick"], ref["pick"]), (name, got["pick"], ref["pick"])
    free = np.ones(Mq, dtype=bool)
    free[ref["pick"]] = False
    assert np.all(np.isneginf(got["gain_last"][~free]))
    check_arrays(f"{name} pick_gain, pick_gain_ctx, gain_last", "cond",
                 [(got["pick_gain"], ref["pick_gain"], ref["pick_scale"]), (got["pick_gain_ctx"], ref["pick_gain_ctx"], ref["pick_scale_ctx"]),
                  (got["gain_last"][free], ref["gain_last"][free], ref["last_scale"][free])])
    if len(use) == 1:
        assert np.array_equal(got["gain_first"], firsts[0]["gain"]) and got["pick"][0] == int(np.argmax(firsts[0]["gain"])), name
    for ci, ctx in enumerate(use):
        lam, mu, E = ctx.design_batch_state(Mq, nbatch)
        S = ref["S"][ci]
        col = [int(np.flatnonzero(ref["pick"] == s)[0]) for s in S]
        (rl, rm, rE), (ls, ms, es) = DB.state(*pcs[ci], vs[ci], NUGGET, S)
        check_arrays(f"{name} context {ci} lambda, mu, E", "cond", [(lam[:, col], rl, ls), (mu[:, col], rm, ms), (E[np.ix_(col, col)], rE, es)])
        assert np.array_equal(E, E.T)
    return got, ref


@pytest.mark.parametrize("nctx", [1, 3])
@pytest.mark.parametrize("name", DESIGN_CASES)
def test_design_batch(ctxs3, name, nctx):
    """eight picks out of 300 candidates, one context and three weighted ones: every design kernel at Np > 256, and
    design_argmax_kernel's threads take a second candidate each before the tree (picks beyond index 255 decide)"""
    got, _ = batch_case(ctxs3, design_inputs(name, "uniform", BATCH_M, nctx), BATCH_PICKS)
    print(f"{name}: {int((got['pick'] > 255).sum())} of {BATCH_PICKS} picks beyond candidate 255")


# ---------------------------------------------------------------------------------------------------- 4. nreg = 63, d = 64
@pytest.mark.parametrize("name", LIMIT_CASES)
def test_limits_of_nreg_and_d(ctxs3, name):
    """nreg = 63 and d = GPEMU_MAX_PARAMS = 64 through gpemu_sens_cov, _post, gpemu_design_gain and three picks of a batch"""
    ctx = ctxs3[0]
    X, fits, o = plug_inputs(name)
    lo, hi = R.boxes(X)["design"]
    ma = TS.fit(ctx, o, X, *fits[0])
    ref, scale = R.covariances(R.NP, X, ma, ma, lo, hi)
    check(name, "plug", ctx.sens_cov(lo, hi), ref, scale, R.KEYS)
    X, y, th, o = post_inputs(name)
    m = TP.fit(ctx, o, X, y, th)
    got = ctx.sens_post(lo, hi)
    ref, scale = SP.post(R.NP, X, m, *ctx.sens_post_state(), lo, hi)
    check(name, "post", got, ref, scale, SP.KEYS)
    TP.ordered(name, got, scale)
    c = design_inputs(name, "uniform", LIMIT_M)
    gain_case(ctx, c)
    batch_case(ctxs3, c, LIMIT_PICKS)


# ---------------------------------------------------------------------------------------------------- 5. long batches
def long_inputs(nctx):
    return design_inputs(LONG_CASE, "uniform", LONG_M, nctx)


def check_prefix(what, got, f, j, state_dev, picks):
    """everything asserted of the prefix picks[:j]: the pick gains, that the pick is optimal as far as it is decided, the
    state.  -> the margin of the reference at this pick (inf at the end)"""
    tol = TOL["cond"]
    Mq, nb = len(f["tot"]), len(picks)
    margin = np.inf
    if j < nb:
        s = int(picks[j])
        e_pick = abs(got["pick_gain"][j] - f["tot"][s]) / f["tot_scale"][s]
        e_ctx = float(np.max(np.abs(got["pick_gain_ctx"][j] - f["gain"][s]) / f["gain_scale"][s]))
        free = np.ones(Mq, dtype=bool)
        free[picks[:j]] = False
        assert free[s], (what, j, s)
        cand = np.where(free, f["tot"], -np.inf)
        qb = int(np.argmax(cand))
        short = cand[qb] - f["tot"][s]
        allowed = tol * (f["tot_scale"][qb] + f["tot_scale"][s])
        rest = cand.copy()
        rest[qb] = -np.inf
        if np.isfinite(rest.max()):
            q2 = int(np.argmax(rest))
            margin = (cand[qb] - rest[q2]) / (f["tot_scale"][qb] + f["tot_scale"][q2])
        WORST["cond"] = max(WORST.get("cond", 0.0), e_pick, e_ctx)
        print(f"{what} prefix {j}: pick {s} (reference's best {qb}, margin {margin:.1e}), pick_gain {e_pick:.2e}, pick_gain_ctx {e_ctx:.2e} "
              f"(bar {tol:.1e}); behind the reference's best by {short / (f['tot_scale'][qb] + f['tot_scale'][s]):.1e} of the two scales")
        assert e_pick < tol and e_ctx < tol, (what, j, e_pick, e_ctx)
        assert short <= allowed, (what, j, s, qb, short, allowed)
    if j > 0:
        for ci, (lam, mu, E) in enumerate(state_dev):
            col = [i for i in range(j) if int(picks[i]) in f["S"][ci]]
            (rl, rm, rE), (ls, ms, es) = f["state"][ci]
            check_arrays(f"{what} prefix {j} context {ci} lambda, mu, E", "cond",
                         [(lam[:, col], rl, ls), (mu[:, col], rm, ms), (E[np.ix_(col, col)], rE, es)])
    return margin


@pytest.mark.parametrize("nctx", [1, 3])
def test_long_batch(ctxs3, nctx):
    """256 picks out of 300, checked conditionally on the device's own picks at the prefixes j of PREFIXES (j in {64, 128, 192}: a
    lane of design_update_kernel starts its next trip, j = 255 fills E): pick_gain[j] and pick_gain_ctx[j] are the reference's gain
    of the device's pick j given the device's picks before it; that pick is optimal as far as the bar decides (where the
    reference's margin exceeds the two bars this forces equality); no candidate twice; every one of the 256 picks conditions (none
    on the v_S <= 0 path, and the reference's own v_S of each is above half the nugget); gain_first and gain_last over all
    candidates, -inf at the picked ones; lambda, mu and E of every prefix (the first j columns of the state after 256 picks:
    the first j picks of a longer batch are a batch of j bit for bit, test_gpu_design_batch.test_same_bits)."""
    c = long_inputs(nctx)
    name, X, o, kind, lo, hi, Xq, weight = (c[k] for k in ("name", "X", "o", "kind", "lo", "hi", "Xq", "weight"))
    use = ctxs3[:nctx]
    models = [TD.fit(ctx, o, X, y, th, kind) for ctx, y, th in zip(use, c["ys"], c["ths"])]
    Mq, nb, tol = len(Xq), LONG_NBATCH, TOL["cond"]
    firsts = [ctx.design_gain(lo, hi, Xq) for ctx in use]
    got = abi.design_batch(use, lo, hi, Xq, nb, weight)
    pcs, vs, state_dev = [], [], []
    for ctx, m, f in zip(use, models, firsts):
        a, b = ctx.design_state(Mq)
        pcs.append(DB.pieces(R.NP, X, m, lo, hi, kind, Xq, a, b))
        vs.append(f["var"])
        state_dev.append(ctx.design_batch_state(Mq, nb))
    picks = got["pick"]
    assert len(set(picks.tolist())) == nb and picks.min() >= 0 and picks.max() < Mq, name
    # Every pick must condition.  With nugget > 0 the exact v_S of a pick is at least the nugget (the Schur complement of
    # Sigma_SS + nugget I, Sigma positive semidefinite), nine orders above its rounding.  Asserted on the reference's own v_S of every
    # pick given the picks before it (the squared diagonal of the Cholesky factor of V over the 256 picks) and then on the device: no
    # pick took the v_S <= 0 path, which leaves zero columns of lambda and mu.  So S is every pick, for the reference too.
    for ci, (lam, mu, _) in enumerate(state_dev):
        v_ref = np.diag(np.linalg.cholesky(pcs[ci][0][np.ix_(picks, picks)] + NUGGET * np.eye(nb))) ** 2
        idle = [i for i in range(nb) if not lam[:, i].any() or not mu[:, i].any()]
        print(f"{name} context {ci}: the reference's smallest v_S of a pick {v_ref.min():.2e} (nugget {NUGGET:.0e}); picks on the v_S <= 0 path: {idle}")
        assert v_ref.min() > 0.5 * NUGGET and not idle, (name, ci, v_ref.min(), idle)
    print(f"{name}: {int((picks > 255).sum())} picks beyond candidate 255")
    t0, decided = time.time(), 0
    for j in PREFIXES:
        f = DB.forced(pcs, vs, NUGGET, picks, j, weight, with_state=j > 0)
        st = [(lam[:, :j], mu[:, :j], E[:j, :j]) for lam, mu, E in state_dev]
        margin = check_prefix(name, got, f, j, st, picks)
        decided += margin > 2 * tol
        if j == 0:
            check_arrays(f"{name} gain_first", "cond", [(got["gain_first"], f["tot"], f["tot_scale"])])
            if nctx == 1:
                assert np.array_equal(got["gain_first"], firsts[0]["gain"])
        if j == nb:
            free = np.ones(Mq, dtype=bool)
            free[picks] = False
            assert np.all(np.isneginf(got["gain_last"][~free])) and np.all(np.isfinite(got["gain_last"][free]))
            check_arrays(f"{name} gain_last", "cond", [(got["gain_last"][free], f["tot"][free], f["tot_scale"][free])])
    print(f"{name}: {decided} of {len(PREFIXES) - 1} checked picks decided by the reference's margin; reference part {time.time() - t0:.1f} s")
    for lam, mu, E in state_dev:
        assert np.array_equal(E, E.T)


# ---------------------------------------------------------------------------------------------------- the CPU figures
def _numpy_models(X, fits, o):
    import meanref
    return [TS.model_of(th, *meanref.trained(1, o, X, y, th)) for y, th in fits]


def _m_plug(args):
    name, mn, cross = args
    X, fits, o = plug_inputs(name)
    kind = kind_of(mn, X.shape[1])
    lo, hi = box_of(mn, kind, X)
    ms = _numpy_models(X, fits, o)
    ma, mb = ms[0], ms[1] if cross else ms[0]
    if name in ENTRY_CASES:
        val, scale, keys = TM.plug_reference(R.NP, kind, X, ma, mb, lo, hi)
        mp, _, _ = TM.plug_reference(R.MP(), kind, X, ma, mb, lo, hi)
        own, pair = split(keys)
        return dict(plug=M.scaled_errors(val, mp, scale, own), pairs_plug=M.scaled_errors(val, mp, scale, pair))
    val, scale = R.covariances(R.NP, X, ma, mb, lo, hi)
    mp, _ = R.covariances(R.MP(), X, ma, mb, lo, hi)
    out = dict(plug=R.scaled_errors(val, mp, scale))
    if name == "n1025-full":
        val, scale = SPR.pair_covariances(R.NP, X, ma, mb, lo, hi)
        mp, _ = SPR.pair_covariances(R.MP(), X, ma, mb, lo, hi)
        out["pairs_plug"] = SPR.scaled_errors(val, mp, scale, ("cov_pair",))
    return out


BAND_MP_COLUMNS = [0, 1, 2, 3, 4, 41, 153, 299]   # of the 300 band values per coordinate, those the 50-digit repeat takes


class LD(R.NP):
    """numpy long double (a 64-bit mantissa, eps 1.1e-19) with erf from mpmath: the reference for ALL 2401 rows of the band, which at
    50 digits would take hours (some 1e9 products).  Every figure of the posterior family lies near 1e-16 of its scale, two to
    three orders above what long double resolves; on the columns BAND_MP_COLUMNS `--measure` prints the figure against both (they
    agree to three digits: 3.156e-17 and 3.154e-17 where they differ most)."""

    def __init__(self):
        assert np.finfo(np.longdouble).eps < 2e-19, "long double is no wider than double here"
        R.MP()
        import mpmath
        self.pi = self._ld(mpmath.pi)
        self._derf = np.frompyfunc(lambda a, b: self._ld(R._mp_derf(self._mpf(a), self._mpf(b))), 2, 1)

    @staticmethod
    def _mpf(v):
        import mpmath
        hi = float(v)
        return mpmath.mpf(hi) + mpmath.mpf(float(v - np.longdouble(hi)))

    @staticmethod
    def _ld(x):
        hi = float(x)
        return np.longdouble(hi) + np.longdouble(float(x - hi))

    @staticmethod
    def arr(x):
        return np.asarray(x, dtype=np.longdouble)

    def derf(self, ulo, uhi):
        return np.asarray(self._derf(np.asarray(ulo, dtype=np.longdouble), np.asarray(uhi, dtype=np.longdouble)), dtype=np.longdouble)


def _m_post(args):
    name, mn = args
    X, y, th, o = post_inputs(name)
    kind = kind_of(mn, X.shape[1])
    lo, hi = box_of(mn, kind, X)
    m = TP.model_of(th)
    P, G, Q, beta, gamma, _, _ = SP.fit_state(X, y, o, m["A"], m["s"], NUGGET)
    if name in ENTRY_CASES:
        val, scale, keys = TM.post_reference(R.NP, kind, X, m, P, G, Q, beta, gamma, lo, hi)
        mp, _, _ = TM.post_reference(R.MP(), kind, X, m, P, G, Q, beta, gamma, lo, hi)
        own, pair = split(keys)
        out = dict(post=M.scaled_errors(val, mp, scale, own), pairs_post=M.scaled_errors(val, mp, scale, pair))
        for grid in band_grids(kind, X, lo, hi):
            bv, bs = M.band(kind, R.NP, X, m, P, G, Q, beta, gamma, lo, hi, grid)
            bx, _ = M.band(kind, LD(), X, m, P, G, Q, beta, gamma, lo, hi, grid)               # every value, in long double
            out["post"] = max(out["post"], SP.scaled_errors(bv, bx, bs, keys=("var", "var_e0", "main")))
            cols = BAND_MP_COLUMNS if grid.shape[1] > len(BAND_MP_COLUMNS) else list(range(grid.shape[1]))
            sub = lambda b: dict(var=b["var"][:, cols], main=b["main"][:, cols], var_e0=b["var_e0"])
            bm, _ = M.band(kind, R.MP(), X, m, P, G, Q, beta, gamma, lo, hi, grid[:, cols])    # some values, at 50 digits
            e_mp, e_ld = (SP.scaled_errors(sub(bv), ref, sub(bs), keys=("var", "var_e0", "main")) for ref in (bm, sub(bx)))
            out["post"] = max(out["post"], e_mp)
            out[f"band{grid.shape[1]}_mp_ld"] = f"{e_mp:.3e}/{e_ld:.3e}"
        return out
    val, scale = SP.post(R.NP, X, m, P, G, Q, lo, hi)
    mp, _ = SP.post(R.MP(), X, m, P, G, Q, lo, hi)
    out = dict(post=SP.scaled_errors(val, mp, scale))
    if name == "n1409-lower":
        val, scale = SPR.pair_post(R.NP, X, m, P, G, Q, lo, hi)
        mp, _ = SPR.pair_post(R.MP(), X, m, P, G, Q, lo, hi)
        out["pairs_post"] = SPR.scaled_errors(val, mp, scale, ("s_pair",))
    return out


def _m_design(args):
    name, mn, Mq = args
    c = design_inputs(name, mn, Mq)
    m = TP.model_of(c["ths"][0])
    a, b, v, _ = D.fit_ab(c["X"], c["o"], m["A"], m["s"], NUGGET, c["Xq"])
    val, scale, _ = D.gain(R.NP, c["X"], m, c["lo"], c["hi"], c["kind"], c["Xq"], a, b, v)
    mp, _, _ = D.gain(R.MP(), c["X"], m, c["lo"], c["hi"], c["kind"], c["Xq"], a, b, v)
    return dict(design=D.scaled_errors(val, mp, scale))


def _numpy_pieces(c, B=R.NP, only=None):
    pcs, vs = [], []
    for ci, th in enumerate(c["ths"]):
        if only is not None and ci != only:
            pcs.append(None), vs.append(None)
            continue
        m = TP.model_of(th)
        a, b, v, _ = D.fit_ab(c["X"], c["o"], m["A"], m["s"], NUGGET, c["Xq"])
        pcs.append(DB.pieces(B, c["X"], m, c["lo"], c["hi"], c["kind"], c["Xq"], a, b))
        vs.append(v)
    return pcs, vs


def carried_picks(pcs, vs, nbatch, weight):
    """the greedy picks by the carried recurrences (designbatchref.carried): fast, and picks enough like the device's to measure at"""
    w = np.ones(len(pcs)) if weight is None else np.asarray(weight, float)
    picks = []
    for _ in range(nbatch):
        tot = sum(wc * DB.carried(pc[0], pc[1], v, NUGGET, picks)[5] for wc, pc, v in zip(w, pcs, vs))
        tot[np.array(picks, dtype=int)] = -np.inf
        picks.append(int(np.argmax(tot)))
    return np.array(picks)


def _mp_state(pm, nugget, S):
    mp = R.MP()
    V = pm[0][np.ix_(S, S)] + mp.arr(nugget * np.eye(len(S)))
    L = DB._cholesky(V)
    lam, mu = DB._fsolve(L, pm[0][S, :] + 0).T, DB._fsolve(L, pm[1][S, :] + 0).T
    E = DB._fsolve(L, DB._fsolve(L, pm[1][np.ix_(S, S)] + 0).T.copy())
    return [R.MP.tofloat(x) for x in (lam, mu, E)]


def _m_cond(args):
    """one context of a batch case: Sigma, G, the conditional values and the state at the given prefixes, numpy against mpmath"""
    name, nctx, ci, nbatch, prefixes, Mq = args
    c = design_inputs(name, "uniform", Mq, nctx)
    pcs, vs = _numpy_pieces(c)
    picks = DB.greedy(pcs, vs, NUGGET, nbatch, c["weight"])["pick"] if nbatch <= 8 else carried_picks(pcs, vs, nbatch, c["weight"])
    pm = _numpy_pieces(c, R.MP(), only=ci)[0][ci]
    pc, v = pcs[ci], vs[ci]
    e = max(float(np.max(np.abs(pc[0] - R.MP.tofloat(pm[0])) / pc[2])), float(np.max(np.abs(pc[1] - R.MP.tofloat(pm[1])) / pc[3])))
    for j in prefixes:
        S = [int(s) for s in picks[:j]]
        cn, cs = DB.conditional(R.NP, *pc, v, NUGGET, S)
        cm, _ = DB.conditional(R.MP(), *pm, v, NUGGET, S)
        e = max(e, DB.scaled_errors(cn, cm, cs))
        if j:
            got, scl = DB.state(*pc, v, NUGGET, S)
            ref = _mp_state(pm, NUGGET, S)
            e = max(e, max(float(np.max(np.abs(g - r) / s)) for g, r, s in zip(got, ref, scl)))
        print(f"  ({name} c{nctx} context {ci} prefix {j}: {e:.3e} so far)", flush=True)
    return dict(cond=e)


def _m_margin(args):
    name, nctx, nbatch, Mq = args
    c = design_inputs(name, "uniform", Mq, nctx)
    pcs, vs = _numpy_pieces(c)
    g = DB.greedy(pcs, vs, NUGGET, nbatch, c["weight"])
    return dict(margin=float(g["margin"].min()), picks=g["pick"].tolist())


def _run(task):
    fn, args = task
    t0 = time.time()
    return fn.__name__, args, fn(args), time.time() - t0


def measure():
    """the figures of MEASURED and the margins (CPU; mpmath over every case: the better part of an hour on 8 cores)"""
    import multiprocessing as mpc
    import sys
    from oracle import oracle as O
    O.build()                                                                                 # (meanref.trained fits through liboracle.so: built once here, not by eight workers at a time)
    early, late = [p for p in PREFIXES if p < 191], [p for p in PREFIXES if p >= 191]
    tasks = []
    for nctx in (1, 3):                                                                       # (the longest first)
        for ci in range(nctx):
            tasks += [(_m_cond, (LONG_CASE, nctx, ci, LONG_NBATCH, late, LONG_M)), (_m_cond, (LONG_CASE, nctx, ci, LONG_NBATCH, early, LONG_M))]
    tasks += [(_m_post, ("n1409-lower", "uniform")), (_m_plug, ("n1025-full", "uniform", True)), (_m_plug, ("n1025-full", "uniform", False))]
    tasks += [(_m_post, ("d64", "uniform")), (_m_post, ("nreg63", "uniform")), (_m_plug, ("d64", "uniform", False)), (_m_plug, ("nreg63", "uniform", False))]
    for name in ENTRY_CASES[::-1]:
        for mn in MEASURES:
            tasks += [(_m_plug, (name, mn, True)), (_m_plug, (name, mn, False)), (_m_post, (name, mn))]
    for name in DESIGN_CASES:
        for nctx in (1, 3):
            tasks += [(_m_cond, (name, nctx, ci, BATCH_PICKS, list(range(BATCH_PICKS + 1)), BATCH_M)) for ci in range(nctx)]
            tasks.append((_m_margin, (name, nctx, BATCH_PICKS, BATCH_M)))
        for mn in ("uniform", "mixed"):
            tasks += [(_m_design, (name, mn, Mq)) for Mq in DESIGN_MS[::-1]]
    for name in LIMIT_CASES:
        tasks += [(_m_design, (name, "uniform", LIMIT_M)), (_m_cond, (name, 1, 0, LIMIT_PICKS, list(range(LIMIT_PICKS + 1)), LIMIT_M)),
                  (_m_margin, (name, 1, LIMIT_PICKS, LIMIT_M))]
    if "--only" in sys.argv:
        keep = tuple(sys.argv[sys.argv.index("--only") + 1].split(","))
        tasks = [t for t in tasks if t[0].__name__[3:] in keep or str(t[1][0]) in keep]
    worst = {}
    with mpc.Pool(min(8, mpc.cpu_count())) as pool:
        for fn, args, out, dt in pool.imap_unordered(_run, tasks):
            print(f"{fn} {args}: " + ", ".join(f"{k} {v:.3e}" if isinstance(v, float) else f"{k} {v}" for k, v in out.items()) + f"  [{dt:.0f} s]", flush=True)
            for k, v in out.items():
                if k in MEASURED and v > worst.get(k, ("", 0.0))[1]:
                    worst[k] = (f"{fn} {args}", v)
    for k, (where, v) in sorted(worst.items()):
        print(f"largest scaled error of numpy against mpmath, {k}: {v:.3e} ({where})")


if __name__ == "__main__":
    if "--measure" in sys.argv:
        measure()
