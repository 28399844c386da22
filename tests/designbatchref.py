"""CPU reference for greedy batches of K runs (gpemu_design_batch, include/gpemu.h).  Test infrastructure only; no
device value enters except as an INPUT.

Conditioning the posterior process of senspostref.py on runs at the picks S (each observed with variance c*(x_s, x_s) + nugget)
leaves, for a further run at the candidate q,

  gain_S(q) = num_S(q) / v_S(q),     V = Sigma_SS + nugget I,   sigma_q = Sigma[q, S],   g_q = G[q, S],
  num_S(q)  = G_qq - 2 g_q^T V^-1 sigma_q + sigma_q^T V^-1 G_SS V^-1 sigma_q,        v_S(q) = v_q - sigma_q^T V^-1 sigma_q,

with Sigma(q, s) = c*(x_q, x_s) and G(q, s) = E_x[c*(x, x_q) c*(x, x_s)].  `pieces` assembles Sigma and G for all pairs of
candidates from designref's Gram pieces, G as the RAW GRAM FORM z_q^T Gamma z_s over phi = [A k(., x_q) | A k(., x_i) | h] (the
device expands it into nine parts and sums them another way), in numpy fp64 (R.NP) or mpmath at 50 digits (R.MP()); a, b and
v are inputs (the device's own, or designref.fit_ab's).  `conditional` evaluates the display above NON-INCREMENTALLY, one solve
with V per call; the device carries lambda = L^-1 sigma, mu = L^-1 g and E = L^-1 G_SS L^-T (V = L L^T) forward pick by pick --
`state` returns those three by a Cholesky factor of V for the comparison of the test hook.

SCALES, as in designref (the sum of the absolute values of the parts), extended to the cross terms and the corrections:
  Sigma(q, s): A |k(x_q, x_s)| + |a_q . k_s| + |b_q . h_s|;          G(q, s): the sum of the absolute values of its nine parts;
  num_S(q):    scale G_qq + 2 sum_i |y_i| scale G(q, S_i) + sum_ii' |y_i| |y_i'| scale G(S_i, S_i'),   y = V^-1 sigma_q;
  v_S(q):      |v_q| + sum_i |y_i| scale Sigma(q, S_i);               gain_S(q): scale num_S / v_S.
lambda, mu and E are compared on  (scale Sigma(q, s_j) + sum_i |lambda_qi lambda_si|) / rho_j  and the like (`state`).

`greedy` runs the picks in floats: the arg-max of sum_c weight_c gain_S,c(q) over the candidates not yet picked, ties to the
lowest index; a pick whose v_S is <= 0 conditions nothing (V would be singular).  Beside the picks it returns every pick's
MARGIN, (best - second best) / (the two candidates' gain scales): the GPU tests keep only cases whose margins exceed the bars,
so that the device's picks must equal these.

`forced` takes the picks as an INPUT and returns the conditional values of every candidate and the state given a prefix of them,
through `conditional` and `state`: long batches, whose margins fall under any bar, are checked on the device's own picks
(tests/test_gpu_closed_form_large.py).  `carried` runs the device's recurrences in numpy, optionally with part of the update's dots
left out (tests/test_closed_form_large_ref.py).

Other routes, no closed form: `quadrature_num` (tensor quadrature of the conditioned c*^2, d <= 3) and `refit` (s_all of the
design minus s_all of the design with the first j picks appended, both by senspostref on a numpy fit).

`python tests/designbatchref.py --measure` prints, over exactly the cases of tests/test_gpu_design_batch.py, the largest scaled
error of the numpy backend against mpmath for the pick gains, Sigma and G, the largest refit gap and every case's smallest
margin; the figures it printed are written down in that file."""
import numpy as np

import designref as D
import sensref as R
import senspostref as SP
import sensmeasureref as SM


def _dot(a, b):
    return np.dot(a, b)


# ---------------------------------------------------------------------------------------------------- Sigma and G
def pieces(B, X, model, lo, hi, kind, Xq, a, b, tables=None):
    """-> (Sigma [M, M], G [M, M], scale Sigma, scale G) in the backend's numbers (scales as floats); a [M, N], b [M, nreg]"""
    d = np.shape(X)[1]
    order = (np.shape(b)[1] - 1) // d
    K, HK, Hm = tables if tables is not None else D.design_tables(B, X, model, lo, hi, kind, order)
    Xf, Xqf = np.asarray(X, float), np.asarray(Xq, float)
    X, Xq, lo, hi, s = B.arr(X), B.arr(Xq), B.arr(lo), B.arr(hi), B.arr(model["s"])
    a, b, A = B.arr(a), B.arr(b), B.arr(model["A"])[()]
    w = D._prod(D.pair(B, Xq[:, None, :], X[None, :, :], s, lo, hi, kind))                  # [M, N]
    Pqq = D._prod(D.pair(B, Xq[:, None, :], Xq[None, :, :], s, lo, hi, kind))               # [M, M]
    HKs = D.basis_tables(B, Xq, s, lo, hi, kind, order)                                       # [nreg, M]
    # G: the raw Gram form
    Grr = np.block([[A * A * K, A * HK.T], [A * HK, Hm]])
    G0 = np.concatenate([A * A * w, A * HKs.T], axis=1)
    Z = np.concatenate([-a, b], axis=1)
    ZG0 = _dot(Z, G0.T)                                                                       # [q, s] = z_q . G0_s
    G = A * A * Pqq + ZG0 + ZG0.T + _dot(_dot(Z, Grr), Z.T)
    aK, aHK = _dot(a, K), _dot(a, HK.T)
    parts = [A * A * Pqq, A * A * _dot(w, a.T), A * _dot(HKs.T, b.T), A * A * _dot(a, w.T), A * _dot(b, HKs), A * A * _dot(aK, a.T),
             A * _dot(aHK, b.T), A * _dot(b, aHK.T), _dot(_dot(b, Hm), b.T)]
    gscale = sum(np.abs(B.tofloat(p)) for p in parts)
    # Sigma
    kq = A * _expk(B, Xq, X, s)                                                               # [M, N]
    kqq = A * _expk(B, Xq, Xq, s)
    hq = B.arr(SP.hmatrix(Xqf, order))
    p1, p2 = _dot(a, kq.T), _dot(b, hq.T)
    Sig = kqq - p1 + p2
    sscale = np.abs(B.tofloat(kqq)) + np.abs(B.tofloat(p1)) + np.abs(B.tofloat(p2))
    return Sig, G, sscale, gscale


def _expk(B, Xa, Xb, s):
    D2 = ((Xa[:, None, :] - Xb[None, :, :]) ** 2 * s).sum(axis=2)
    return B.exp(-D2 / 2)


# ---------------------------------------------------------------------------------------------------- generic small solves
def _cholesky(V):
    """lower factor by rows, in whatever numbers V holds"""
    n = len(V)
    L = np.zeros_like(V)
    for i in range(n):
        for j in range(i + 1):
            t = V[i, j] - sum((L[i, k] * L[j, k] for k in range(j)), V[i, j] * 0)
            L[i, j] = t ** 0.5 if i == j else t / L[j, j]
    return L


def _fsolve(L, Bm):
    """L^-1 Bm (Bm: n x m)"""
    Y = np.zeros_like(Bm)
    for i in range(len(L)):
        Y[i] = (Bm[i] - sum((L[i, k] * Y[k] for k in range(i)), Bm[i] * 0)) / L[i, i]
    return Y


def _bsolve(L, Bm):
    """L^-T Bm"""
    n = len(L)
    Y = np.zeros_like(Bm)
    for i in range(n - 1, -1, -1):
        Y[i] = (Bm[i] - sum((L[k, i] * Y[k] for k in range(i + 1, n)), Bm[i] * 0)) / L[i, i]
    return Y


# ---------------------------------------------------------------------------------------------------- conditional gains
def conditional(B, Sig, G, sscale, gscale, v, nugget, S):
    """-> (dict(num [M], var [M], gain [M]), the same keys with the scales) conditional on the picks S (indices, may be empty), floats"""
    M = len(v)
    v = B.arr(v)
    num0, ns = np.array([G[q, q] for q in range(M)]), np.diag(gscale).copy()
    vs = np.abs(B.tofloat(v))
    if len(S) == 0:
        num, var = num0, v
    else:
        S = list(S)
        V = Sig[np.ix_(S, S)] + B.arr(nugget * np.eye(len(S)))
        L = _cholesky(V)
        Y = _bsolve(L, _fsolve(L, Sig[S, :] + v[None, :] * 0))                               # [j, M]: column q = V^-1 sigma_q
        GS = G[np.ix_(S, S)]
        num = num0 - 2 * (G[S, :] * Y).sum(axis=0) + (Y * _dot(GS, Y)).sum(axis=0)
        var = v - (Sig[S, :] * Y).sum(axis=0)
        Ya = np.abs(B.tofloat(Y))
        ns = ns + 2 * (gscale[S, :] * Ya).sum(axis=0) + (Ya * (gscale[np.ix_(S, S)] @ Ya)).sum(axis=0)
        vs = vs + (sscale[S, :] * Ya).sum(axis=0)
    num, var = B.tofloat(num), B.tofloat(var)
    ok = var > 0
    vv = np.where(ok, var, 1.0)
    return (dict(num=num, var=var, gain=np.where(ok, num / vv, 0.0)), dict(num=ns, var=vs, gain=np.where(ok, ns / vv, ns)))


KEYS = ("num", "var", "gain")


def scaled_errors(got, ref, scale, keys=KEYS):
    return R.scaled_errors(got, ref, scale, keys)


def state(Sig, G, sscale, gscale, v, nugget, S):
    """floats -> (lambda [M, j], mu [M, j], E [j, j]) and their scales: V = L L^T, lambda = L^-1 sigma, mu = L^-1 g, E = L^-1 G_SS L^-T;
    scales: entry j of lambda_q on (scale Sigma(q, s_j) + sum_i<j |lambda_qi lambda_sj,i|) / rho_j, mu likewise with scale G and
    |mu_qi lambda_sj,i|, E_ij on (|mu_sj,i| scale + sum_k |E_ik lambda_sj,k|) / rho_j for i < j and scale num_S / v_S on the diagonal"""
    S = list(S)
    j = len(S)
    V = Sig[np.ix_(S, S)] + nugget * np.eye(j)
    L = np.linalg.cholesky(V)
    import scipy.linalg as sl
    lam = sl.solve_triangular(L, Sig[S, :], lower=True).T
    mu = sl.solve_triangular(L, G[S, :], lower=True).T
    E = sl.solve_triangular(L, sl.solve_triangular(L, G[np.ix_(S, S)], lower=True).T, lower=True)
    E = (E + E.T) / 2
    rho = np.diag(L)
    ls, ms, es = np.zeros_like(lam), np.zeros_like(mu), np.zeros_like(E)
    for t, s in enumerate(S):
        ls[:, t] = (sscale[:, s] + np.abs(lam[:, :t]) @ np.abs(lam[s, :t])) / rho[t]
        ms[:, t] = (gscale[:, s] + np.abs(mu[:, :t]) @ np.abs(lam[s, :t])) / rho[t]
    for t, s in enumerate(S):
        for i in range(t):
            es[i, t] = es[t, i] = (ms[s, i] + np.abs(E[i, :t]) @ np.abs(lam[s, :t])) / rho[t]
        es[t, t] = (gscale[s, s] + 2 * np.abs(lam[s, :t]) @ ms[s, :t] + np.abs(lam[s, :t]) @ np.abs(E[:t, :t]) @ np.abs(lam[s, :t])) / rho[t] ** 2
    return (lam, mu, E), (ls, ms, es)


# ---------------------------------------------------------------------------------------------------- the greedy picks
def greedy(ctx_pieces, vs, nugget, nbatch, weight=None, twin=None):
    """ctx_pieces: per context (Sigma, G, scale Sigma, scale G) as float arrays, vs: per context v [M] ->
    dict(pick [nbatch], pick_gain [nbatch], pick_gain_ctx [nbatch, nctx], gain_first [M], gain_last [M], S: per context the picks
    that condition, margin [nbatch]: (best - second best weighted gain) / the sum of the two candidates' weighted gain scales
    (inf when one candidate is left; twin = (i, i'): two identical rows, not each other's second best), pick_scale [nbatch], pick_scale_ctx [nbatch, nctx], last_scale [M])"""
    nctx, M = len(ctx_pieces), len(vs[0])
    w = np.ones(nctx) if weight is None else np.asarray(weight, float)
    S = [[] for _ in range(nctx)]
    taken = np.zeros(M, dtype=bool)
    out = dict(pick=np.zeros(nbatch, dtype=int), pick_gain=np.zeros(nbatch), pick_gain_ctx=np.zeros((nbatch, nctx)), margin=np.zeros(nbatch),
               pick_scale=np.zeros(nbatch), pick_scale_ctx=np.zeros((nbatch, nctx)))

    def gains():
        vals = [conditional(R.NP, *ctx_pieces[c], vs[c], nugget, S[c]) for c in range(nctx)]
        g = np.stack([x[0]["gain"] for x in vals], axis=1)
        var = np.stack([x[0]["var"] for x in vals], axis=1)
        sc = np.stack([x[1]["gain"] for x in vals], axis=1)
        return g, var, g @ w, sc @ w, sc

    for j in range(nbatch):
        g, var, tot, sc, scc = gains()
        if j == 0:
            out["gain_first"] = tot.copy()
        cand = np.where(taken, -np.inf, np.where(np.isnan(tot), -np.inf, tot))
        s = int(np.argmax(cand))                                                             # (the first of equal values)
        rest = cand.copy()
        rest[s] = -np.inf
        if twin is not None and s in twin:                                                   # (an identical row: the tie is exact and goes to the lower index)
            rest[list(twin)] = -np.inf
        if np.isfinite(rest.max()):
            s2 = int(np.argmax(rest))
            out["margin"][j] = (cand[s] - rest[s2]) / (sc[s] + sc[s2])
        else:
            out["margin"][j] = np.inf
        out["pick"][j], out["pick_gain"][j], out["pick_gain_ctx"][j], out["pick_scale"][j] = s, tot[s], g[s], sc[s]
        out["pick_scale_ctx"][j] = scc[s]
        taken[s] = True
        for c in range(nctx):
            if var[s, c] > 0:
                S[c].append(s)
    g, var, tot, sc, scc = gains()
    out["gain_last"] = np.where(taken, -np.inf, tot)
    out["last_scale"] = sc
    out["S"] = S
    return out


def forced(ctx_pieces, vs, nugget, picks, j, weight=None, conditions=None, with_state=True):
    """the picks are an INPUT (the device's own, say): the conditional values of every candidate given the prefix picks[:j], NON-
    INCREMENTALLY (one `conditional` and one `state` per context, nothing carried from a shorter prefix).  conditions: per context
    one flag per pick, whether it conditions (a pick whose v_S was <= 0 does not); None: every pick does, which holds in exact
    arithmetic whenever nugget > 0.  ->
    dict(gain, num, var [M, nctx] and gain_scale, num_scale, var_scale [M, nctx]; tot [M] = gain @ weight and tot_scale [M];
    S: per context the conditioning picks; state: per context ((lambda, mu, E), (their scales)) of S, None where S is empty).
    On greedy's own picks these are greedy's numbers bit for bit (test_designbatchref.py)."""
    nctx = len(ctx_pieces)
    w = np.ones(nctx) if weight is None else np.asarray(weight, float)
    S = [[int(s) for i, s in enumerate(picks[:j]) if conditions is None or conditions[c][i]] for c in range(nctx)]
    vals = [conditional(R.NP, *ctx_pieces[c], vs[c], nugget, S[c]) for c in range(nctx)]
    out = dict(S=S)
    for k in KEYS:
        out[k] = np.stack([x[0][k] for x in vals], axis=1)
        out[k + "_scale"] = np.stack([x[1][k] for x in vals], axis=1)
    out["tot"], out["tot_scale"] = out["gain"] @ w, out["gain_scale"] @ w
    if with_state:
        out["state"] = [state(*ctx_pieces[c], vs[c], nugget, S[c]) if S[c] else None for c in range(nctx)]
    return out


def carried(Sig, G, v, nugget, S, keep=None):
    """lambda, mu, E, v_S, num_S and the gains carried forward pick by pick in the recurrences the device uses, in
    numpy:  rho = sqrt(v_S(s)),  e = (mu_s - E lambda_s) / rho,  E_new,new = num_S(s) / v_S(s),
            lambda_new = (Sigma(., s) - lambda . lambda_s) / rho,   mu_new = (G(., s) - mu . lambda_s) / rho,
            v_S -= lambda_new^2,   num_S += 2 lambda_new (e . lambda - mu_new) + E_new,new lambda_new^2.
    keep = None: the whole recurrence (test_designbatchref.py holds it to `conditional` and `state`).  keep = k: the entries
    i >= k of lambda and mu are LEFT OUT of the three dots of the update (lambda . lambda_s, mu . lambda_s, e . lambda): what an
    update whose lanes make one trip of k entries would carry.  For the leave-out tests only.
    -> (lambda [M, j], mu [M, j], E [j, j], v_S [M], num_S [M], gain [M])"""
    S = list(S)
    M, n = len(v), len(S)
    lam, mu, E = np.zeros((M, n)), np.zeros((M, n)), np.zeros((n, n))
    vS, numS = np.array(v, dtype=float), np.diag(G).copy()
    for t, s in enumerate(S):
        c = t if keep is None else min(t, keep)
        rho = np.sqrt(vS[s])
        ls = lam[s, :t].copy()
        e = (mu[s, :t] - E[:t, :t] @ ls) / rho
        E[:t, t] = E[t, :t] = e
        E[t, t] = numS[s] / vS[s]
        ln = (Sig[:, s] - lam[:, :c] @ ls[:c]) / rho
        mn = (G[:, s] - mu[:, :c] @ ls[:c]) / rho
        el = lam[:, :c] @ e[:c]
        lam[:, t], mu[:, t] = ln, mn
        vS = vS - ln * ln
        numS = numS + 2 * ln * (el - mn) + E[t, t] * ln * ln
    return lam, mu, E, vS, numS, np.where(vS > 0, numS / np.where(vS > 0, vS, 1.0), 0.0)


# ---------------------------------------------------------------------------------------------------- no closed form
def quadrature_num(X, model, order, nugget, lo, hi, kind, Xq, S, n=24):
    """num_S and v_S of every candidate by tensor quadrature of the CONDITIONED c*(x, x_q)^2 over the measure (d <= 3):
    c*_S(x, q) = c*(x, q) - c*(x, S) V^-1 c*(S, q), all from senspostref.cstar on a numpy fit"""
    X, Xq = np.asarray(X, float), np.asarray(Xq, float)
    d = X.shape[1]
    assert d <= 3
    P, G, Q = SP.fit_state(X, np.zeros(len(X)), order, model["A"], model["s"], nugget)[:3]
    nw = SM.nodes_weights(D._kind(kind, d), lo, hi, n)
    mesh = np.stack([g.ravel() for g in np.meshgrid(*[t for t, _ in nw], indexing="ij")], axis=1)
    wt = nw[0][1]
    for _, w in nw[1:]:
        wt = np.multiply.outer(wt, w)
    cs = SP.cstar(X, model, P, G, Q, mesh, Xq)                                               # [mesh, M]
    cqq = SP.cstar(X, model, P, G, Q, Xq, Xq)
    v = np.diag(cqq) + nugget
    if len(S):
        S = list(S)
        Y = np.linalg.solve(cqq[np.ix_(S, S)] + nugget * np.eye(len(S)), cqq[S, :])
        cs = cs - cs[:, S] @ Y
        v = v - (cqq[S, :] * Y).sum(axis=0)
    return wt.ravel() @ (cs * cs), v


def refit(X, model, order, nugget, lo, hi, kind, Xq, picks):
    """-> (s_all(design) - s_all(design + the first j picks) for j = 1 .. len(picks), the sum of the two values' scales)"""
    X, Xq = np.asarray(X, float), np.asarray(Xq, float)
    kind = D._kind(kind, X.shape[1])

    def s_all(Z):
        P, G, Q = SP.fit_state(Z, np.zeros(len(Z)), order, model["A"], model["s"], nugget)[:3]
        val, scale = SM.post(kind, R.NP, Z, model, P, G, Q, np.asarray(lo, float), np.asarray(hi, float))
        return float(val["s_all"]), float(scale["s_all"])

    v0, s0 = s_all(X)
    out = [s_all(np.vstack([X, Xq[list(picks[:j])]])) for j in range(1, len(picks) + 1)]
    return np.array([v0 - v for v, _ in out]), np.array([s0 + s for _, s in out])


if __name__ == "__main__":
    import os
    import sys
    if "--measure" in sys.argv:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        import test_gpu_design_batch
        test_gpu_design_batch.measure()
