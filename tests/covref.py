"""What an element written by the covariance fill MEANS, evaluated in numpy.longdouble (64-bit mantissa), the expected image
of a whole staged region, and the bar an element has to meet -- the reference of tests/test_gpu_fill_launch.py for
gpemu_test_fill_launch (include/gpemu.h).

TEST INFRASTRUCTURE, host only: nothing here comes from the device library or the oracle.  Inputs are the fp64 values the
device gets (design, query rows, thetas), converted to longdouble; the constants are the device's literals.

  D_k = x_ak - x_bk;  same point (the nugget rule): every |D_k| < eps with the differences taken in fp64,
                      eps = 1e-10 pow-exp, 1e-16 Matern
  pow-exp:     u2 = 1/2 sum_k D_k^2 e^{-2 t_{k+2}},  c = amp e^{-u2},                               amp = e^{t_0}, nug = e^{t_1}
  Matern 3/2:  s2 = sum_k D_k^2 e^{-2 t_2}, s = sqrt(s2), c = amp (1 + r s) e^{-r s},               r = 1.732050808
  Matern 5/2:  c = amp (1 + r s + (5.0/3.0) s^2) e^{-r s},                                          r = 2.236067978
               amp = t_0, nug = t_1 as they come, or e^{t_0}, e^{t_1} with GPEMU_MODE_MATERN_LOG (matern_log)
  element = c + nug at a same point;  k-vectors: elements below 1E-10 are 0

The bar is the project's own and is not tuned:  |got - ref| <= (1e-13 + 1e-15 |exp argument|) |ref|  (ELEM_RTOL, ARG_RTOL:
tests/gradsumref.py, test_cov_matrix_extreme_hyperparameters), the same for the Gram form and for coordinate differences:
DESIGN.md 4.3 and the kernel comments promise 1e-13 for the stored fill in either form.

Region images (row stride Np = N rounded up to 64, 64 x 64 tiles):
  staged matrix b: rows [0, Np): lower tiles (tr, tc <= tr) hold the elements for i, j < N, 1.0 on the diagonal beyond N, 0.0
                   elsewhere inside them; tiles strictly above the diagonal keep the prefill;
                   rows [Np, Np + Rp): the right-hand-side rows bit for bit; then the guard rows keep the prefill
  k-vectors:       Mp x Np, zero for rows >= M and columns >= N, then guard rows that keep the prefill
  full matrix:     Np x Np, both triangles, zero padding, then guard rows

gram_model_u2 is an fp64 model of the Gram-form squared distance in the order gram_tile_u2 (kernels_cov.hip) takes it:
centred coordinates times the scale (root included), four k-group norms by sequential FMAs and their sum, the products
x'.(-2 y') accumulated sequentially, the final step adding both norms.  It is there to show ON THE CPU that the inputs of
the GPU tests leave room under the bar (tests/test_covref.py); it is no device number.  (An FMA is modelled as one
longdouble multiply-add rounded to fp64: 2^-64 of the product off the single rounding.)
"""
import numpy as np

from madaiemulator_amd import synth

LD = np.longdouble
ROOT = {1: LD(1.0), 2: LD(1.732050808), 3: LD(2.236067978)}     # the doubles nearest to the device's literals
FIVE_THIRDS = LD(5.0 / 3.0)                                      # the fp64 quotient, as the device has it
EPS = {1: 1e-10, 2: 1e-16, 3: 1e-16}
CLAMP = 1E-10
ELEM_RTOL, ARG_RTOL = LD(1e-13), LD(1e-15)
FT = 64
ADMIT = 16.0          # make_cov_params: Gram form while norm2 <= this


def round_up(n, m=FT):
    return (n + m - 1) // m * m


def nthetas_for(kind, d):
    return d + 2 if kind == 1 else 3


def amp_nug(kind, th, matern_log=False):
    if kind == 1 or matern_log:
        return np.exp(LD(th[0])), np.exp(LD(th[1]))
    return LD(th[0]), LD(th[1])


def same_point(kind, Xr, Xc=None):
    """the nugget rule on the fp64 coordinates, as the device applies it (gradsumref.same_point for two point sets)"""
    Xr = np.asarray(Xr, np.float64)
    Xc = Xr if Xc is None else np.asarray(Xc, np.float64)
    same = np.ones((Xr.shape[0], Xc.shape[0]), dtype=bool)
    for k in range(Xr.shape[1]):
        same &= np.abs(Xr[:, k][:, None] - Xc[:, k][None, :]) < EPS[kind]
    return same


def sq_dist(kind, Xr, Xc, th):
    """pow-exp: u2 = 1/2 sum D_k^2 e^{-2 t_k}; Matern: s2 = sum D_k^2 e^{-2 t_2} (longdouble)"""
    Xr = np.asarray(Xr, np.float64).astype(LD)
    Xc = np.asarray(Xc, np.float64).astype(LD)
    out = np.zeros((Xr.shape[0], Xc.shape[0]), dtype=LD)
    for k in range(Xr.shape[1]):
        D = Xr[:, k][:, None] - Xc[:, k][None, :]
        e2 = np.exp(LD(-2.0) * LD(th[2 + k if kind == 1 else 2]))
        out += (LD(0.5) if kind == 1 else LD(1.0)) * e2 * D * D
    return out


def value(kind, a, amp):
    """(the element before the nugget, its exp argument) from sq_dist's a"""
    if kind == 1:
        return amp * np.exp(-a), -a
    s = np.sqrt(a)
    r = ROOT[kind]
    if kind == 2:
        return amp * (LD(1.0) + r * s) * np.exp(-r * s), -r * s
    return amp * (LD(1.0) + r * s + FIVE_THIRDS * s * s) * np.exp(-r * s), -r * s


def elements(kind, Xr, Xc, th, matern_log=False, clamp=False):
    """-> (ref, exp argument), both len(Xr) x len(Xc) longdouble"""
    amp, nug = amp_nug(kind, th, matern_log)
    v, arg = value(kind, sq_dist(kind, Xr, Xc, th), amp)
    v = np.where(same_point(kind, Xr, Xc), v + nug, v)
    if clamp:
        v = np.where(v < LD(CLAMP), LD(0.0), v)
    return v, arg


def bar(ref, arg):
    return (ELEM_RTOL + ARG_RTOL * np.abs(arg)) * np.abs(ref)


def scales(kind, d, th):
    """the coordinate scales w_k in fp64, as make_cov_params computes them"""
    if kind == 1:
        return np.sqrt(0.5) / np.exp(np.asarray(th, np.float64)[2:2 + d])
    return np.full(d, 1.0 / np.exp(float(th[2])))


def norm2(kind, X, th):
    """the admission rule's sum_k (w_k half range_k)^2 in fp64, in make_cov_params' order"""
    X = np.asarray(X, np.float64)
    half = 0.5 * (X.max(axis=0) - X.min(axis=0))
    out = 0.0
    for t in half * scales(kind, X.shape[1], th):
        out += t * t
    return out


# ---------------------------------------------------------------------------- images of whole regions
class Image:
    """want: the expected region (longdouble); elem: where `want` is a covariance element that takes the bar (everywhere
    else the region must hold want's value bit for bit); arg: the exp arguments there (0 elsewhere); written: the cells the
    launch writes (the others keep the prefill)"""

    def __init__(self, prefill):
        self.prefill = np.array(prefill, dtype=np.float64)
        self.want = self.prefill.astype(LD)
        self.elem = np.zeros(self.want.shape, dtype=bool)
        self.written = np.zeros(self.want.shape, dtype=bool)
        self.arg = np.zeros(self.want.shape, dtype=LD)

    def check(self, got):
        """-> (worst error / bar over the elements, number of other cells that differ from the image in their bits)"""
        got = np.asarray(got, np.float64).reshape(self.want.shape)
        e = self.elem
        b = bar(self.want[e], self.arg[e])
        err = np.abs(got[e].astype(LD) - self.want[e])
        zero = b == 0
        ratio = np.where(zero, np.where(err == 0, LD(0.0), LD(np.inf)), err / np.where(zero, LD(1.0), b))
        exact = np.where(self.written, self.want.astype(np.float64), self.prefill)[~e]
        nbad = int(np.count_nonzero(exact.view(np.int64) != np.ascontiguousarray(got[~e]).view(np.int64)))
        nbad += int(np.count_nonzero(~np.isfinite(got[e])))
        return (float(ratio.max()) if ratio.size else 0.0), nbad


def staged_image(kind, X, ths, prefill, rrows, rstride=0, Rp=64, guard=0, matern_log=False, pre=None):
    """prefill: nb x (Np + Rp + guard) x Np; rrows: flat, matrix b's Rp x Np block at b * rstride; pre: elements() of every
    theta, if the caller has them already"""
    X = np.asarray(X, np.float64)
    N, Np = X.shape[0], round_up(X.shape[0])
    ths = np.atleast_2d(ths)
    img = Image(prefill)
    assert img.want.shape == (ths.shape[0], Np + Rp + guard, Np)
    rrows = np.asarray(rrows, np.float64).ravel()
    low = np.zeros((Np, Np), dtype=bool)
    for tr in range(Np // FT):
        low[FT * tr:FT * tr + FT, :FT * tr + FT] = True
    pad = np.where(np.eye(Np, dtype=bool), LD(1.0), LD(0.0))
    for b, th in enumerate(ths):
        v, arg = pre[b] if pre is not None else elements(kind, X, X, th, matern_log)
        full, a = pad.copy(), np.zeros((Np, Np), dtype=LD)
        full[:N, :N], a[:N, :N] = v, arg
        img.want[b, :Np][low] = full[low]
        img.arg[b, :Np][low] = a[low]
        img.elem[b, :N, :N] = low[:N, :N]
        img.want[b, Np:Np + Rp] = rrows[b * rstride:b * rstride + Rp * Np].reshape(Rp, Np)
        img.written[b, :Np] = low
        img.written[b, Np:Np + Rp] = True
    return img


def kvec_image(kind, X, Xq, th, prefill, guard=0, matern_log=False):
    X, Xq = np.asarray(X, np.float64), np.asarray(Xq, np.float64).reshape(-1, np.shape(X)[1])
    N, Np, M, Mp = X.shape[0], round_up(X.shape[0]), Xq.shape[0], round_up(Xq.shape[0])
    img = Image(prefill)
    assert img.want.shape == (Mp + guard, Np)
    v, arg = elements(kind, Xq, X, th, matern_log, clamp=True)
    img.want[:Mp] = 0.0
    img.want[:M, :N], img.arg[:M, :N] = v, arg
    img.written[:Mp] = True
    img.elem[:M, :N] = v != 0          # a clamped element is an exact zero (the inputs keep clear of the clamp: clamp_margin)
    return img


def full_image(kind, X, th, prefill, guard=0, matern_log=False):
    X = np.asarray(X, np.float64)
    N, Np = X.shape[0], round_up(X.shape[0])
    img = Image(prefill)
    assert img.want.shape == (Np + guard, Np)
    v, arg = elements(kind, X, X, th, matern_log)
    img.want[:Np] = 0.0
    img.want[:N, :N], img.arg[:N, :N] = v, arg
    img.elem[:N, :N] = True
    img.written[:Np] = True
    return img


def clamp_margin(kind, X, Xq, th, matern_log=False):
    """smallest relative distance of an unclamped reference k-vector element from the clamp value"""
    v, _ = elements(kind, Xq, X, th, matern_log)
    return float(np.min(np.abs(v - LD(CLAMP))) / LD(CLAMP))


# ---------------------------------------------------------------------------- fp64 model of the Gram-form distance
def _fma(a, b, c):
    return (a.astype(LD) * b.astype(LD) + c.astype(LD)).astype(np.float64)


def gram_model_u2(kind, X, th, Xq=None):
    """the Gram form's squared scaled distance (root included) of every pair in fp64, in gram_tile_u2's order; rows: the
    design, or the query rows Xq centred on the fly"""
    X = np.asarray(X, np.float64)
    d = X.shape[1]
    mid = 0.5 * (X.max(axis=0) + X.min(axis=0))
    wsc = scales(kind, d, th) * float(ROOT[kind])
    B = (X - mid) * wsc                                  # the centred copy is made on the host, the scale applied in the kernel
    A = B if Xq is None else (np.asarray(Xq, np.float64).reshape(-1, d) - mid) * wsc

    def norms(P):
        n = np.zeros((4, P.shape[0]))
        for k in range(d):
            n[k % 4] = _fma(P[:, k], P[:, k], n[k % 4])
        return (n[0] + n[1]) + (n[2] + n[3])

    na, nb = norms(A), norms(B)
    acc = np.zeros((A.shape[0], B.shape[0]))
    for k in range(d):
        acc = _fma(np.broadcast_to(A[:, k][:, None], acc.shape), np.broadcast_to(-2.0 * B[:, k][None, :], acc.shape), acc)
    acc = acc + na[:, None]
    return acc + nb[None, :]


def gram_model_ratio(kind, X, th, matern_log=False, Xq=None):
    """worst |model element - reference| / bar over the pairs the Gram form does not recompute from differences (nugget
    candidates; query rows beyond the far test |x'|^2 > 16 root^2)"""
    c2 = ROOT[kind] * ROOT[kind]
    u2 = gram_model_u2(kind, X, th, Xq)
    ref_a = sq_dist(kind, X if Xq is None else Xq, X, th)
    cand_g = 64.0 * 2.220446049250313e-16 * (2.0 * norm2(kind, X, th) + 1.0) * float(c2)
    keep = u2 > cand_g
    if Xq is not None:
        mid = 0.5 * (np.max(X, axis=0) + np.min(X, axis=0))
        far = (((np.asarray(Xq, np.float64).reshape(-1, np.shape(X)[1]) - mid) * scales(kind, np.shape(X)[1], th)) ** 2).sum(axis=1) > ADMIT
        keep &= ~far[:, None]
    amp, _ = amp_nug(kind, th, matern_log)
    ref, arg = value(kind, ref_a, amp)
    got, _ = value(kind, np.maximum(u2, 0.0).astype(LD) / c2, amp)
    ratio = np.abs(got - ref)[keep] / bar(ref, arg)[keep]
    return float(ratio.max()) if ratio.size else 0.0


# ---------------------------------------------------------------------------- input builders of the GPU tests
def box_design(N, d, seed):
    """uniform in the unit box"""
    return synth.uniform(seed, (N, d))


def corner_design(N, d, seed):
    """every point within 2 % of a corner of the unit box, so every |x'|^2 is close to norm2; the first two rows are
    opposite corners themselves: the box is exactly [0, 1]^d"""
    X = np.where(synth.uniform(seed, (N, d)) < 0.5, 0.0, 1.0)
    X = X + np.where(X > 0.5, -0.02, 0.02) * synth.uniform(seed + 1, (N, d))
    if N > 1:
        X[0], X[1] = 1.0, 0.0
    return X


def thetas_for_norm2(kind, X, target, step=0.05, amp=None, nug=None):
    """length scales e^{t + step k} (Matern: one) with norm2(kind, X, th) = target up to rounding; amp / nug default to
    (0.25, -3.0) pow-exp and (1.5, 0.01) Matern.  A one-point design (norm2 = 0 at any scale) gets scale 0.6."""
    X = np.asarray(X, np.float64)
    d = X.shape[1]
    nl = d if kind == 1 else 1
    th = np.concatenate([[0.25 if kind == 1 else 1.5, -3.0 if kind == 1 else 0.01], step * np.arange(nl)])
    if amp is not None:
        th[0] = amp
    if nug is not None:
        th[1] = nug
    n1 = norm2(kind, X, th)
    th[2:] += 0.5 * np.log(n1 / target) if n1 > 0 else np.log(0.6)
    return th


JUST_UNDER, JUST_OVER = ADMIT * (1 - 1e-3), ADMIT * (1 + 1e-3)

# (N, d): every N of {1, 63, 64, 65, 130, 257, 400} -- 1, 1, 1, 3, 6, 15, 28 lower tiles: 28 is a multiple of the four tiles a
# workgroup of the Gram kernel takes, the others are not, 1 and 3 are less than one workgroup's share -- and every d of
# {1, 3, 4, 5, 16, 64} (the remainders of the 4-wide k loop, GPEMU_MAX_PARAMS), the bigger d with the smaller N; N = 400 twice
SHAPES = [(1, 64), (63, 16), (64, 5), (65, 3), (130, 64), (257, 4), (400, 1), (400, 3)]
BATCH_NORM2 = (2.0, 4.5, 7.0, 11.0, 15.0)          # five different thetas, all admitted


def shape_design(N, d):
    return box_design(N, d, 9000 + 10 * N + d)


def batch_thetas(kind, X):
    return np.array([thetas_for_norm2(kind, X, t, step=0.03 * (i + 1) / X.shape[1], amp=(0.1 * i if kind == 1 else 0.5 + 0.4 * i),
                                      nug=(-3.0 - 0.5 * i if kind == 1 else 0.01 * (i + 1))) for i, t in enumerate(BATCH_NORM2)])


BOUNDARY_SHAPES = [(130, 4), (65, 16), (63, 64)]


def boundary_case(kind, N, d, target):
    X = corner_design(N, d, 9100 + N + d)
    return X, thetas_for_norm2(kind, X, target, step=0.0)


def mixed_thetas(kind, X):
    """alternately admitted and refused"""
    return np.array([thetas_for_norm2(kind, X, t, step=0.02) for t in (6.0, 40.0, JUST_UNDER, JUST_OVER, 1.0)])


# near pairs: (i, j > i): element (j, i) lies in lower tile (j // 64, i // 64).  N = 150: tile row 2 is an edge row.
PAIR_N = 150
PAIR_SPOTS = {
    "one_16_row_group_of_a_diagonal_tile": (3, 9),
    "across_waves_of_a_diagonal_tile": (5, 40),
    "full_off_diagonal_tile": (20, 100),
    "second_diagonal_tile": (70, 120),
    "edge_tile_off_the_diagonal": (30, 140),
    "diagonal_edge_tile": (130, 145),
}
PAIR_OFFSETS = {          # name -> (offset of the first coordinate, offset of the others)
    1: {"duplicate": (0.0, 0.0), "all_5e-11": (5e-11, 5e-11), "all_2e-10": (2e-10, 2e-10), "one_2e-10_rest_5e-11": (2e-10, 5e-11)},
    2: {"duplicate": (0.0, 0.0), "all_5e-17": (5e-17, 5e-17), "all_2e-16": (2e-16, 2e-16)},
}
PAIR_OFFSETS[3] = PAIR_OFFSETS[2]


def pair_design(kind, name, d=3, seed=9200):
    """every spot of PAIR_SPOTS carries a pair `name` apart.  Matern: the first point of a pair is scaled into [0, 1e-3)^d,
    where fp64 resolves an offset of 5e-17 (spacing 2e-19)"""
    X = box_design(PAIR_N, d, seed)
    X[0], X[1] = 1.0, 0.0
    first, rest = PAIR_OFFSETS[kind][name]
    off = np.array([first] + [rest] * (d - 1))
    for i, j in PAIR_SPOTS.values():
        if kind != 1:
            X[i] *= 1e-3
        X[j] = X[i] + off
    return X


LADDER = [10.0 ** -e for e in range(9, 1, -1)]          # 1e-9 .. 1e-2


def ladder_design(d, N=65, seed=9300):
    """row 0: the corner of the box where |x'|^2 is largest; rows 2.. : partners offset INTO the box by each step of the
    ladder along the first coordinate, then along all of them"""
    X = corner_design(N, d, seed + d)
    one = np.zeros(d)
    one[0] = 1.0
    for n, off in enumerate(LADDER):
        X[2 + n] = X[0] - off * one
        X[2 + len(LADDER) + n] = X[0] - off
    return X


def table_design():
    """d = 1, pow-exp, norm2 just under 16: the pair exponents spread over [0, 64) -- every entry of the 1024-entry table"""
    X = box_design(400, 1, 9400)
    X[0], X[1] = 1.0, 0.0
    return X, thetas_for_norm2(1, X, JUST_UNDER)


def table_indices(arg):
    """(table index, octave) the Gram form's exp takes for an exp argument: round(-arg 1024 / ln 2) split at 10 bits"""
    ki = np.rint(np.asarray(-arg, dtype=LD) * LD(1024.0) / np.log(LD(2.0))).astype(np.int64)
    return ki & 1023, ki >> 10


KVEC_SHAPES = [(130, 4), (65, 16)]
KVEC_M = (1, 64, 65, 130)


def kvec_case(kind, N, d, M):
    """design, theta at norm2 just under 16, M query rows: inside the box; equal to design points; on the sphere |x'|^2 =
    16 (1 -+ 1e-3) around the box's centre (just inside / outside the Gram form's far test); one far row (30 in every
    coordinate) in a wave of ordinary rows"""
    X = box_design(N, d, 9500 + N + d)
    X[0], X[1] = 1.0, 0.0
    th = thetas_for_norm2(kind, X, JUST_UNDER, step=0.0)
    Xq = synth.queries(M, d, 9600 + M + d)
    if M > 1:
        w = scales(kind, d, th)
        u = synth.uniform(9700 + d, (2, d)) - 0.5
        u /= np.sqrt(((u * w) ** 2).sum(axis=1))[:, None]           # scaled length 1
        Xq[3] = X[5]
        Xq[4] = X[N - 1]
        Xq[17] = 0.5 + u[0] * np.sqrt(JUST_UNDER)
        Xq[33] = 0.5 + u[1] * np.sqrt(JUST_OVER)
        Xq[50] = 30.0
        Xq[M - 1] = X[0]
    return X, th, Xq


def pair_theta(kind, X):
    return thetas_for_norm2(kind, X, 6.0, step=0.04)


def ladder_theta(kind, X):
    return thetas_for_norm2(kind, X, JUST_UNDER, step=0.0)


def gram_inputs():
    """every (label, kind, design, theta, query rows or None) the GPU tests send through the Gram form"""
    for kind in (1, 2, 3):
        for N, d in SHAPES:
            X = shape_design(N, d)
            for b, th in enumerate(batch_thetas(kind, X)):
                yield f"shape N={N} d={d} theta {b}", kind, X, th, None
        for N, d in BOUNDARY_SHAPES:
            X, th = boundary_case(kind, N, d, JUST_UNDER)
            yield f"boundary N={N} d={d}", kind, X, th, None
            for b, th in enumerate(mixed_thetas(kind, X)):
                if norm2(kind, X, th) <= ADMIT:
                    yield f"mixed N={N} d={d} theta {b}", kind, X, th, None
        for name in PAIR_OFFSETS[kind]:
            X = pair_design(kind, name)
            yield f"pairs {name}", kind, X, pair_theta(kind, X), None
        for d in (4, 16):
            X = ladder_design(d)
            yield f"ladder d={d}", kind, X, ladder_theta(kind, X), None
        for N, d in KVEC_SHAPES:
            for M in KVEC_M:
                X, th, Xq = kvec_case(kind, N, d, M)
                yield f"kvec N={N} d={d} M={M}", kind, X, th, Xq
    X, th = table_design()
    yield "table", 1, X, th, None
