// kernels_sens.hip -- main effects and Sobol indices of the posterior mean in closed form (gpemu_sens_cov / gpemu_sens_main,
// include/gpemu.h).  Power-exponential covariance, independent uniform inputs on a box: every conditional
// expectation of  m(x) = beta_0 + sum_l q_l(x_l) + A sum_i gamma_i prod_l k_l(x_il, x_l)  is a product of one-dimensional
// integrals with an erf closed form.  Three launches: the per-point integrals (prep), the N x N sweep of pair terms into
// per-tile partial sums, and the finish that adds the partials in a fixed order and assembles the polynomial parts.
// No atomics, no workgroup waits for another; every sum has one order, so two calls return the same bits.
// Second half: the emulator uncertainty of the same quantities (gpemu_sens_post / gpemu_sens_main_var) -- the
// sweep again, weighted by an element of P = C^-1 - W Q W^T per pair, and the confidence band of the main-effect curves.
// The input measure (gpemu_sens_set_measure) is per coordinate: uniform on [lo, hi] or Gaussian N(lo, hi^2).
// It enters the per-point tables, the pair factor II_l, the moments E x^p and the prior double integral UU_l, nothing else.
#include "gpemu_internal.hpp"
#include "sens_device.hpp"   // erf_diff, sens_pair_factor, sens_lower_tile, sens_moment, sens_eh: shared with kernels_design.hip

#include <cmath>

namespace gpemu {

// fixed-order sum over the 256 threads of a workgroup (red: 256 doubles); every thread returns the sum
__device__ __forceinline__ double block_sum(double v, double *red)
{
	const int tid = threadIdx.x;
	__syncthreads();
	red[tid] = v;
	__syncthreads();
	for (int h = 128; h > 0; h >>= 1) {
		if (tid < h) red[tid] += red[tid + h];
		__syncthreads();
	}
	return red[0];
}

// ---------------------------------------------------------------------------
// prep: per context c (blockIdx.y: 0 = a with the lengths s, 1 = b with t) and design point i the five N x d tables
//   I_l(i), J^1_l(i), J^2_l(i), J^3_l(i)  = (1/w_l) int x^p k_l(x_il, x) dx,  and  Pex_l(i) = prod_{l' != l} I_l'(i)
// (prefix and suffix products, no division), table q of context c at prep + ((c * 5 + q) * d + l) * N + i.
// J^p by  s int x^p k = s x_i int x^{p-1} k + (p-1) int x^{p-2} k - [x^{p-1} k]_lo^hi.
// Workgroup (0, 0) also leaves the sweep's per-coordinate constants (SENS_CST_ROWS rows of GPEMU_MAX_PARAMS) in cst.
// A Gaussian coordinate, x ~ N(mu, sg^2) (mu = lo, sg = hi), with D1 = 1 + s sg^2 and D2 = 1 + (s + t) sg^2:
//   I = D1^-1/2 exp(-(s / D1) (x_i - mu)^2 / 2),   J^1 = I c,  J^2 = I (c^2 + v),  J^3 = I (c^3 + 3 c v),
//   c = (s sg^2 x_i + mu) / D1,  v = sg^2 / D1  -- mean and variance of the product of the kernel and the density --
// and the same seven rows of cst hold the Gaussian pair factor's constants:
//   II = D2^-1/2 exp(-[h (x - x')^2 + fa (x - mu)^2 + fb (x' - mu)^2] / 2),   h = s t sg^2 / D2,  fa = s / D2,  fb = t / D2.
// Everything is written in sg^2, so a very wide and a very narrow measure stay finite.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sens_prep_kernel(const double *X, int N, SensBox bx, double *prep, double *cst)
{
	const int d = bx.d, c = blockIdx.y;
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (blockIdx.x == 0 && c == 0 && threadIdx.x < d) {
		const int l = threadIdx.x;
		if (bx.kind[l] == GPEMU_MEASURE_GAUSS) {
			const double s = bx.s[l], t = bx.t[l], mu = bx.lo[l], sg = bx.hi[l], D2 = 1.0 + (s + t) * (sg * sg);
			cst[0 * GPEMU_MAX_PARAMS + l] = s * t * (sg * sg) / D2;                   // h
			cst[1 * GPEMU_MAX_PARAMS + l] = s / D2;                                   // fa
			cst[2 * GPEMU_MAX_PARAMS + l] = t / D2;                                   // fb
			cst[3 * GPEMU_MAX_PARAMS + l] = 0.0;
			cst[4 * GPEMU_MAX_PARAMS + l] = 1.0 / sqrt(D2);
			cst[5 * GPEMU_MAX_PARAMS + l] = mu;
			cst[6 * GPEMU_MAX_PARAMS + l] = sg;
		} else {
			const double s = bx.s[l], t = bx.t[l], st = s + t, al = sqrt(0.5 * st);
			cst[0 * GPEMU_MAX_PARAMS + l] = s * t / st;                               // h: exp(-h (x - x')^2 / 2)
			cst[1 * GPEMU_MAX_PARAMS + l] = s / st;                                   // c = fa x + fb x'
			cst[2 * GPEMU_MAX_PARAMS + l] = t / st;
			cst[3 * GPEMU_MAX_PARAMS + l] = al;
			cst[4 * GPEMU_MAX_PARAMS + l] = sqrt(M_PI / (2.0 * st)) / (bx.hi[l] - bx.lo[l]);
			cst[5 * GPEMU_MAX_PARAMS + l] = bx.lo[l];
			cst[6 * GPEMU_MAX_PARAMS + l] = bx.hi[l];
		}
		cst[SENS_CST_KIND * GPEMU_MAX_PARAMS + l] = bx.kind[l] == GPEMU_MEASURE_GAUSS ? 1.0 : 0.0;
		cst[SENS_CST_S * GPEMU_MAX_PARAMS + l] = bx.s[l];
	}
	if (i >= N) return;
	double *tab = prep + (long)c * 5 * d * N + i;
	const long q = (long)d * N;                                                   // one table
	for (int l = 0; l < d; l++) {
		if (bx.kind[l] == GPEMU_MEASURE_GAUSS) {
			const double s = c ? bx.t[l] : bx.s[l], mu = bx.lo[l], v2 = bx.hi[l] * bx.hi[l], D1 = 1.0 + s * v2;
			const double x = X[(long)i * d + l], dm = x - mu;
			const double I0 = exp(-0.5 * (s / D1) * dm * dm) / sqrt(D1);
			const double cm = (s * v2 * x + mu) / D1, v = v2 / D1;
			tab[0 * q + (long)l * N] = I0;
			tab[1 * q + (long)l * N] = I0 * cm;
			tab[2 * q + (long)l * N] = I0 * (cm * cm + v);
			tab[3 * q + (long)l * N] = I0 * (cm * (cm * cm + 3.0 * v));
			continue;
		}
		const double s = c ? bx.t[l] : bx.s[l], lo = bx.lo[l], hi = bx.hi[l], w = hi - lo;
		const double x = X[(long)i * d + l], r = sqrt(0.5 * s);
		const double K0 = sqrt(M_PI / (2.0 * s)) * erf_diff(r * (lo - x), r * (hi - x));
		const double khi = exp(-0.5 * s * (hi - x) * (hi - x)), klo = exp(-0.5 * s * (lo - x) * (lo - x));
		const double K1 = x * K0 - (khi - klo) / s;
		const double K2 = x * K1 + (K0 - (hi * khi - lo * klo)) / s;
		const double K3 = x * K2 + (2.0 * K1 - (hi * hi * khi - lo * lo * klo)) / s;
		tab[0 * q + (long)l * N] = K0 / w;
		tab[1 * q + (long)l * N] = K1 / w;
		tab[2 * q + (long)l * N] = K2 / w;
		tab[3 * q + (long)l * N] = K3 / w;
	}
	double run = 1.0;
	for (int l = 0; l < d; l++) {
		tab[4 * q + (long)l * N] = run;
		run *= tab[(long)l * N];
	}
	run = 1.0;
	for (int l = d - 1; l >= 0; l--) {
		tab[4 * q + (long)l * N] *= run;
		run *= tab[(long)l * N];
	}
}

// ---------------------------------------------------------------------------
// sweep: the full N x N square of pairs (i of context a, i' of context b) in 64 x 64 tiles, one workgroup per tile -- no
// symmetric shortcut, the cross case has none.  A thread owns row i = tile row + (tid & 63) and the columns wave + 4 k of
// every 16-column chunk; the chunk's coordinates and its weights gamma'_i' I'_l(i'), gamma'_i' Pex'_l(i') go through LDS
// (every lane of a wave reads the same word).  Per pair and coordinate
//   II_l = exp(-h_l (x - x')^2 / 2) pref_l [erf(al_l (hi_l - c)) - erf(al_l (lo_l - c))],   c = fa_l x + fb_l x'
// and the pair adds to 2 d + 1 sums:  prod_l II_l;  II_j prod_{l != j} I_l I'_l;  (prod_{l != j} II_l) I_j I'_j.
// The leave-one-out products of II come from prefix and suffix products (the factors underflow to 0 for far pairs: never a
// division); those of I I' are the per-point tables Pex.  The row's own factors gamma_i, gamma_i I_j(i), gamma_i Pex_j(i)
// multiply the thread's sums once, at the end.  Then the 64 lanes of a wave are added by a fixed butterfly, the four waves
// in order, and the tile writes its 2 d + 1 partial sums: part[tile * (2 d + 1) + k], k = 0: all, 1 + j: first, 1 + d + j: rest.
// DM: the most coordinates the unrolled form keeps in registers (8, 16); DM = GPEMU_MAX_PARAMS is the same loop rolled,
// with its per-coordinate arrays in private memory (the slower form for d > 16).
// Rows and columns i >= N are computed on zero coordinates with zero weights: finite values times 0.
// WEIGHTED (gpemu_sens_post; one context, s = t): the same pair terms weighted by a matrix element per pair
// in place of gamma_i gamma'_i' -- Pw[i' * ldp + i] = P_ii' for every pair of the lower tiles (sens_pmat_kernel; ldp = N
// rounded up to 64, zero from N on), read by the 64 rows of a wave as one line.  One workgroup per LOWER tile (blockIdx.x,
// sens_lower_tile), whose sums count twice off the diagonal, and one sum more per tile, the rank-one
// sum P_ii' prod_l I_l(i) prod_l I_l(i') at index 2 d + 1.  gamA and gamB are not read.  Everything weighted sits under
// `if constexpr`: the unweighted instantiation is the kernel it was before there was a second one.
// MEAS: 0 every coordinate uniform -- the code above, as it was; 1 every coordinate Gaussian -- the pair
// factor is pref_l exp(-[h_l (x - x')^2 + fa_l (x - mu_l)^2 + fb_l (x' - mu_l)^2] / 2), one exp of three terms <= 0, and the
// instantiation holds no erf or erfc code; 2 both kinds -- a branch per coordinate on its kind, which is the same for every
// lane (the coordinate index is), with the kind row of cst staged beside the seven others.
// ---------------------------------------------------------------------------
constexpr int SENS_CHUNK = 16;

// (the pair factor II_l of one coordinate, sens_pair_factor<MEAS>, and the lower-tile enumeration: sens_device.hpp)

template <int DM, bool WEIGHTED, int MEAS>
__global__ __launch_bounds__(256) void sens_sweep_kernel(const double *X, int N, int d, const double *gamA, const double *gamB,
                                                         const double *prepA, const double *prepB, const double *cst, double *part,
                                                         const double *Pw)
{
	constexpr int UN = DM <= 16 ? DM : 1;
	constexpr int RS = 2 * DM + 1 + (WEIGHTED ? 1 : 0);                           // sums a wave leaves in red
	constexpr int CR = MEAS == 2 ? SENS_CST_KIND + 1 : SENS_CST;                  // rows of cst staged: the mixed form reads the kind
	__shared__ double cst_s[CR * DM];
	__shared__ double xb_s[SENS_CHUNK * DM], wr_s[SENS_CHUNK * DM], wf_s[SENS_CHUNK * DM], gb_s[SENS_CHUNK];
	__shared__ double red[4 * RS];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	int tr = blockIdx.y, tc = blockIdx.x;
	if constexpr (WEIGHTED) sens_lower_tile(blockIdx.x, tr, tc);
	const long q = (long)d * N;
	for (int e = tid; e < CR * d; e += 256) cst_s[(e / d) * DM + e % d] = cst[(e / d) * GPEMU_MAX_PARAMS + e % d];
	const int row = tr * 64 + lane;
	const bool rowv = row < N;
	const int dl = DM <= 16 ? DM : d;                                             // (the unrolled forms run to DM under a guard: no early exit)
	double xr[DM], accF[DM], accR[DM], accA = 0.0;
	[[maybe_unused]] double accN = 0.0;                                           // (weighted) sum_i' P_ii' prod_l I_l(i')
	[[maybe_unused]] const long ldp = (long)((N + 63) / 64) * 64;
#pragma unroll UN
	for (int l = 0; l < dl; l++) {
		xr[l] = (rowv && l < d) ? X[(long)row * d + l] : 0.0;
		accF[l] = 0.0;
		accR[l] = 0.0;
	}
	for (int ch = 0; ch < 64 / SENS_CHUNK; ch++) {
		__syncthreads();
		for (int e = tid; e < SENS_CHUNK * d; e += 256) {
			const int cc = e % SENS_CHUNK, l = e / SENS_CHUNK;
			const int col = tc * 64 + ch * SENS_CHUNK + cc;
			const bool cv = col < N;
			if constexpr (WEIGHTED) {
				// gamma' = 1; gb: prod_l I_l(i'), the column's factor of the rank-one sum
				xb_s[cc * DM + l] = cv ? X[(long)col * d + l] : 0.0;
				wr_s[cc * DM + l] = cv ? prepB[0 * q + (long)l * N + col] : 0.0;
				wf_s[cc * DM + l] = cv ? prepB[4 * q + (long)l * N + col] : 0.0;
				if (l == 0) gb_s[cc] = cv ? prepB[col] * prepB[4 * q + col] : 0.0;
			} else {
				const double g = cv ? gamB[col] : 0.0;
				xb_s[cc * DM + l] = cv ? X[(long)col * d + l] : 0.0;
				wr_s[cc * DM + l] = cv ? g * prepB[0 * q + (long)l * N + col] : 0.0;
				wf_s[cc * DM + l] = cv ? g * prepB[4 * q + (long)l * N + col] : 0.0;
				if (l == 0) gb_s[cc] = g;
			}
		}
		__syncthreads();
		for (int k = 0; k < SENS_CHUNK / 4; k++) {
			const int cc = wave + 4 * k;
			const double *xc = xb_s + cc * DM, *wr = wr_s + cc * DM, *wf = wf_s + cc * DM;
			double a[DM], pre[DM], run = 1.0;
			[[maybe_unused]] double pw = 1.0;
			if constexpr (WEIGHTED) {
				// the pair's weight starts the running product: it reaches the all-sum and every leave-one-out product of II
				pw = Pw[(long)(tc * 64 + ch * SENS_CHUNK + cc) * ldp + row];
				run = pw;
				accN = fma(pw, gb_s[cc], accN);
			}
#pragma unroll UN
			for (int l = 0; l < dl; l++) {
				if (l >= d) continue;
				double v;
				if constexpr (MEAS == 0) {
					const double dx = xr[l] - xc[l];
					const double c = cst_s[1 * DM + l] * xr[l] + cst_s[2 * DM + l] * xc[l], al = cst_s[3 * DM + l];
					v = exp(-0.5 * cst_s[0 * DM + l] * dx * dx) * cst_s[4 * DM + l] *
					    erf_diff(al * (cst_s[5 * DM + l] - c), al * (cst_s[6 * DM + l] - c));
				} else {
					v = sens_pair_factor<MEAS>(xr[l], xc[l], cst_s[0 * DM + l], cst_s[1 * DM + l], cst_s[2 * DM + l], cst_s[3 * DM + l],
					                           cst_s[4 * DM + l], cst_s[5 * DM + l], cst_s[6 * DM + l],
					                           MEAS == 2 ? cst_s[(CR - 1) * DM + l] : 0.0);
				}
				a[l] = v;
				pre[l] = run;
				run *= v;
				if constexpr (WEIGHTED) accF[l] = fma(wf[l] * pw, v, accF[l]);
				else accF[l] = fma(wf[l], v, accF[l]);
			}
			if constexpr (WEIGHTED) accA += run;
			else accA = fma(gb_s[cc], run, accA);
			double suf = 1.0;
#pragma unroll UN
			for (int l = dl - 1; l >= 0; l--) {
				if (l >= d) continue;
				accR[l] = fma(wr[l], pre[l] * suf, accR[l]);
				suf *= a[l];
			}
		}
	}
	// the row's own factors, the 64 rows of the wave by a butterfly, the four waves in order
	double gr;
	if constexpr (WEIGHTED) gr = rowv ? 1.0 : 0.0;
	else gr = rowv ? gamA[row] : 0.0;
	const int np = 2 * d + 1 + (WEIGHTED ? 1 : 0);
	{
		double t = gr * accA;
		for (int m = 1; m < 64; m <<= 1) t += __shfl_xor(t, m);
		if (lane == 0) red[wave * RS] = t;
	}
	if constexpr (WEIGHTED) {
		double t = rowv ? prepA[row] * prepA[4 * q + row] * accN : 0.0;
		for (int m = 1; m < 64; m <<= 1) t += __shfl_xor(t, m);
		if (lane == 0) red[wave * RS + 2 * DM + 1] = t;
	}
#pragma unroll UN
	for (int l = 0; l < dl; l++) {
		if (l >= d) continue;
		double f = rowv ? gr * prepA[4 * q + (long)l * N + row] * accF[l] : 0.0;
		double r = rowv ? gr * prepA[0 * q + (long)l * N + row] * accR[l] : 0.0;
		for (int m = 1; m < 64; m <<= 1) {
			f += __shfl_xor(f, m);
			r += __shfl_xor(r, m);
		}
		if (lane == 0) {
			red[wave * RS + 1 + l] = f;
			red[wave * RS + 1 + DM + l] = r;
		}
	}
	__syncthreads();
	if (tid < np) {
		int k = tid == 0 ? 0 : (tid <= d ? tid : 1 + DM + (tid - 1 - d));
		if constexpr (WEIGHTED) if (tid == 2 * d + 1) k = 2 * DM + 1;
		const double t = ((red[k] + red[RS + k]) + red[2 * RS + k]) + red[3 * RS + k];
		// (weighted) an off-diagonal tile stands for its mirror image too: P and the pair terms are symmetric
		if constexpr (WEIGHTED) part[(long)blockIdx.x * np + tid] = tr > tc ? 2.0 * t : t;
		else part[((long)tr * gridDim.x + tc) * np + tid] = t;
	}
}

// ---------------------------------------------------------------------------
// finish: workgroup k of 2 d + 1 assembles output k (0: cov_all, 1 + j: cov_first[j], 1 + d + j: cov_rest[j]) into
// out[2 + k]; workgroup 0 also writes E0 of a and of b to out[0], out[1].  With q~_l = q_l - E q_l and F = E f (f the
// kernel part), m_u - E0 = sum_{l in u} q~_l + (f_u - F) -- E0 has left the constant term before any second moment is
// formed, so a small index is not the difference of two large numbers of the polynomial's size -- and
//   cov_u = sum_{l in u} D_l + A A' KK_u - F^a F^b,
//   D_l = Cov(q^a_l, q^b_l) + (E[q^a_l f^b] - E q^a_l F^b) + (E[q^b_l f^a] - E q^b_l F^a),
//   E[q^a_l f^b] = A' sum_i gamma'_i (sum_p beta^a_{p,l} J^{p,b}_l(i)) Pex^b_l(i),   E x^p = (hi^{p+1} - lo^{p+1}) / ((p+1) w).
// KK_u: the tiles' partial sums in tile order (thread-strided, then the workgroup's tree).  Every workgroup computes the
// D_l it needs itself, by the same instructions in the same order as any other.
// ---------------------------------------------------------------------------
struct SensSide {
	const double *gam, *beta, *prep;   // gamma (N), beta (nreg), the five tables of this context
	double A;
};

// (E x_l^p under the measure of coordinate l, sens_moment, and E h_a, sens_eh: sens_device.hpp)

// the squared inverse length s_l of a one-context call: a uniform coordinate keeps 2 (s t / (s + t)) of row 0 (s = t: s / 2),
// a Gaussian one, whose row 0 holds something else, takes the row of its own
__device__ __forceinline__ double sens_len(const double *cst, int l)
{
	return cst[SENS_CST_KIND * GPEMU_MAX_PARAMS + l] != 0.0 ? cst[SENS_CST_S * GPEMU_MAX_PARAMS + l] : 2.0 * cst[l];
}

// E q_l of the side whose polynomial coefficients are beta
__device__ __forceinline__ double sens_eq(const double *beta, int order, int d, int l, const double *cst)
{
	double v = 0.0;
	for (int p = 1; p <= order; p++) v = fma(beta[1 + (p - 1) * d + l], sens_moment(cst, l, p), v);
	return v;
}

// F = A sum_i gamma_i prod_l I_l(i)
__device__ double sens_kernel_mean(const SensSide &s, int N, int d, double *red)
{
	const long q = (long)d * N;
	double v = 0.0;
	for (int i = threadIdx.x; i < N; i += 256) v = fma(s.gam[i], s.prep[i] * s.prep[4 * q + i], v);
	return s.A * block_sum(v, red);
}

// E[q^p_l f^k]: the polynomial of side p against the kernel part of side k
__device__ double sens_poly_kernel(const SensSide &p, const SensSide &k, int order, int N, int d, int l, double *red)
{
	const long q = (long)d * N;
	double v = 0.0;
	for (int i = threadIdx.x; i < N; i += 256) {
		double g = 0.0;
		for (int o = 1; o <= order; o++) g = fma(p.beta[1 + (o - 1) * d + l], k.prep[o * q + (long)l * N + i], g);
		v = fma(k.gam[i] * g, k.prep[4 * q + (long)l * N + i], v);
	}
	return k.A * block_sum(v, red);
}

__global__ __launch_bounds__(256) void sens_finish_kernel(const double *part, int ntiles, SensSide a, SensSide b, int N, int d, int order,
                                                          const double *cst, double *out)
{
	__shared__ double red[256];
	const int k = blockIdx.x, np = 2 * d + 1;
	double kk = 0.0;
	for (int t = threadIdx.x; t < ntiles; t += 256) kk += part[(long)t * np + k];
	kk = block_sum(kk, red);
	const double Fa = sens_kernel_mean(a, N, d, red), Fb = sens_kernel_mean(b, N, d, red);
	double sumD = 0.0, Sa = a.beta[0], Sb = b.beta[0];
	for (int l = 0; l < d; l++) {
		const double Eqa = sens_eq(a.beta, order, d, l, cst), Eqb = sens_eq(b.beta, order, d, l, cst);
		Sa += Eqa;
		Sb += Eqb;
		const bool inu = k == 0 || (k <= d ? l == k - 1 : l != k - 1 - d);
		if (!inu || order == 0) continue;
		double cq = 0.0;                                                          // Cov(q^a_l, q^b_l)
		for (int p = 1; p <= order; p++)
			for (int r = 1; r <= order; r++)
				cq = fma(a.beta[1 + (p - 1) * d + l] * b.beta[1 + (r - 1) * d + l],
				         sens_moment(cst, l, p + r) - sens_moment(cst, l, p) * sens_moment(cst, l, r), cq);
		const double Hab = sens_poly_kernel(a, b, order, N, d, l, red), Hba = sens_poly_kernel(b, a, order, N, d, l, red);
		sumD += cq + (Hab - Eqa * Fb) + (Hba - Eqb * Fa);
	}
	if (threadIdx.x == 0) {
		out[2 + k] = sumD + (a.A * b.A * kk - Fa * Fb);
		if (k == 0) { out[0] = Sa + Fa; out[1] = Sb + Fb; }
	}
}

// ---------------------------------------------------------------------------
// main effects: workgroup (g, j) -> E[m | x_j = grid[j][g]] = beta_0 + q_j(g) + sum_{l != j} E q_l + A sum_i gamma_i
// k_j(x_ij, g) Pex_j(i); workgroup (0, 0) also writes E0 to e0.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sens_main_kernel(const double *X, SensSide a, int N, int d, int order, const double *cst,
                                                        const double *grid, int ngrid, double *e0, double *out)
{
	__shared__ double red[256];
	const int g = blockIdx.x, j = blockIdx.y;
	const double sj = sens_len(cst, j);
	const double x = grid[(long)j * ngrid + g];
	const long q = (long)d * N;
	double v = 0.0;
	for (int i = threadIdx.x; i < N; i += 256) {
		const double dx = x - X[(long)i * d + j];
		v = fma(a.gam[i] * a.prep[4 * q + (long)j * N + i], exp(-0.5 * sj * dx * dx), v);
	}
	const double kern = a.A * block_sum(v, red);
	double S = a.beta[0], rest = a.beta[0];
	for (int l = 0; l < d; l++) {
		const double Eq = sens_eq(a.beta, order, d, l, cst);
		S += Eq;
		if (l != j) rest += Eq;
	}
	double qj = 0.0, xp = 1.0;
	for (int p = 1; p <= order; p++) {
		xp *= x;
		qj = fma(a.beta[1 + (p - 1) * d + j], xp, qj);
	}
	if (threadIdx.x == 0) out[(long)j * ngrid + g] = rest + qj + kern;
	if (g == 0 && j == 0) {
		const double F = sens_kernel_mean(a, N, d, red);
		if (threadIdx.x == 0) *e0 = S + F;
	}
}

// ===========================================================================
// Emulator uncertainty of the same quantities (gpemu_sens_post / gpemu_sens_main_var): the posterior
// covariance  c*(x, x') = c - k^T P k' + h^T Q h' - h^T G^T k' - k^T G h',  P = C^-1 - W Q W^T, G = W Q, integrated over the
// box with the coordinates of a set u shared between x and x':
//   S_u = CC_u - A^2 sum_ii' P_ii' KK_u(i, i') + sum_ab Q_ab Hm_u(a, b) - 2 sum_a sum_i G_ia HK_u(a, i).
// ===========================================================================
// UU = (1 / w^2) int int k_l dx dx' over the box, a = w sqrt(s / 2):  (2 / w^2) [w sqrt(pi / 2 s) erf(a) - (1 - e^{-a^2}) / s]
__device__ __forceinline__ double sens_uu(double s, double w)
{
	const double a = w * sqrt(0.5 * s);
	return 2.0 / (w * w) * (w * sqrt(M_PI / (2.0 * s)) * erf(a) + expm1(-a * a) / s);
}

// UU_l under the measure of coordinate l (one context): the box's above, or (1 + 2 s sg^2)^-1/2 for a Gaussian coordinate
__device__ __forceinline__ double sens_uu(const double *cst, int l)
{
	const double lo = cst[5 * GPEMU_MAX_PARAMS + l], hi = cst[6 * GPEMU_MAX_PARAMS + l];
	if (cst[SENS_CST_KIND * GPEMU_MAX_PARAMS + l] != 0.0) return 1.0 / sqrt(1.0 + 2.0 * cst[SENS_CST_S * GPEMU_MAX_PARAMS + l] * (hi * hi));
	return sens_uu(2.0 * cst[l], hi - lo);                                        // (s = t: row 0 of cst holds s / 2)
}

// ---------------------------------------------------------------------------
// pmat: one workgroup per lower 64 x 64 tile (tr, tc).  S: the corner C^-1 = U U^T of gpemu_get_cinverse, lower triangle at
// (Rp, Rp), W = C^-1 H in its columns 1 .. nreg (read, never written).  The workgroup forms G = W Q for its 64 rows in LDS
// (column tiles tc = 0 also store them: G, N x nreg) and writes
//   Pw[i' * ldp + i] = (C^-1)_{hi,lo} - sum_a G_{hi,a} W_{lo,a},   hi = max(i, i'), lo = min(i, i')
// for every pair of the tile -- a diagonal tile in full, both halves from the one expression, so the sweep needs no max / min.
// Pairs with hi >= N are 0.  Dynamic LDS: two blocks of 64 x (nreg | 1) doubles.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sens_pmat_kernel(const double *S, long lds, int Rp, const double *Q, int N, int nreg, double *G,
                                                        double *Pw, long ldp)
{
	extern __shared__ double pm_s[];
	const int ls = nreg | 1;
	double *Ws = pm_s, *Gs = pm_s + 64 * ls;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	int tr, tc;
	sens_lower_tile(blockIdx.x, tr, tc);
	for (int e = tid; e < 64 * nreg; e += 256) {
		const int r = e / nreg, a = e % nreg, row = tr * 64 + r;
		Ws[r * ls + a] = row < N ? S[(long)(Rp + row) * lds + 1 + a] : 0.0;
	}
	__syncthreads();
	for (int e = tid; e < 64 * nreg; e += 256) {
		const int r = e / nreg, a = e % nreg, row = tr * 64 + r;
		double g = 0.0;
		for (int b = 0; b < nreg; b++) g = fma(Ws[r * ls + b], Q[b * nreg + a], g);
		Gs[r * ls + a] = g;
		if (tc == 0 && row < N) G[(long)row * nreg + a] = g;
	}
	__syncthreads();
	if (tc != tr)
		for (int e = tid; e < 64 * nreg; e += 256) {
			const int r = e / nreg, a = e % nreg, row = tc * 64 + r;
			Ws[r * ls + a] = row < N ? S[(long)(Rp + row) * lds + 1 + a] : 0.0;
		}
	__syncthreads();
	for (int k = 0; k < 16; k++) {
		const int c = wave + 4 * k;
		const bool flip = tr == tc && lane < c;
		const int hl = flip ? c : lane, ll = flip ? lane : c;
		const int ghi = tr * 64 + hl, glo = tc * 64 + ll;
		double v = 0.0;
		if (ghi < N) {
			double acc = 0.0;
			for (int a = 0; a < nreg; a++) acc = fma(Gs[hl * ls + a], Ws[ll * ls + a], acc);
			v = S[(long)(Rp + ghi) * lds + Rp + glo] - acc;
		}
		Pw[(long)(tc * 64 + c) * ldp + tr * 64 + lane] = v;
	}
}

// ---------------------------------------------------------------------------
// post finish: workgroup k of 2 d + 2 assembles S_u for u = all (k = 0), {j} (1 + j), all but j (1 + d + j), none (2 d + 1)
// into out: s_none, s_all, first[d], rest[d].  The weighted sweep's partial sums in tile order, then
//   CC_u = A prod_{l not in u} UU_l,
//   Hm_u(a, b) = E h_a E h_b, but E x_l^{p+q} for a = (p, l), b = (q, l) in one coordinate l of u,
//   HK_u(a, i) = A J^p_l(i) Pex_l(i) for a = (p, l) with l in u, else E h_a A prod_l I_l(i).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sens_post_finish_kernel(const double *part, int ntiles, const double *prep, const double *G,
                                                               const double *Q, double A, int N, int d, int order, int nreg,
                                                               const double *cst, double *out)
{
	__shared__ double red[256], eh[GPEMU_MAX_PARAMS];
	const int k = blockIdx.x, np = 2 * d + 2, tid = threadIdx.x;
	const long q = (long)d * N;
	(void)order;
	auto inu = [&](int l) { return k == 0 || (k <= d ? l == k - 1 : (k <= 2 * d ? l != k - 1 - d : false)); };
	if (tid < nreg) eh[tid] = sens_eh(tid, d, cst);
	double kk = 0.0;
	for (int t = tid; t < ntiles; t += 256) kk += part[(long)t * np + k];
	kk = block_sum(kk, red);                                                      // (its barriers publish eh)
	double cc = A;
	for (int l = 0; l < d; l++)
		if (!inu(l)) cc *= sens_uu(cst, l);
	double hq = 0.0;
	for (int e = tid; e < nreg * nreg; e += 256) {
		const int a = e / nreg, b = e % nreg;
		double hm = eh[a] * eh[b];
		if (a > 0 && b > 0 && (a - 1) % d == (b - 1) % d && inu((a - 1) % d)) {
			const int l = (a - 1) % d;
			hm = sens_moment(cst, l, (a - 1) / d + (b - 1) / d + 2);
		}
		hq = fma(Q[e], hm, hq);
	}
	hq = block_sum(hq, red);
	double hk = 0.0;
	for (int i = tid; i < N; i += 256) {
		const double pi = prep[i] * prep[4 * q + i];
		double g = 0.0;
		for (int a = 0; a < nreg; a++) {
			const int l = a ? (a - 1) % d : 0, p = a ? (a - 1) / d + 1 : 0;
			const double t = (a && inu(l)) ? prep[p * q + (long)l * N + i] * prep[4 * q + (long)l * N + i] : eh[a] * pi;
			g = fma(G[(long)i * nreg + a], t, g);
		}
		hk += g;
	}
	hk = block_sum(hk, red);
	if (tid == 0) out[k == 2 * d + 1 ? 0 : 1 + k] = ((cc - A * A * kk) + hq) - 2.0 * A * hk;
}

// ---------------------------------------------------------------------------
// tvec: rows r0 .. r0 + mb of the M = d ngrid + 1 "k-vectors" of the band, into the prediction's k-vector buffer (mbp rows
// of Np, mbp = mb rounded up to 64): row j ngrid + g holds T_i = A k_j(x_ij, grid[j][g]) Pex_j(i), the last row A prod_l I_l(i);
// columns i >= N and rows beyond mb are 0.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sens_tvec_kernel(const double *X, const double *prep, const double *cst, double A, int N, int Np,
                                                        int d, const double *grid, int ngrid, int r0, int mb, double *Kq)
{
	const int col = blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
	if (col >= Np) return;
	const long q = (long)d * N;
	const int gr = r0 + row;
	double v = 0.0;
	if (row < mb && col < N) {
		if (gr == d * ngrid) v = A * (prep[col] * prep[4 * q + col]);
		else {
			const int j = gr / ngrid;
			const double dx = grid[gr] - X[(long)col * d + j];
			const double hs = cst[SENS_CST_KIND * GPEMU_MAX_PARAMS + j] != 0.0 ? 0.5 * cst[SENS_CST_S * GPEMU_MAX_PARAMS + j] : cst[j];
			v = A * (exp(-hs * dx * dx) * prep[4 * q + (long)j * N + col]);       // (row 0 of cst: s / 2 on a uniform coordinate)
		}
	}
	Kq[(long)row * Np + col] = v;
}

// ---------------------------------------------------------------------------
// band finish, one wave per row of  V = [L^-1 T (Np) | T . gamma | T^T W (nreg)]  as predict_finish_kernel:
//   main = hm . beta + T . gamma,   var = A prod_{l != j} UU_l - |L^-1 T|^2 + r^T Q r,   r = hm - W^T T,
// hm_a = E[h_a | x_j = x]: 1, x^p for a = (p, j), E x_l^p otherwise; the last row (no coordinate fixed) gives E0 and Var*[E0].
// Lane a holds r_a; the sums over the lanes are fixed butterflies.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sens_band_finish_kernel(const double *V, long ldv, int mb, int r0, int Np, int nreg, int d,
                                                               int ngrid, const double *cst, const double *grid, const double *betaQ,
                                                               double A, double *main, double *var)
{
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int row = min(blockIdx.x * 4 + wave, mb - 1);                           // (a spare wave repeats the last row and stores nothing)
	const bool store = blockIdx.x * 4 + wave < mb && lane == 0;
	const double *v = V + (long)row * ldv;
	double ss = 0.0;
	for (int i = lane * 2; i < Np; i += 128) {
		const double2 t = *reinterpret_cast<const double2 *>(v + i);
		ss += t.x * t.x;
		ss += t.y * t.y;
	}
	const int gr = r0 + row, j = gr == d * ngrid ? -1 : gr / ngrid;
	const double x = j >= 0 ? grid[gr] : 0.0;
	double hm = 0.0, ra = 0.0;
	if (lane < nreg) {
		hm = sens_eh(lane, d, cst);
		if (lane > 0 && (lane - 1) % d == j) {
			hm = x;
			for (int p = 1; p < (lane - 1) / d + 1; p++) hm *= x;
		}
		ra = hm - v[Np + 1 + lane];
	}
	double t = 0.0;
	for (int b = 0; b < nreg; b++) {
		const double rb = __shfl(ra, b);
		if (lane < nreg) t = fma(betaQ[nreg + lane * nreg + b], rb, t);
	}
	double reg = ra * t, mean = lane < nreg ? hm * betaQ[lane] : 0.0;
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) {
		ss += __shfl_xor(ss, off);
		reg += __shfl_xor(reg, off);
		mean += __shfl_xor(mean, off);
	}
	if (store) {
		double cc = A;
		for (int l = 0; l < d; l++)
			if (l != j) cc *= sens_uu(cst, l);
		if (main) main[gr] = mean + v[Np];
		var[gr] = (cc - ss) + reg;
	}
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
size_t sens_prep_elems(int N, int d) { return (size_t)2 * 5 * d * N; }
size_t sens_part_elems(int N, int d) { const size_t nt = (size_t)((N + 63) / 64); return nt * nt * (size_t)(2 * d + 1); }
size_t sens_post_part_elems(int N, int d) { const size_t nt = (size_t)((N + 63) / 64); return nt * (nt + 1) / 2 * (size_t)(2 * d + 2); }

hipError_t launch_sens_prep(hipStream_t s, const double *X, int N, const SensBox &bx, double *prep, double *cst)
{
	if (N < 1 || bx.d < 1 || bx.d > GPEMU_MAX_PARAMS) return hipErrorInvalidValue;
	hipLaunchKernelGGL(sens_prep_kernel, dim3((N + 255) / 256, 2), dim3(256), 0, s, X, N, bx, prep, cst);
	return hipGetLastError();
}

// the sweep's instantiation for d (8, 16 or the rolled form) and the call's measure (SensBox::meas)
template <bool WEIGHTED, int MEAS>
static void sens_sweep_launch(hipStream_t s, dim3 grid, const double *X, int N, int d, const double *gamA, const double *gamB, const double *pa,
                              const double *pb, const double *cst, double *part, const double *Pw)
{
	if (d <= 8)
		hipLaunchKernelGGL((sens_sweep_kernel<8, WEIGHTED, MEAS>), grid, dim3(256), 0, s, X, N, d, gamA, gamB, pa, pb, cst, part, Pw);
	else if (d <= 16)
		hipLaunchKernelGGL((sens_sweep_kernel<16, WEIGHTED, MEAS>), grid, dim3(256), 0, s, X, N, d, gamA, gamB, pa, pb, cst, part, Pw);
	else
		hipLaunchKernelGGL((sens_sweep_kernel<GPEMU_MAX_PARAMS, WEIGHTED, MEAS>), grid, dim3(256), 0, s, X, N, d, gamA, gamB, pa, pb, cst, part, Pw);
}

hipError_t launch_sens_sweep(hipStream_t s, const double *X, int N, int d, const double *gamA, const double *gamB, const double *prep,
                             const double *cst, int meas, double *part)
{
	if (N < 1 || d < 1 || d > GPEMU_MAX_PARAMS || meas < 0 || meas > 2) return hipErrorInvalidValue;
	const int nt = (N + 63) / 64;
	const dim3 grid(nt, nt);
	const double *pa = prep, *pb = prep + (size_t)5 * d * N;
	const double *none = nullptr;
	if (meas == 0) sens_sweep_launch<false, 0>(s, grid, X, N, d, gamA, gamB, pa, pb, cst, part, none);
	else if (meas == 1) sens_sweep_launch<false, 1>(s, grid, X, N, d, gamA, gamB, pa, pb, cst, part, none);
	else sens_sweep_launch<false, 2>(s, grid, X, N, d, gamA, gamB, pa, pb, cst, part, none);
	return hipGetLastError();
}

hipError_t launch_sens_sweep_weighted(hipStream_t s, const double *X, int N, int d, const double *prep, const double *cst, int meas,
                                      const double *Pw, double *part)
{
	if (N < 1 || d < 1 || d > GPEMU_MAX_PARAMS || meas < 0 || meas > 2) return hipErrorInvalidValue;
	const int nt = (N + 63) / 64;
	const dim3 grid(nt * (nt + 1) / 2);
	const double *none = nullptr;
	if (meas == 0) sens_sweep_launch<true, 0>(s, grid, X, N, d, none, none, prep, prep, cst, part, Pw);
	else if (meas == 1) sens_sweep_launch<true, 1>(s, grid, X, N, d, none, none, prep, prep, cst, part, Pw);
	else sens_sweep_launch<true, 2>(s, grid, X, N, d, none, none, prep, prep, cst, part, Pw);
	return hipGetLastError();
}

hipError_t launch_sens_pmat(hipStream_t s, const double *S, long lds, int Rp, const double *Q, int N, int nreg, double *G, double *Pw)
{
	if (N < 1 || nreg < 1 || nreg >= Rp) return hipErrorInvalidValue;
	const int nt = (N + 63) / 64;
	const size_t lds_bytes = (size_t)2 * 64 * (nreg | 1) * sizeof(double);        // at most 2 x 64 x 63 doubles: under 64 KiB
	hipLaunchKernelGGL(sens_pmat_kernel, dim3(nt * (nt + 1) / 2), dim3(256), lds_bytes, s, S, lds, Rp, Q, N, nreg, G, Pw, (long)nt * 64);
	return hipGetLastError();
}

hipError_t launch_sens_post_finish(hipStream_t s, const double *part, int N, int d, int order, int nreg, double amp, const double *prep,
                                   const double *cst, const double *G, const double *Q, double *out)
{
	const int nt = (N + 63) / 64;
	hipLaunchKernelGGL(sens_post_finish_kernel, dim3(2 * d + 2), dim3(256), 0, s, part, nt * (nt + 1) / 2, prep, G, Q, amp, N, d, order, nreg,
	                   cst, out);
	return hipGetLastError();
}

hipError_t launch_sens_tvec(hipStream_t s, const double *X, int N, int Np, int d, double amp, const double *prep, const double *cst,
                            const double *grid, int ngrid, int r0, int mb, int mbp, double *Kq)
{
	if (mb < 1 || mbp < mb || mbp > 65535 || N < 1 || d < 1 || d > GPEMU_MAX_PARAMS) return hipErrorInvalidValue;
	hipLaunchKernelGGL(sens_tvec_kernel, dim3((Np + 255) / 256, mbp), dim3(256), 0, s, X, prep, cst, amp, N, Np, d, grid, ngrid, r0, mb, Kq);
	return hipGetLastError();
}

hipError_t launch_sens_band_finish(hipStream_t s, const double *V, long ldv, int mb, int r0, int Np, int nreg, int d, int ngrid,
                                   const double *cst, const double *grid, const double *betaQ, double amp, double *main, double *var)
{
	hipLaunchKernelGGL(sens_band_finish_kernel, dim3((mb + 3) / 4), dim3(256), 0, s, V, ldv, mb, r0, Np, nreg, d, ngrid, cst, grid, betaQ, amp,
	                   main, var);
	return hipGetLastError();
}

hipError_t launch_sens_finish(hipStream_t s, const double *part, int N, int d, int order, const double *gamA, const double *betaA,
                              double ampA, const double *gamB, const double *betaB, double ampB, const double *prep, const double *cst,
                              double *out)
{
	const int nt = (N + 63) / 64;
	const SensSide a{gamA, betaA, prep, ampA}, b{gamB, betaB, prep + (size_t)5 * d * N, ampB};
	hipLaunchKernelGGL(sens_finish_kernel, dim3(2 * d + 1), dim3(256), 0, s, part, nt * nt, a, b, N, d, order, cst, out);
	return hipGetLastError();
}

hipError_t launch_sens_main(hipStream_t s, const double *X, int N, int d, int order, const double *gam, const double *beta, double amp,
                            const double *prep, const double *cst, const double *grid, int ngrid, double *e0, double *out)
{
	if (ngrid < 1 || N < 1 || d < 1 || d > GPEMU_MAX_PARAMS) return hipErrorInvalidValue;
	const SensSide a{gam, beta, prep, amp};
	hipLaunchKernelGGL(sens_main_kernel, dim3(ngrid, d), dim3(256), 0, s, X, a, N, d, order, cst, grid, ngrid, e0, out);
	return hipGetLastError();
}

// ===========================================================================
// Second order (gpemu_sens_pairs / gpemu_sens_pairs_post / gpemu_sens_joint): u = {j, k}, j < k, numbered
// p(j, k) = j (2 d - j - 1) / 2 + (k - j - 1).  The pair term is  II_j II_k Pex2_jk(i) Pex2'_jk(i'),  Pex2_jk = prod_{l != j,k} I_l.
// New kernels beside the ones above, which they leave as they are; the per-point tables and cst are sens_prep_kernel's.
// ===========================================================================
constexpr int SENS_PB = 8;                                                        // coordinates of a block of the pair sweep

__host__ __device__ __forceinline__ int sens_pair_index(int j, int k, int d) { return j * (2 * d - j - 1) / 2 + (k - j - 1); }

// pair p -> (j, k)
__device__ __forceinline__ void sens_pair_coords(int p, int d, int &j, int &k)
{
	j = 0;
	while (p >= d - 1 - j) { p -= d - 1 - j; j++; }
	k = j + 1 + p;
}

// ---------------------------------------------------------------------------
// pair prep: workgroup (x, c, j) writes, for 256 design points of context c, Pex2_jk(i) for every k > j:
// table c at pex2 + c * npairs * N, pair p at p * N + i.  prod_{l < j} I_l, then the suffix products on the way down and the
// running middle products on the way up, in the table itself: O(d^2) products per point, no division (the factors underflow
// to 0 for far points), no private array.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sens_pair_prep_kernel(const double *prep, int N, int d, double *pex2)
{
	const int c = blockIdx.y, j = blockIdx.z, i = blockIdx.x * 256 + threadIdx.x;
	if (i >= N) return;
	const double *I = prep + (long)c * 5 * d * N + i;                             // I_l(i) at I[l * N]
	double *out = pex2 + ((long)c * (d * (d - 1) / 2) + sens_pair_index(j, j + 1, d)) * N + i;   // pair (j, k) at out[(k - j - 1) * N]
	double pre = 1.0;
	for (int l = 0; l < j; l++) pre *= I[(long)l * N];
	double suf = 1.0;
	for (int k = d - 1; k > j; k--) {
		out[(long)(k - j - 1) * N] = pre * suf;
		suf *= I[(long)k * N];
	}
	double mid = 1.0;
	for (int k = j + 1; k < d; k++) {
		out[(long)(k - j - 1) * N] *= mid;
		mid *= I[(long)k * N];
	}
}

// ---------------------------------------------------------------------------
// pair sweep: the N x N square of point pairs in 64 x 64 tiles (blockIdx.x, .y) as sens_sweep_kernel walks it, times the
// blocks of SENS_PB x SENS_PB coordinates (Ja <= Kb) in blockIdx.z.  DIAG: Ja = Kb = z, the 28 pairs j < k of one block, 8 II
// values per pair of points; otherwise z numbers the blocks Ja < Kb, 64 pairs, 16 II values.  A thread owns a row and the
// columns wave + 4 k of every 16-column chunk, whose coordinates and weights gamma'_i' Pex2'_jk(i') go through LDS (slot
// jj * 8 + kk of 64 per column, a diagonal block uses those with jj < kk); it keeps one sum per pair in registers (the loops
// unroll completely: no private memory) and applies the row's own gamma_i Pex2_jk(i) once at the end.  Then the butterfly over
// the lanes, the four waves in order, and part[tile * npairs + p(j, k)].  Coordinates >= d give II = 0 and weights 0 and are
// never stored; rows and columns >= N are computed on zero coordinates with zero weights: finite values times 0.
// WEIGHTED (gpemu_sens_pairs_post; one context): P_ii' from sens_pmat_kernel in place of gamma_i gamma'_i', one workgroup
// per LOWER tile (blockIdx.x), sums counted twice off the diagonal.
// MEAS: as for sens_sweep_kernel; a block of 8 x 8 coordinates may hold both kinds, and takes the branch per coordinate.
// ---------------------------------------------------------------------------
template <bool DIAG, bool WEIGHTED, int MEAS>
__global__ __launch_bounds__(256) void sens_pair_sweep_kernel(const double *X, int N, int d, const double *gamA, const double *gamB,
                                                              const double *pex2A, const double *pex2B, const double *cst, double *part,
                                                              const double *Pw)
{
	constexpr int B = SENS_PB, NC = DIAG ? B : 2 * B, NP = B * B;
	constexpr int CR = MEAS == 2 ? SENS_CST_KIND + 1 : SENS_CST;                  // rows of cst staged: the mixed form reads the kind
	__shared__ double cst_s[CR * 2 * B], xb_s[SENS_CHUNK * 2 * B], w_s[SENS_CHUNK * NP], red[4 * NP];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	int tr = blockIdx.y, tc = blockIdx.x;
	if constexpr (WEIGHTED) sens_lower_tile(blockIdx.x, tr, tc);
	int Ja = blockIdx.z, Kb = blockIdx.z;
	if constexpr (!DIAG) {
		sens_lower_tile(blockIdx.z, Kb, Ja);                                      // Ja <= Kb' < Kb' + 1
		Kb += 1;
	}
	const int npairs = d * (d - 1) / 2;
	// slot t of the NC coordinates: the block Ja first, then (off the diagonal) the block Kb
	auto coord = [&](int t) { return (t < B ? Ja : Kb) * B + (t & (B - 1)); };
	for (int e = tid; e < CR * NC; e += 256) {
		const int r = e / NC, t = e % NC, l = coord(t);
		cst_s[r * 2 * B + t] = l < d ? cst[r * GPEMU_MAX_PARAMS + l] : 0.0;
	}
	const int row = tr * 64 + lane;
	const bool rowv = row < N;
	[[maybe_unused]] const long ldp = (long)((N + 63) / 64) * 64;
	double xr[NC], acc[NP];
#pragma unroll
	for (int t = 0; t < NC; t++) {
		const int l = coord(t);
		xr[t] = (rowv && l < d) ? X[(long)row * d + l] : 0.0;
	}
#pragma unroll
	for (int e = 0; e < NP; e++) acc[e] = 0.0;
	for (int ch = 0; ch < 64 / SENS_CHUNK; ch++) {
		__syncthreads();
		for (int e = tid; e < SENS_CHUNK * NC; e += 256) {
			const int cc = e % SENS_CHUNK, t = e / SENS_CHUNK, l = coord(t);
			const int col = tc * 64 + ch * SENS_CHUNK + cc;
			xb_s[cc * 2 * B + t] = (col < N && l < d) ? X[(long)col * d + l] : 0.0;
		}
		for (int e = tid; e < SENS_CHUNK * NP; e += 256) {
			const int cc = e % SENS_CHUNK, lp = e / SENS_CHUNK;
			const int col = tc * 64 + ch * SENS_CHUNK + cc;
			const int j = Ja * B + lp / B, k = Kb * B + lp % B;
			double w = 0.0;
			if (col < N && j < k && k < d) {
				w = pex2B[(long)sens_pair_index(j, k, d) * N + col];
				if constexpr (!WEIGHTED) w *= gamB[col];
			}
			w_s[cc * NP + lp] = w;
		}
		__syncthreads();
		for (int k4 = 0; k4 < SENS_CHUNK / 4; k4++) {
			const int cc = wave + 4 * k4;
			const double *xc = xb_s + cc * 2 * B, *w = w_s + cc * NP;
			double a[NC];
#pragma unroll
			for (int t = 0; t < NC; t++) {
				a[t] = 0.0;
				if (coord(t) >= d) continue;
				if constexpr (MEAS == 0) {
					const double dx = xr[t] - xc[t];
					const double c = cst_s[1 * 2 * B + t] * xr[t] + cst_s[2 * 2 * B + t] * xc[t], al = cst_s[3 * 2 * B + t];
					a[t] = exp(-0.5 * cst_s[0 * 2 * B + t] * dx * dx) * cst_s[4 * 2 * B + t] *
					       erf_diff(al * (cst_s[5 * 2 * B + t] - c), al * (cst_s[6 * 2 * B + t] - c));
				} else {
					a[t] = sens_pair_factor<MEAS>(xr[t], xc[t], cst_s[0 * 2 * B + t], cst_s[1 * 2 * B + t], cst_s[2 * 2 * B + t],
					                              cst_s[3 * 2 * B + t], cst_s[4 * 2 * B + t], cst_s[5 * 2 * B + t], cst_s[6 * 2 * B + t],
					                              MEAS == 2 ? cst_s[(CR - 1) * 2 * B + t] : 0.0);
				}
			}
			[[maybe_unused]] double pw = 1.0;
			if constexpr (WEIGHTED) pw = Pw[(long)(tc * 64 + ch * SENS_CHUNK + cc) * ldp + row];
#pragma unroll
			for (int jj = 0; jj < B; jj++) {
				const double aj = WEIGHTED ? pw * a[jj] : a[jj];
#pragma unroll
				for (int kk = DIAG ? jj + 1 : 0; kk < B; kk++)
					acc[jj * B + kk] = fma(w[jj * B + kk], aj * a[DIAG ? kk : B + kk], acc[jj * B + kk]);
			}
		}
	}
	// the row's own factor, the 64 rows of the wave by a butterfly, the four waves in order
	double gr;
	if constexpr (WEIGHTED) gr = rowv ? 1.0 : 0.0;
	else gr = rowv ? gamA[row] : 0.0;
#pragma unroll
	for (int jj = 0; jj < B; jj++) {
#pragma unroll
		for (int kk = DIAG ? jj + 1 : 0; kk < B; kk++) {
			const int j = Ja * B + jj, k = Kb * B + kk;
			if (k >= d) continue;                                                 // (j < k: the same for every thread of the workgroup)
			double t = rowv ? gr * pex2A[(long)sens_pair_index(j, k, d) * N + row] * acc[jj * B + kk] : 0.0;
			for (int m = 1; m < 64; m <<= 1) t += __shfl_xor(t, m);
			if (lane == 0) red[wave * NP + jj * B + kk] = t;
		}
	}
	__syncthreads();
	if (tid < NP) {
		const int j = Ja * B + tid / B, k = Kb * B + tid % B;
		if (j < k && k < d) {
			const double t = ((red[tid] + red[NP + tid]) + red[2 * NP + tid]) + red[3 * NP + tid];
			const long p = sens_pair_index(j, k, d);
			// (weighted) an off-diagonal tile stands for its mirror image too: P and the pair terms are symmetric
			if constexpr (WEIGHTED) part[(long)blockIdx.x * npairs + p] = tr > tc ? 2.0 * t : t;
			else part[((long)tr * gridDim.x + tc) * npairs + p] = t;
		}
	}
}

// D_l of sens_finish_kernel, by its instructions in its order
__device__ double sens_dl(const SensSide &a, const SensSide &b, int order, int N, int d, int l, const double *cst, double Fa, double Fb,
                          double *red)
{
	const double Eqa = sens_eq(a.beta, order, d, l, cst), Eqb = sens_eq(b.beta, order, d, l, cst);
	double cq = 0.0;                                                              // Cov(q^a_l, q^b_l)
	for (int p = 1; p <= order; p++)
		for (int r = 1; r <= order; r++)
			cq = fma(a.beta[1 + (p - 1) * d + l] * b.beta[1 + (r - 1) * d + l],
			         sens_moment(cst, l, p + r) - sens_moment(cst, l, p) * sens_moment(cst, l, r), cq);
	const double Hab = sens_poly_kernel(a, b, order, N, d, l, red), Hba = sens_poly_kernel(b, a, order, N, d, l, red);
	return cq + (Hab - Eqa * Fb) + (Hba - Eqb * Fa);
}

// ---------------------------------------------------------------------------
// pair finish: workgroup p -> out[p] = cov_pair[p] = D_j + D_k + A A' KK_jk - F^a F^b  (the rule at sens_finish_kernel with
// u = {j, k}: E0 has left the constant term before any second moment is formed); the tiles' sums in tile order.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sens_pair_finish_kernel(const double *part, int ntiles, SensSide a, SensSide b, int N, int d,
                                                               int order, const double *cst, double *out)
{
	__shared__ double red[256];
	const int p = blockIdx.x, np = d * (d - 1) / 2;
	int j, k;
	sens_pair_coords(p, d, j, k);
	double kk = 0.0;
	for (int t = threadIdx.x; t < ntiles; t += 256) kk += part[(long)t * np + p];
	kk = block_sum(kk, red);
	const double Fa = sens_kernel_mean(a, N, d, red), Fb = sens_kernel_mean(b, N, d, red);
	double sumD = 0.0;
	if (order > 0) {
		sumD += sens_dl(a, b, order, N, d, j, cst, Fa, Fb, red);
		sumD += sens_dl(a, b, order, N, d, k, cst, Fa, Fb, red);
	}
	if (threadIdx.x == 0) out[p] = sumD + (a.A * b.A * kk - Fa * Fb);
}

// ---------------------------------------------------------------------------
// pair post finish: workgroup p -> out[p] = S_u for u = {j, k}, by the rules at sens_post_finish_kernel (CC_u, Hm_u, HK_u;
// two different coordinates of u are independent: E h_a E h_b), the weighted pair sweep's sums in tile order.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sens_pair_post_finish_kernel(const double *part, int ntiles, const double *prep, const double *G,
                                                                    const double *Q, double A, int N, int d, int nreg, const double *cst,
                                                                    double *out)
{
	__shared__ double red[256], eh[GPEMU_MAX_PARAMS];
	const int p = blockIdx.x, np = d * (d - 1) / 2, tid = threadIdx.x;
	const long q = (long)d * N;
	int j, k;
	sens_pair_coords(p, d, j, k);
	auto inu = [&](int l) { return l == j || l == k; };
	if (tid < nreg) eh[tid] = sens_eh(tid, d, cst);
	double kk = 0.0;
	for (int t = tid; t < ntiles; t += 256) kk += part[(long)t * np + p];
	kk = block_sum(kk, red);                                                      // (its barriers publish eh)
	double cc = A;
	for (int l = 0; l < d; l++)
		if (!inu(l)) cc *= sens_uu(cst, l);
	double hq = 0.0;
	for (int e = tid; e < nreg * nreg; e += 256) {
		const int a = e / nreg, b = e % nreg;
		double hm = eh[a] * eh[b];
		if (a > 0 && b > 0 && (a - 1) % d == (b - 1) % d && inu((a - 1) % d)) {
			const int l = (a - 1) % d;
			hm = sens_moment(cst, l, (a - 1) / d + (b - 1) / d + 2);
		}
		hq = fma(Q[e], hm, hq);
	}
	hq = block_sum(hq, red);
	double hk = 0.0;
	for (int i = tid; i < N; i += 256) {
		const double pi = prep[i] * prep[4 * q + i];
		double g = 0.0;
		for (int a = 0; a < nreg; a++) {
			const int l = a ? (a - 1) % d : 0, o = a ? (a - 1) / d + 1 : 0;
			const double t = (a && inu(l)) ? prep[o * q + (long)l * N + i] * prep[4 * q + (long)l * N + i] : eh[a] * pi;
			g = fma(G[(long)i * nreg + a], t, g);
		}
		hk += g;
	}
	hk = block_sum(hk, red);
	if (tid == 0) out[p] = ((cc - A * A * kk) + hq) - 2.0 * A * hk;
}

// ---------------------------------------------------------------------------
// joint: workgroup g, in the shape of sens_main_kernel, for the pair (j, k) and the point (xj[g], xk[g]):
//   joint[g] = beta_0 + q_j + q_k + sum_{l != j,k} E q_l + A sum_i gamma_i k_j k_k Pex2_jk(i),
//   inter[g] = joint - main_j - main_k + E0 = A sum_i gamma_i [k_j k_k Pex2_jk - k_j Pex_j - k_k Pex_k + prod_l I_l](i)
// -- the regression basis is additive, the polynomial parts cancel exactly and are never formed.  Workgroup 0 also writes E0.
// pex2: the table of the pair, N values.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sens_joint_kernel(const double *X, SensSide a, const double *pex2, int N, int d, int order,
                                                         const double *cst, int j, int k, const double *xj, const double *xk, double *e0,
                                                         double *joint, double *inter)
{
	__shared__ double red[256];
	const int g = blockIdx.x;
	const double sj = sens_len(cst, j), sk = sens_len(cst, k);
	const double x = xj[g], z = xk[g];
	const long q = (long)d * N;
	double vj = 0.0, vi = 0.0;
	for (int i = threadIdx.x; i < N; i += 256) {
		const double dx = x - X[(long)i * d + j], dz = z - X[(long)i * d + k];
		const double kj = exp(-0.5 * sj * dx * dx), kz = exp(-0.5 * sk * dz * dz);
		const double t = kj * kz * pex2[i];
		vj = fma(a.gam[i], t, vj);
		vi = fma(a.gam[i], ((t - kj * a.prep[4 * q + (long)j * N + i]) - kz * a.prep[4 * q + (long)k * N + i]) + a.prep[i] * a.prep[4 * q + i], vi);
	}
	const double kern = a.A * block_sum(vj, red), kint = a.A * block_sum(vi, red);
	double S = a.beta[0], rest = a.beta[0];
	for (int l = 0; l < d; l++) {
		const double Eq = sens_eq(a.beta, order, d, l, cst);
		S += Eq;
		if (l != j && l != k) rest += Eq;
	}
	double qq = 0.0, xp = 1.0, zp = 1.0;
	for (int p = 1; p <= order; p++) {
		xp *= x;
		zp *= z;
		qq += a.beta[1 + (p - 1) * d + j] * xp + a.beta[1 + (p - 1) * d + k] * zp;
	}
	if (threadIdx.x == 0) {
		joint[g] = rest + qq + kern;
		inter[g] = kint;
	}
	if (g == 0) {
		const double F = sens_kernel_mean(a, N, d, red);
		if (threadIdx.x == 0) *e0 = S + F;
	}
}

size_t sens_pex2_elems(int N, int d) { return (size_t)2 * (size_t)(d * (d - 1) / 2) * N; }
size_t sens_pair_part_elems(int N, int d) { const size_t nt = (size_t)((N + 63) / 64); return nt * nt * (size_t)(d * (d - 1) / 2); }

hipError_t launch_sens_pair_prep(hipStream_t s, const double *prep, int N, int d, double *pex2)
{
	if (N < 1 || d < 2 || d > GPEMU_MAX_PARAMS) return hipErrorInvalidValue;
	hipLaunchKernelGGL(sens_pair_prep_kernel, dim3((N + 255) / 256, 2, d - 1), dim3(256), 0, s, prep, N, d, pex2);
	return hipGetLastError();
}

// the diagonal coordinate blocks, then (d > SENS_PB) the blocks Ja < Kb; Pw = nullptr: unweighted over the full square of
// tiles, else weighted over the lower tiles (gamA, gamB not read, pex2 of context 0 on both sides)
template <int MEAS>
static void sens_pair_sweep_launch(hipStream_t s, const double *X, int N, int d, const double *gamA, const double *gamB, const double *pa,
                                   const double *pb, const double *cst, const double *Pw, double *part)
{
	const int nt = (N + 63) / 64, nb = (d + SENS_PB - 1) / SENS_PB, noff = nb * (nb - 1) / 2;
	if (Pw) {
		const int ntl = nt * (nt + 1) / 2;
		hipLaunchKernelGGL((sens_pair_sweep_kernel<true, true, MEAS>), dim3(ntl, 1, nb), dim3(256), 0, s, X, N, d, gamA, gamB, pa, pb, cst, part, Pw);
		if (noff)
			hipLaunchKernelGGL((sens_pair_sweep_kernel<false, true, MEAS>), dim3(ntl, 1, noff), dim3(256), 0, s, X, N, d, gamA, gamB, pa, pb, cst, part, Pw);
	} else {
		hipLaunchKernelGGL((sens_pair_sweep_kernel<true, false, MEAS>), dim3(nt, nt, nb), dim3(256), 0, s, X, N, d, gamA, gamB, pa, pb, cst, part, Pw);
		if (noff)
			hipLaunchKernelGGL((sens_pair_sweep_kernel<false, false, MEAS>), dim3(nt, nt, noff), dim3(256), 0, s, X, N, d, gamA, gamB, pa, pb, cst, part, Pw);
	}
}

hipError_t launch_sens_pair_sweep(hipStream_t s, const double *X, int N, int d, const double *gamA, const double *gamB, const double *pex2,
                                  const double *cst, int meas, const double *Pw, double *part)
{
	if (N < 1 || d < 2 || d > GPEMU_MAX_PARAMS || meas < 0 || meas > 2) return hipErrorInvalidValue;
	const double *pa = pex2, *pb = Pw ? pex2 : pex2 + sens_pex2_elems(N, d) / 2;
	if (meas == 0) sens_pair_sweep_launch<0>(s, X, N, d, gamA, gamB, pa, pb, cst, Pw, part);
	else if (meas == 1) sens_pair_sweep_launch<1>(s, X, N, d, gamA, gamB, pa, pb, cst, Pw, part);
	else sens_pair_sweep_launch<2>(s, X, N, d, gamA, gamB, pa, pb, cst, Pw, part);
	return hipGetLastError();
}

hipError_t launch_sens_pair_finish(hipStream_t s, const double *part, int N, int d, int order, const double *gamA, const double *betaA,
                                   double ampA, const double *gamB, const double *betaB, double ampB, const double *prep, const double *cst,
                                   double *out)
{
	const int nt = (N + 63) / 64;
	const SensSide a{gamA, betaA, prep, ampA}, b{gamB, betaB, prep + (size_t)5 * d * N, ampB};
	hipLaunchKernelGGL(sens_pair_finish_kernel, dim3(d * (d - 1) / 2), dim3(256), 0, s, part, nt * nt, a, b, N, d, order, cst, out);
	return hipGetLastError();
}

hipError_t launch_sens_pair_post_finish(hipStream_t s, const double *part, int N, int d, int nreg, double amp, const double *prep,
                                        const double *cst, const double *G, const double *Q, double *out)
{
	const int nt = (N + 63) / 64;
	hipLaunchKernelGGL(sens_pair_post_finish_kernel, dim3(d * (d - 1) / 2), dim3(256), 0, s, part, nt * (nt + 1) / 2, prep, G, Q, amp, N, d,
	                   nreg, cst, out);
	return hipGetLastError();
}

hipError_t launch_sens_joint(hipStream_t s, const double *X, int N, int d, int order, const double *gam, const double *beta, double amp,
                             const double *prep, const double *pex2, const double *cst, int j, int k, int npts, const double *xj,
                             const double *xk, double *e0, double *joint, double *inter)
{
	if (npts < 1 || N < 1 || d < 2 || d > GPEMU_MAX_PARAMS || j < 0 || k <= j || k >= d) return hipErrorInvalidValue;
	const SensSide a{gam, beta, prep, amp};
	hipLaunchKernelGGL(sens_joint_kernel, dim3(npts), dim3(256), 0, s, X, a, pex2 + (size_t)sens_pair_index(j, k, d) * N, N, d, order, cst, j, k,
	                   xj, xk, e0, joint, inter);
	return hipGetLastError();
}

} // namespace gpemu
