// kernels_sens.hip -- main effects and Sobol indices of the posterior mean in closed form (gpemu_sens_cov / gpemu_sens_main,
// include/gpemu.h).  Power-exponential covariance, independent uniform inputs on a box: every conditional
// expectation of  m(x) = beta_0 + sum_l q_l(x_l) + A sum_i gamma_i prod_l k_l(x_il, x_l)  is a product of one-dimensional
// integrals with an erf closed form.  Three launches: the per-point integrals (prep), the N x N sweep of pair terms into
// per-tile partial sums, and the finish that adds the partials in a fixed order and assembles the polynomial parts.
// No atomics, no workgroup waits for another; every sum has one order, so two calls return the same bits.
// Second half: the emulator uncertainty of the same quantities (gpemu_sens_post / gpemu_sens_main_var) -- the
// sweep again, weighted by an element of P = C^-1 - W Q W^T per pair, and the confidence band of the main-effect curves.
#include "gpemu_internal.hpp"

#include <cmath>

namespace gpemu {

// erf(uhi) - erf(ulo) for uhi >= ulo.  Two arguments of one sign take the erfc form: beyond |u| of about 4 both erf values
// are 1 - O(1e-8) and their difference has no relative accuracy left, while erfc keeps it down to its underflow.  A box that
// leaves design points outside makes that the common case.
__device__ __forceinline__ double erf_diff(double ulo, double uhi)
{
	if (ulo > 0.0 || uhi < 0.0) {
		const double p = fabs(ulo), q = fabs(uhi);
		return erfc(fmin(p, q)) - erfc(fmax(p, q));
	}
	return erf(uhi) - erf(ulo);
}

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
// Workgroup (0, 0) also leaves the sweep's per-coordinate constants (SENS_CST rows of GPEMU_MAX_PARAMS) in cst.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sens_prep_kernel(const double *X, int N, SensBox bx, double *prep, double *cst)
{
	const int d = bx.d, c = blockIdx.y;
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (blockIdx.x == 0 && c == 0 && threadIdx.x < d) {
		const int l = threadIdx.x;
		const double s = bx.s[l], t = bx.t[l], st = s + t, al = sqrt(0.5 * st);
		cst[0 * GPEMU_MAX_PARAMS + l] = s * t / st;                               // h: exp(-h (x - x')^2 / 2)
		cst[1 * GPEMU_MAX_PARAMS + l] = s / st;                                   // c = fa x + fb x'
		cst[2 * GPEMU_MAX_PARAMS + l] = t / st;
		cst[3 * GPEMU_MAX_PARAMS + l] = al;
		cst[4 * GPEMU_MAX_PARAMS + l] = sqrt(M_PI / (2.0 * st)) / (bx.hi[l] - bx.lo[l]);
		cst[5 * GPEMU_MAX_PARAMS + l] = bx.lo[l];
		cst[6 * GPEMU_MAX_PARAMS + l] = bx.hi[l];
	}
	if (i >= N) return;
	double *tab = prep + (long)c * 5 * d * N + i;
	const long q = (long)d * N;                                                   // one table
	for (int l = 0; l < d; l++) {
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
// ---------------------------------------------------------------------------
constexpr int SENS_CHUNK = 16;

// lower tile t = tr (tr + 1) / 2 + tc, tc <= tr, of a launch over the lower 64 x 64 tiles alone
__device__ __forceinline__ void sens_lower_tile(int t, int &tr, int &tc)
{
	int r = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
	while (r * (r + 1) / 2 > t) r--;
	while ((r + 1) * (r + 2) / 2 <= t) r++;
	tr = r;
	tc = t - r * (r + 1) / 2;
}

template <int DM, bool WEIGHTED>
__global__ __launch_bounds__(256) void sens_sweep_kernel(const double *X, int N, int d, const double *gamA, const double *gamB,
                                                         const double *prepA, const double *prepB, const double *cst, double *part,
                                                         const double *Pw)
{
	constexpr int UN = DM <= 16 ? DM : 1;
	constexpr int RS = 2 * DM + 1 + (WEIGHTED ? 1 : 0);                           // sums a wave leaves in red
	__shared__ double cst_s[SENS_CST * DM];
	__shared__ double xb_s[SENS_CHUNK * DM], wr_s[SENS_CHUNK * DM], wf_s[SENS_CHUNK * DM], gb_s[SENS_CHUNK];
	__shared__ double red[4 * RS];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	int tr = blockIdx.y, tc = blockIdx.x;
	if constexpr (WEIGHTED) sens_lower_tile(blockIdx.x, tr, tc);
	const long q = (long)d * N;
	for (int e = tid; e < SENS_CST * d; e += 256) cst_s[(e / d) * DM + e % d] = cst[(e / d) * GPEMU_MAX_PARAMS + e % d];
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
				const double dx = xr[l] - xc[l];
				const double c = cst_s[1 * DM + l] * xr[l] + cst_s[2 * DM + l] * xc[l], al = cst_s[3 * DM + l];
				const double v = exp(-0.5 * cst_s[0 * DM + l] * dx * dx) * cst_s[4 * DM + l] *
				                 erf_diff(al * (cst_s[5 * DM + l] - c), al * (cst_s[6 * DM + l] - c));
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

__device__ __forceinline__ double sens_moment(double lo, double hi, int p)
{
	double a = hi, b = lo;
	for (int k = 0; k < p; k++) { a *= hi; b *= lo; }
	return (a - b) / ((p + 1) * (hi - lo));
}

// E q_l of the side whose polynomial coefficients are beta
__device__ __forceinline__ double sens_eq(const double *beta, int order, int d, int l, double lo, double hi)
{
	double v = 0.0;
	for (int p = 1; p <= order; p++) v = fma(beta[1 + (p - 1) * d + l], sens_moment(lo, hi, p), v);
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
	const double *lo = cst + 5 * GPEMU_MAX_PARAMS, *hi = cst + 6 * GPEMU_MAX_PARAMS;
	double kk = 0.0;
	for (int t = threadIdx.x; t < ntiles; t += 256) kk += part[(long)t * np + k];
	kk = block_sum(kk, red);
	const double Fa = sens_kernel_mean(a, N, d, red), Fb = sens_kernel_mean(b, N, d, red);
	double sumD = 0.0, Sa = a.beta[0], Sb = b.beta[0];
	for (int l = 0; l < d; l++) {
		const double Eqa = sens_eq(a.beta, order, d, l, lo[l], hi[l]), Eqb = sens_eq(b.beta, order, d, l, lo[l], hi[l]);
		Sa += Eqa;
		Sb += Eqb;
		const bool inu = k == 0 || (k <= d ? l == k - 1 : l != k - 1 - d);
		if (!inu || order == 0) continue;
		double cq = 0.0;                                                          // Cov(q^a_l, q^b_l)
		for (int p = 1; p <= order; p++)
			for (int r = 1; r <= order; r++)
				cq = fma(a.beta[1 + (p - 1) * d + l] * b.beta[1 + (r - 1) * d + l],
				         sens_moment(lo[l], hi[l], p + r) - sens_moment(lo[l], hi[l], p) * sens_moment(lo[l], hi[l], r), cq);
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
	const double *lo = cst + 5 * GPEMU_MAX_PARAMS, *hi = cst + 6 * GPEMU_MAX_PARAMS;
	const double sj = 2.0 * cst[j];                                               // (one context, s = t: row 0 holds s t / (s + t) = s / 2)
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
		const double Eq = sens_eq(a.beta, order, d, l, lo[l], hi[l]);
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

// E h_a under the box: 1 for the constant, E x_l^p for a = 1 + (p - 1) d + l
__device__ __forceinline__ double sens_eh(int a, int d, const double *lo, const double *hi)
{
	if (a == 0) return 1.0;
	const int l = (a - 1) % d, p = (a - 1) / d + 1;
	return sens_moment(lo[l], hi[l], p);
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
	const double *lo = cst + 5 * GPEMU_MAX_PARAMS, *hi = cst + 6 * GPEMU_MAX_PARAMS;
	const long q = (long)d * N;
	(void)order;
	auto inu = [&](int l) { return k == 0 || (k <= d ? l == k - 1 : (k <= 2 * d ? l != k - 1 - d : false)); };
	if (tid < nreg) eh[tid] = sens_eh(tid, d, lo, hi);
	double kk = 0.0;
	for (int t = tid; t < ntiles; t += 256) kk += part[(long)t * np + k];
	kk = block_sum(kk, red);                                                      // (its barriers publish eh)
	double cc = A;
	for (int l = 0; l < d; l++)
		if (!inu(l)) cc *= sens_uu(2.0 * cst[l], hi[l] - lo[l]);                  // (s = t: row 0 of cst holds s / 2)
	double hq = 0.0;
	for (int e = tid; e < nreg * nreg; e += 256) {
		const int a = e / nreg, b = e % nreg;
		double hm = eh[a] * eh[b];
		if (a > 0 && b > 0 && (a - 1) % d == (b - 1) % d && inu((a - 1) % d)) {
			const int l = (a - 1) % d;
			hm = sens_moment(lo[l], hi[l], (a - 1) / d + (b - 1) / d + 2);
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
			v = A * (exp(-cst[j] * dx * dx) * prep[4 * q + (long)j * N + col]);   // (row 0 of cst: s / 2)
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
	const double *lo = cst + 5 * GPEMU_MAX_PARAMS, *hi = cst + 6 * GPEMU_MAX_PARAMS;
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
		hm = sens_eh(lane, d, lo, hi);
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
			if (l != j) cc *= sens_uu(2.0 * cst[l], hi[l] - lo[l]);
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

hipError_t launch_sens_sweep(hipStream_t s, const double *X, int N, int d, const double *gamA, const double *gamB, const double *prep,
                             const double *cst, double *part)
{
	if (N < 1 || d < 1 || d > GPEMU_MAX_PARAMS) return hipErrorInvalidValue;
	const int nt = (N + 63) / 64;
	const dim3 grid(nt, nt);
	const double *pa = prep, *pb = prep + (size_t)5 * d * N;
	const double *none = nullptr;
	if (d <= 8)
		hipLaunchKernelGGL((sens_sweep_kernel<8, false>), grid, dim3(256), 0, s, X, N, d, gamA, gamB, pa, pb, cst, part, none);
	else if (d <= 16)
		hipLaunchKernelGGL((sens_sweep_kernel<16, false>), grid, dim3(256), 0, s, X, N, d, gamA, gamB, pa, pb, cst, part, none);
	else
		hipLaunchKernelGGL((sens_sweep_kernel<GPEMU_MAX_PARAMS, false>), grid, dim3(256), 0, s, X, N, d, gamA, gamB, pa, pb, cst, part, none);
	return hipGetLastError();
}

hipError_t launch_sens_sweep_weighted(hipStream_t s, const double *X, int N, int d, const double *prep, const double *cst, const double *Pw,
                                      double *part)
{
	if (N < 1 || d < 1 || d > GPEMU_MAX_PARAMS) return hipErrorInvalidValue;
	const int nt = (N + 63) / 64;
	const dim3 grid(nt * (nt + 1) / 2);
	const double *none = nullptr;
	if (d <= 8)
		hipLaunchKernelGGL((sens_sweep_kernel<8, true>), grid, dim3(256), 0, s, X, N, d, none, none, prep, prep, cst, part, Pw);
	else if (d <= 16)
		hipLaunchKernelGGL((sens_sweep_kernel<16, true>), grid, dim3(256), 0, s, X, N, d, none, none, prep, prep, cst, part, Pw);
	else
		hipLaunchKernelGGL((sens_sweep_kernel<GPEMU_MAX_PARAMS, true>), grid, dim3(256), 0, s, X, N, d, none, none, prep, prep, cst, part, Pw);
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

} // namespace gpemu
