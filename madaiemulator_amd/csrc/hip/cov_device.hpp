// cov_device.hpp -- the difference-form element of the three covariance functions and the 64 x 64 tile of it, shared by the
// fills of kernels_cov.hip and the target sweep of kernels_design.hip.  Device code only; every function is
// inlined where it is used, so the two translation units evaluate an element with the same instructions.
#pragma once
#include "gpemu_internal.hpp"

namespace gpemu {

constexpr int FT = 64;            // fill tile edge
constexpr int DCH = 8;            // dimensions handled per register chunk

// exp(x) for x <= 0: x = (64 m + j) ln2/64 + r, |r| <= ln2/128; exp = 2^m * 2^(j/64) * P5(r) (truncation 4e-17), ~1 ulp.
// 11 fp64 VALU operations: the rounding to an integer is the 1.5 * 2^52 addition (the integer
// sits in the low mantissa word: no rint, no convert), the scaling by 2^m an integer add on the exponent field (no
// ldexp).  Arguments below -700 are treated as -700 (1e-304: the result stays a normal number for the exponent add).
constexpr int EXP_TAB = 64;
__device__ __forceinline__ double fast_exp_neg(double x, const double *tab /* LDS: 2^(j/64), j < 64 */)
{
	x = fmax(x, -700.0);
	const double magic = 6755399441055744.0;                              // 1.5 * 2^52
	const double t = fma(x, 92.332482616893656768, magic);                // 64 / ln 2
	const int ki = __double2loint(t);
	const double kf = t - magic;
	double r = fma(kf, -1.08304246932675596327e-02, x);                   // ln2_hi / 64 (32 significant bits: exact product)
	r = fma(kf, -2.98158582698529346878e-12, r);                          // ln2_lo / 64
	double p = fma(r, 1.0 / 120.0, 1.0 / 24.0);
	p = fma(p, r, 1.0 / 6.0);
	p = fma(p, r, 0.5);
	p = fma(p, r, 1.0);
	p = fma(p, r, 1.0);
	const double v = tab[ki & (EXP_TAB - 1)] * p;
	return __hiloint2double(__double2hiint(v) + ((ki >> 6) << 20), __double2loint(v));
}

// sqrt(a), a >= 0: hardware rsqrt estimate + two Heron corrections
__device__ __forceinline__ double fast_sqrt(double a)
{
	const double y = __builtin_amdgcn_rsq(a);
	double s = a * y;
	const double h = 0.5 * y;
	s = fma(fma(-s, s, a), h, s);
	s = fma(fma(-s, s, a), h, s);
	return (a > 0.0) ? s : 0.0;
}

// value of an element from a = sum ((x_k - y_k) w_k)^2, difference form, before the nugget rule and the clamp (shared by the
// stored fill below and the fused mean sweep, predict_mean_kernel)
__device__ __forceinline__ double cov_from_a_diff(double a, int kind, double amp, const double *tab /* LDS: 2^(j/64) */)
{
	if (kind == GPEMU_POWEREXP) return fast_exp_neg(-a, tab) * amp;                 // emulator.c:133,141
	const double sdist = fast_sqrt(a);                                              // distance / rho
	if (kind == GPEMU_MATERN32) {
		const double root3 = 1.732050808;                                           // emulator.c:359 (literal)
		return amp * (1 + root3 * sdist) * fast_exp_neg(-root3 * sdist, tab);
	}
	const double root5 = 2.236067978;                                               // emulator.c:452 (literal)
	return amp * (1 + root5 * sdist + (5.0 / 3.0) * sdist * sdist) * fast_exp_neg(-root5 * sdist, tab);
}

// out[r][c] = cov(Xr[r], Xc[c]);  rows/cols beyond nr/nc (padding up to the
// launch grid) get identity (square factorisation matrix) or zero.
// p.w[k] is the per-dimension scale applied while staging: pow-exp sqrt(0.5)/r_k (so the exponent is
// -sum d'^2), Matern 1/rho (so sqrt(sum d'^2) is distance/rho).  p.eps is the reference's per-coordinate
// "same point" threshold on the UNSCALED coordinates; p.cand bounds sum d'^2 for pairs that can pass it.
//
// the elements of one FT x FT tile (tr, tc) of the fill: emit(t, row, col, v) receives element (row tr * FT + (tid >> 6) + 4 t,
// column tc * FT + (tid & 63)), t = 0 .. 15, where the value is made.  Shared by the stored fill (cov_fill_tile), the prior
// tile of the joint posterior covariance (predict_cov_prior_kernel) and the target sweep (design_target_sweep_kernel).
template <class Emit>
__device__ __forceinline__ void cov_tile_values(const double *Xr, int nr, const double *Xc, int nc, int d, const CovParams &p, int mode,
                                                int tr, int tc, Emit &&emit)
{
	__shared__ double xr_s[FT * (GPEMU_MAX_PARAMS + 1)];
	__shared__ double tab[EXP_TAB];
	const int tid = threadIdx.x;
	const int sd = d + 1;
	for (int e = tid; e < FT * d; e += 256) {
		int r = e / d, k = e % d;
		int gr = tr * FT + r;
		xr_s[r * sd + k] = (gr < nr) ? Xr[(long)gr * d + k] * p.w[(p.kind == GPEMU_POWEREXP) ? k : 0] : 0.0;
	}
	if (tid < EXP_TAB) tab[tid] = exp2((double)tid * (1.0 / EXP_TAB));
	__syncthreads();

	const int col = tc * FT + (tid & 63);
	const int rsub = tid >> 6;                 // rows rsub, rsub+4, ...
	const bool colv = col < nc;

	double acc[16];
#pragma unroll
	for (int t = 0; t < 16; t++) acc[t] = 0.0;

	for (int k0 = 0; k0 < d; k0 += DCH) {
		double xc[DCH];
#pragma unroll
		for (int k = 0; k < DCH; k++) {
			const bool kv = (k0 + k) < d;
			xc[k] = (kv && colv) ? Xc[(long)col * d + k0 + k] * p.w[(p.kind == GPEMU_POWEREXP) ? (k0 + k) : 0] : 0.0;
		}
#pragma unroll
		for (int t = 0; t < 16; t++) {
			const double *xr = &xr_s[(rsub + 4 * t) * sd + k0];
#pragma unroll
			for (int k = 0; k < DCH; k++) {
				if (k0 + k < d) {
					const double diff = xr[k] - xc[k];
					acc[t] = fma(diff, diff, acc[t]);
				}
			}
		}
	}

#pragma unroll
	for (int t = 0; t < 16; t++) {
		const int row = tr * FT + rsub + 4 * t;
		double v;
		if (row < nr && colv) {
			const double a = acc[t];
			v = cov_from_a_diff(a, p.kind, p.amp, tab);
			if (a <= p.cand) {
				// rare: the two points may coincide in every coordinate -> exact test on the raw coordinates
				// (emulator.c:136-150 / :368-384 / :462-478: nugget wherever ALL |x_k - y_k| < eps)
				int cnt = 0;
				for (int k = 0; k < d; k++)
					cnt += (fabs(Xr[(long)row * d + k] - Xc[(long)col * d + k]) < p.eps) ? 1 : 0;
				if (cnt == d) v += p.nug;
			}
			if ((mode & FILL_CLAMP) && v < 1E-10) v = 0.0;                          // emulator.c:588-590
		} else {
			v = ((mode & FILL_IDENT_PAD) && row == col) ? 1.0 : 0.0;
		}
		emit(t, row, col, v);
	}
}

} // namespace gpemu
