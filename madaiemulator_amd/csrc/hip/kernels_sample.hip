// kernels_sample.hip -- the affine-invariant ensemble sampler's own launches (gpemu.h): the stretch proposal
// of one half of the walkers against the other half (Goodman & Weare 2010, in the parallel form of Foreman-Mackey et al.
// 2013), the accept step, and the log posterior of given points for the start of a run.  The random numbers are counter
// based (sample_philox.hpp): a walker's draws depend on (seed, walker, step) alone, never on a launch's shape.
//
// Host part: gpemu_philox4x32 and gpemu_sample_uniforms, the kernels' generator for a caller without a device.
//
// The prior table (SAMPLE_PRIOR_ROWS rows of GPEMU_MAX_PARAMS): row 0 the kind (0.0 / 1.0), rows 1-2 lo and hi (Gaussian:
// mean and standard deviation), row 3 the coordinate's constant, -log(hi - lo) or -log sd - log(2 pi) / 2.
#include "gpemu_internal.hpp"
#include "sample_philox.hpp"

#include <cmath>

namespace gpemu {

constexpr int SAMPLE_WPB = 64;       // walkers of a workgroup
constexpr int SAMPLE_BLOCK = 256;    // its lanes: they walk the flat tile of the walkers' coordinates

// the stretch z = ((a - 1) u + 1)^2 / a: density proportional to 1 / sqrt(z) on [1 / a, a].  No contraction: +, * and / of
// fp64 round once each, so the device, the host and a numpy replica agree bit for bit
__host__ __device__ inline double sample_stretch(double a, double u)
{
#pragma clang fp contract(off)
	const double s = (a - 1.0) * u + 1.0;
	return s * s / a;
}

// one coordinate's log prior; a NaN counts as outside a uniform coordinate's interval
__device__ inline double sample_prior_term(const double *__restrict__ prior, int c, double v)
{
#pragma clang fp contract(off)
	const double lo = prior[GPEMU_MAX_PARAMS + c], hi = prior[2 * GPEMU_MAX_PARAMS + c], cst = prior[3 * GPEMU_MAX_PARAMS + c];
	if (prior[c] != 0.0) {
		const double r = (v - lo) / hi;
		return -0.5 * (r * r) + cst;
	}
	return (v >= lo && v <= hi) ? cst : -INFINITY;
}

// Workgroup b owns the active walkers i0 = 64 b ... of the half.  Phase 1, one lane per walker: the two uniforms, the partner
// and the stretch into LDS, (d - 1) log z out.  Phase 2, every lane over the flat 64 x d tile: the walker's own row and the
// tile of y are unit-stride across the wave for any d (the partner's row is a gather by its nature: whole rows, contiguous
// in the coordinate); each element's prior term goes to LDS.  Phase 3, one lane per walker: the terms in index order from 0.0.
__global__ __launch_bounds__(SAMPLE_BLOCK) void sample_propose_kernel(int W, int d, int half, unsigned long long step,
                                                                       unsigned long long seed, double a,
                                                                       const double *__restrict__ prior,
                                                                       const double *__restrict__ x, double *__restrict__ y,
                                                                       double *__restrict__ aux)
{
#pragma clang fp contract(off)
	__shared__ double zs[SAMPLE_WPB];
	__shared__ int js[SAMPLE_WPB];
	__shared__ double term[SAMPLE_WPB * GPEMU_MAX_PARAMS];
	const int h = W / 2;
	const int i0 = blockIdx.x * SAMPLE_WPB;
	const int nq = min(SAMPLE_WPB, h - i0);
	const int base = half * h, other = (1 - half) * h;
	if ((int)threadIdx.x < nq) {
		const int i = i0 + threadIdx.x;
		double u1, u2;
		sample_u12(seed, (uint32_t)(base + i), step, &u1, &u2);
		int j = (int)(u1 * (double)h);
		if (j > h - 1) j = h - 1;
		const double z = sample_stretch(a, u2);
		js[threadIdx.x] = other + j;
		zs[threadIdx.x] = z;
		aux[i] = d == 1 ? 0.0 : (double)(d - 1) * log(z);
	}
	__syncthreads();
	const long xk0 = (long)(base + i0) * d, y0 = (long)i0 * d;
	for (int e = threadIdx.x; e < nq * d; e += SAMPLE_BLOCK) {
		const int ql = e / d, c = e - ql * d;
		const double xj = x[(long)js[ql] * d + c], xk = x[xk0 + e];
		const double v = xj + zs[ql] * (xk - xj);
		y[y0 + e] = v;
		term[e] = sample_prior_term(prior, c, v);
	}
	__syncthreads();
	if ((int)threadIdx.x < nq) {
		double s = 0.0;
		for (int c = 0; c < d; c++) s += term[threadIdx.x * d + c];
		aux[h + i0 + threadIdx.x] = s;
	}
}

// Phase 1, one lane per active walker: the decision; lp and the count of the walkers that move.  Phase 2, every lane over the
// flat tile: the rows of the walkers that move, unit-stride.  A walker has one owner: no atomics.
__global__ __launch_bounds__(SAMPLE_BLOCK) void sample_accept_kernel(int W, int d, int half, unsigned long long step,
                                                                      unsigned long long seed, const double *__restrict__ y,
                                                                      const double *__restrict__ aux,
                                                                      const double *__restrict__ loglik, double *__restrict__ x,
                                                                      double *__restrict__ lp, int *__restrict__ nacc)
{
#pragma clang fp contract(off)
	__shared__ int take[SAMPLE_WPB];
	const int h = W / 2;
	const int i0 = blockIdx.x * SAMPLE_WPB;
	const int nq = min(SAMPLE_WPB, h - i0);
	const int base = half * h;
	if ((int)threadIdx.x < nq) {
		const int i = i0 + threadIdx.x, k = base + i;
		const double lpy = loglik[i] + aux[h + i];
		const double u3 = sample_u3(seed, (uint32_t)k, step);
		const bool ok = isfinite(lpy) && log(u3) < aux[i] + lpy - lp[k];
		take[threadIdx.x] = ok;
		if (ok) {
			lp[k] = lpy;
			nacc[k] += 1;
		}
	}
	__syncthreads();
	const long xk0 = (long)(base + i0) * d, y0 = (long)i0 * d;
	for (int e = threadIdx.x; e < nq * d; e += SAMPLE_BLOCK)
		if (take[e / d]) x[xk0 + e] = y[y0 + e];
}

// lp[q] = loglik[q] + log prior of row q of x, the prior's terms in index order from 0.0: the same tile walk
__global__ __launch_bounds__(SAMPLE_BLOCK) void sample_logpost_kernel(int M, int d, const double *__restrict__ prior,
                                                                       const double *__restrict__ x,
                                                                       const double *__restrict__ loglik, double *__restrict__ lp)
{
#pragma clang fp contract(off)
	__shared__ double term[SAMPLE_WPB * GPEMU_MAX_PARAMS];
	const int i0 = blockIdx.x * SAMPLE_WPB;
	const int nq = min(SAMPLE_WPB, M - i0);
	const long x0 = (long)i0 * d;
	for (int e = threadIdx.x; e < nq * d; e += SAMPLE_BLOCK) {
		const int ql = e / d;
		term[e] = sample_prior_term(prior, e - ql * d, x[x0 + e]);
	}
	__syncthreads();
	if ((int)threadIdx.x < nq) {
		double s = 0.0;
		for (int c = 0; c < d; c++) s += term[threadIdx.x * d + c];
		lp[i0 + threadIdx.x] = loglik[i0 + threadIdx.x] + s;
	}
}

void sample_fill_prior(int d, const int *kind, const double *lo, const double *hi, double *tab)
{
	for (int c = 0; c < SAMPLE_PRIOR_ROWS * GPEMU_MAX_PARAMS; c++) tab[c] = 0.0;
	for (int c = 0; c < d; c++) {
		const bool g = kind && kind[c] == GPEMU_MEASURE_GAUSS;
		tab[c] = g ? 1.0 : 0.0;
		tab[GPEMU_MAX_PARAMS + c] = lo[c];
		tab[2 * GPEMU_MAX_PARAMS + c] = hi[c];
		tab[3 * GPEMU_MAX_PARAMS + c] = g ? -std::log(hi[c]) - 0.91893853320467274178032973640562 : -std::log(hi[c] - lo[c]);
	}
}

hipError_t launch_sample_propose(hipStream_t s, const double *prior, int W, int d, int half, unsigned long long step,
                                 unsigned long long seed, double a, const double *x, double *y, double *aux)
{
	const int h = W / 2;
	hipLaunchKernelGGL(sample_propose_kernel, dim3((h + SAMPLE_WPB - 1) / SAMPLE_WPB), dim3(SAMPLE_BLOCK), 0, s, W, d, half, step, seed, a,
	                   prior, x, y, aux);
	return hipGetLastError();
}

hipError_t launch_sample_accept(hipStream_t s, int W, int d, int half, unsigned long long step, unsigned long long seed, const double *y,
                                const double *aux, const double *loglik, double *x, double *lp, int *nacc)
{
	const int h = W / 2;
	hipLaunchKernelGGL(sample_accept_kernel, dim3((h + SAMPLE_WPB - 1) / SAMPLE_WPB), dim3(SAMPLE_BLOCK), 0, s, W, d, half, step, seed, y,
	                   aux, loglik, x, lp, nacc);
	return hipGetLastError();
}

hipError_t launch_sample_logpost(hipStream_t s, const double *prior, int M, int d, const double *x, const double *loglik, double *lp)
{
	hipLaunchKernelGGL(sample_logpost_kernel, dim3((M + SAMPLE_WPB - 1) / SAMPLE_WPB), dim3(SAMPLE_BLOCK), 0, s, M, d, prior, x, loglik, lp);
	return hipGetLastError();
}

} // namespace gpemu

extern "C" int gpemu_philox4x32(const unsigned ctr[4], const unsigned key[2], unsigned out[4])
{
	if (!ctr || !key || !out) return GPEMU_ERR_ARG;
	const uint32_t c[4] = {ctr[0], ctr[1], ctr[2], ctr[3]}, k[2] = {key[0], key[1]};
	uint32_t o[4];
	gpemu::philox4x32_10(c, k, o);
	for (int i = 0; i < 4; i++) out[i] = o[i];
	return GPEMU_OK;
}

extern "C" int gpemu_sample_uniforms(unsigned long long seed, unsigned walker, unsigned long long step, double u[3])
{
	if (!u) return GPEMU_ERR_ARG;
	gpemu::sample_u12(seed, walker, step, &u[0], &u[1]);
	u[2] = gpemu::sample_u3(seed, walker, step);
	return GPEMU_OK;
}
