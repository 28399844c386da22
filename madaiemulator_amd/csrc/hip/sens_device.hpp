// sens_device.hpp -- the device functions that kernels_sens.hip and kernels_design.hip share: the erf difference, the pair
// factor II_l of one coordinate, the moments E x^p under the measure, the enumeration of lower tiles.  They are the functions
// kernels_sens.hip held before there was a second user, moved here word for word (all inlined: its kernels compile to the
// instructions they compiled to before).
#pragma once
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

// the pair factor II_l of one coordinate from its seven constants c0 .. c6 (rows 0 .. 6 of cst) and, MEAS = 2, its kind
template <int MEAS>
__device__ __forceinline__ double sens_pair_factor(double xa, double xb, double c0, double c1, double c2, double c3, double c4, double c5,
                                                   double c6, double kind)
{
	const double dx = xa - xb;
	if (MEAS == 1 || (MEAS == 2 && kind != 0.0)) {
		const double da = xa - c5, db = xb - c5;
		return c4 * exp(-0.5 * fma(c0 * dx, dx, fma(c1 * da, da, c2 * db * db)));
	}
	const double c = c1 * xa + c2 * xb;
	return exp(-0.5 * c0 * dx * dx) * c4 * erf_diff(c3 * (c5 - c), c3 * (c6 - c));
}

// lower tile t = tr (tr + 1) / 2 + tc, tc <= tr, of a launch over the lower 64 x 64 tiles alone
__device__ __forceinline__ void sens_lower_tile(int t, int &tr, int &tc)
{
	int r = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
	while (r * (r + 1) / 2 > t) r--;
	while ((r + 1) * (r + 2) / 2 <= t) r++;
	tr = r;
	tc = t - r * (r + 1) / 2;
}

__device__ __forceinline__ double sens_moment(double lo, double hi, int p)
{
	double a = hi, b = lo;
	for (int k = 0; k < p; k++) { a *= hi; b *= lo; }
	return (a - b) / ((p + 1) * (hi - lo));
}

// E x_l^p under the measure of coordinate l, from the rows of cst: the box's moment above, or for a Gaussian coordinate
// m_0 = 1, m_1 = mu, m_n = mu m_{n-1} + (n - 1) sg^2 m_{n-2}
__device__ __forceinline__ double sens_moment(const double *cst, int l, int p)
{
	const double lo = cst[5 * GPEMU_MAX_PARAMS + l], hi = cst[6 * GPEMU_MAX_PARAMS + l];
	if (cst[SENS_CST_KIND * GPEMU_MAX_PARAMS + l] != 0.0) {
		double m0 = 1.0, m1 = lo;
		for (int n = 2; n <= p; n++) {
			const double m = fma(lo, m1, (n - 1) * (hi * hi) * m0);
			m0 = m1;
			m1 = m;
		}
		return p ? m1 : m0;
	}
	return sens_moment(lo, hi, p);
}

// E h_a under the measure: 1 for the constant, E x_l^p for a = 1 + (p - 1) d + l
__device__ __forceinline__ double sens_eh(int a, int d, const double *cst)
{
	if (a == 0) return 1.0;
	const int l = (a - 1) % d, p = (a - 1) / d + 1;
	return sens_moment(cst, l, p);
}

} // namespace gpemu
