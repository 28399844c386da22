// kernels_design.hip -- expected reduction of the IMSE by one more run, in closed form (gpemu_design_gain, include/gpemu.h,
// DESIGN.md 4.20).  Conditioning the posterior process on a run at x* is a rank-one update of its covariance, so
//   gain(x*) = E_x[c*(x, x*)^2] / v(x*),   c*(x, x*) = c(x, x*) - k(x)^T a + h(x)^T b,   a = C^-1 k* + W Q r,  b = Q r,
// and the expectation is made of the pair factors II_l of kernels_sens.hip (sens_device.hpp) and its per-point tables:
//   num = A^2 prod_l II_l(x*, x*) - 2 A^2 sum_i a_i w_i + 2 A sum_al b_al HK*_al + A^2 a^T K a - 2 A sum_al b_al (a^T HK_al) + b^T Hm b,
//   K_ii' = prod_l II_l(x_i, x_i'),  w_i = prod_l II_l(x_i, x*),  HK_al,i = E[h_al(x) prod_l k_l(x_il, x_l)],  Hm = E[h h^T].
// K, HK and Hm depend on the design, the lengths and the measure alone: they are built once and kept.  Per block of candidates
// the unclamped k rows, then (in gpemu_api.hip) the prediction's two triangular products for a and T = a [K | HK], then the
// cross sweep for sum_i a_i (T_i - 2 w_i) and the finish.  No atomics, no workgroup waits for another; every sum has one order.
#include "gpemu_internal.hpp"
#include "sens_device.hpp"

#include <cmath>

namespace gpemu {

// the product over the coordinates of the pair factor of (xa, xb), coordinates and constants from global memory
template <int MEAS>
__device__ __forceinline__ double design_pair_product(const double *xa, const double *xb, int d, const double *cst)
{
	double v = 1.0;
	for (int l = 0; l < d; l++)
		v *= sens_pair_factor<MEAS>(xa[l], xb[l], cst[0 * GPEMU_MAX_PARAMS + l], cst[1 * GPEMU_MAX_PARAMS + l], cst[2 * GPEMU_MAX_PARAMS + l],
		                            cst[3 * GPEMU_MAX_PARAMS + l], cst[4 * GPEMU_MAX_PARAMS + l], cst[5 * GPEMU_MAX_PARAMS + l],
		                            cst[6 * GPEMU_MAX_PARAMS + l], MEAS == 2 ? cst[SENS_CST_KIND * GPEMU_MAX_PARAMS + l] : 0.0);
	return v;
}

// ---------------------------------------------------------------------------
// kmat: one workgroup per lower 64 x 64 tile (tr, tc) of K, KH[i * Np + i'] = prod_l II_l(x_i, x_i') (one context: s = t).
// A thread takes column tc * 64 + lane of the rows wave + 4 k; the factor is evaluated with the larger index first, so the
// two halves of a diagonal tile agree to the bit, and an off-diagonal tile writes its mirror image too.  Rows and columns >= N
// are 0 (Np / 64 tile rows: the whole buffer is written).  Built once per (set-up, box, kinds): no LDS, the design through
// the caches.
// ---------------------------------------------------------------------------
template <int MEAS>
__global__ __launch_bounds__(256) void design_kmat_kernel(const double *X, int N, int Np, int d, const double *cst, double *KH)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	int tr, tc;
	sens_lower_tile(blockIdx.x, tr, tc);
	const int col = tc * 64 + lane;
	for (int k = 0; k < 16; k++) {
		const int row = tr * 64 + wave + 4 * k;
		double v = 0.0;
		if (row < N && col < N) {
			const int hi = max(row, col), lo = min(row, col);
			v = design_pair_product<MEAS>(X + (long)hi * d, X + (long)lo * d, d, cst);
		}
		KH[(long)row * Np + col] = v;
		if (tr != tc) KH[(long)col * Np + row] = v;
	}
}

// ---------------------------------------------------------------------------
// hk: rows Np .. Np + 63 of KH: row Np + al holds HK_al,i for al < nreg -- prod_l I_l(i) for the constant, J^p_l(i) Pex_l(i) for
// al = 1 + (p - 1) d + l -- from the design's tables (sens_prep_kernel); the other rows and the columns i >= N are 0.
// Workgroup (0, 0) also writes Hm (64 x 64, zero beyond nreg): E h_al E h_be across coordinates, E x_l^{p+q} within one.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void design_hk_kernel(const double *prep, int N, int Np, int d, int nreg, const double *cst, double *KH,
                                                        double *Hm)
{
	const int i = blockIdx.x * 256 + threadIdx.x, al = blockIdx.y;
	const long q = (long)d * N;
	if (blockIdx.x == 0 && al == 0)
		for (int e = threadIdx.x; e < 64 * 64; e += 256) {
			const int a = e >> 6, b = e & 63;
			double hm = 0.0;
			if (a < nreg && b < nreg) {
				hm = sens_eh(a, d, cst) * sens_eh(b, d, cst);
				if (a > 0 && b > 0 && (a - 1) % d == (b - 1) % d) hm = sens_moment(cst, (a - 1) % d, (a - 1) / d + (b - 1) / d + 2);
			}
			Hm[e] = hm;
		}
	if (i >= Np) return;
	double v = 0.0;
	if (i < N && al < nreg) {
		if (al == 0) v = prep[i] * prep[4 * q + i];
		else {
			const int l = (al - 1) % d, p = (al - 1) / d + 1;
			v = prep[p * q + (long)l * N + i] * prep[4 * q + (long)l * N + i];
		}
	}
	KH[(long)(Np + al) * Np + i] = v;
}

// ---------------------------------------------------------------------------
// kvec: the unclamped k rows of mb candidates into the prediction's k-vector buffer (mbp rows of Np, mbp = mb rounded up to 64):
// Kq[q * Np + i] = A exp(-sum_l s_l (x*_ql - x_il)^2 / 2); columns i >= N and rows >= mb are 0.  No clamp and no nugget rule:
// the conventions of DESIGN.md 4.15.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void design_kvec_kernel(const double *X, int N, int Np, int d, const double *cst, double A,
                                                          const double *Xq, int mb, double *Kq)
{
	const int col = blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
	if (col >= Np) return;
	double v = 0.0;
	if (row < mb && col < N) {
		double e = 0.0;
		for (int l = 0; l < d; l++) {
			const double dx = Xq[(long)row * d + l] - X[(long)col * d + l];
			e = fma(cst[SENS_CST_S * GPEMU_MAX_PARAMS + l] * dx, dx, e);
		}
		v = A * exp(-0.5 * e);
	}
	Kq[(long)row * Np + col] = v;
}

// ---------------------------------------------------------------------------
// cross: 64 candidates x 64 design points per workgroup (blockIdx.y, blockIdx.x).  A thread owns candidate q = tile row +
// lane, its coordinates in registers, and the columns wave + 4 k of every 16-column chunk, whose coordinates go through LDS as
// in sens_sweep_kernel (every lane of a wave reads the same word); the chunk's pieces of the rows of a (Am, mbp x lda) and of
// T = a [K | HK] (Tm, ldt) are staged beside them by whole 128-byte row pieces.  Per pair w_qi = prod_l II_l(x*_q, x_i) and
//   acc += a_qi (T_qi - 2 w_qi);
// then the four waves in order and one partial per candidate and column tile: part[tile column * pstride + q].
// DM = 8, 16: the coordinate loop unrolled, DM = GPEMU_MAX_PARAMS the same loop rolled with the candidate's coordinates in
// private memory.  Rows q >= mb and columns i >= N are computed on zero coordinates with a = 0: finite values times 0.
// ---------------------------------------------------------------------------
constexpr int DESIGN_CHUNK = 16, DESIGN_LD = DESIGN_CHUNK + 1;

template <int DM, int MEAS>
__global__ __launch_bounds__(256) void design_cross_kernel(const double *X, int N, int d, const double *Xq, int mb, const double *cst,
                                                           const double *Am, long lda, const double *Tm, long ldt, double *part,
                                                           long pstride)
{
	constexpr int UN = DM <= 16 ? DM : 1;
	constexpr int CR = MEAS == 2 ? SENS_CST_KIND + 1 : SENS_CST;
	__shared__ double cst_s[CR * DM];
	__shared__ double xb_s[DESIGN_CHUNK * DM], a_s[64 * DESIGN_LD], t_s[64 * DESIGN_LD];
	__shared__ double red[4 * 64];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int tr = blockIdx.y, tc = blockIdx.x;
	for (int e = tid; e < CR * d; e += 256) cst_s[(e / d) * DM + e % d] = cst[(e / d) * GPEMU_MAX_PARAMS + e % d];
	const int row = tr * 64 + lane;
	const bool rowv = row < mb;
	const int dl = DM <= 16 ? DM : d;
	double xr[DM], acc = 0.0;
#pragma unroll UN
	for (int l = 0; l < dl; l++) xr[l] = (rowv && l < d) ? Xq[(long)row * d + l] : 0.0;
	for (int ch = 0; ch < 64 / DESIGN_CHUNK; ch++) {
		__syncthreads();
		for (int e = tid; e < DESIGN_CHUNK * d; e += 256) {
			const int cc = e % DESIGN_CHUNK, l = e / DESIGN_CHUNK;
			const int col = tc * 64 + ch * DESIGN_CHUNK + cc;
			xb_s[cc * DM + l] = col < N ? X[(long)col * d + l] : 0.0;
		}
		for (int e = tid; e < 64 * DESIGN_CHUNK; e += 256) {
			const int r = e / DESIGN_CHUNK, cc = e % DESIGN_CHUNK;
			const int q = tr * 64 + r, col = tc * 64 + ch * DESIGN_CHUNK + cc;
			const bool v = q < mb && col < N;
			a_s[r * DESIGN_LD + cc] = v ? Am[(long)q * lda + col] : 0.0;
			t_s[r * DESIGN_LD + cc] = v ? Tm[(long)q * ldt + col] : 0.0;
		}
		__syncthreads();
		for (int k = 0; k < DESIGN_CHUNK / 4; k++) {
			const int cc = wave + 4 * k;
			const double *xc = xb_s + cc * DM;
			double w = 1.0;
#pragma unroll UN
			for (int l = 0; l < dl; l++) {
				if (l >= d) continue;
				w *= sens_pair_factor<MEAS>(xr[l], xc[l], cst_s[0 * DM + l], cst_s[1 * DM + l], cst_s[2 * DM + l], cst_s[3 * DM + l],
				                            cst_s[4 * DM + l], cst_s[5 * DM + l], cst_s[6 * DM + l],
				                            MEAS == 2 ? cst_s[(CR - 1) * DM + l] : 0.0);
			}
			acc = fma(a_s[lane * DESIGN_LD + cc], t_s[lane * DESIGN_LD + cc] - 2.0 * w, acc);
		}
	}
	red[wave * 64 + lane] = acc;
	__syncthreads();
	if (tid < 64 && rowv) part[(long)tc * pstride + row] = ((red[lane] + red[64 + lane]) + red[128 + lane]) + red[192 + lane];
}

// ---------------------------------------------------------------------------
// finish: one wave per candidate q.  The partials in tile order; the self term A^2 prod_l II_l(x*, x*); with lane al holding
// b_al (V's columns Np + 1 .., predict_qr_kernel) the three b terms -- HK* from the candidate's own tables (prepq: the tables
// sens_prep_kernel wrote for the block, mb points), a^T HK from the columns Np .. of T, b^T Hm b -- and r . b; |u|^2 over the row
// of V as predict_finish_kernel takes it.  Then
//   var = (A + nugget - |u|^2) + r^T Q r,   gain = var > 0 ? num / var : 0,
// num and var as computed.  bkeep (mb x 64): b itself, for gpemu_test_design_state.
// ---------------------------------------------------------------------------
template <int MEAS>
__global__ __launch_bounds__(256) void design_finish_kernel(const double *part, long pstride, int ntc, const double *V, long ldv,
                                                            const double *R, long ldr, const double *Tm, long ldt, const double *prepq,
                                                            const double *Xq, int mb, int Np, int d, int nreg, const double *cst,
                                                            const double *Hm, double A, double kappa, double *gain, double *num,
                                                            double *var, double *bkeep)
{
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int q = min(blockIdx.x * 4 + wave, mb - 1);                             // (a spare wave repeats the last candidate and stores nothing)
	const bool store = blockIdx.x * 4 + wave < mb;
	const double *v = V + (long)q * ldv;
	double ss = 0.0;
	for (int i = lane * 2; i < Np; i += 128) {
		const double2 t = *reinterpret_cast<const double2 *>(v + i);
		ss += t.x * t.x;
		ss += t.y * t.y;
	}
	const long tq = (long)d * mb;                                                 // one table of the block
	double b = 0.0, hks = 0.0, ahk = 0.0, rb = 0.0;
	if (lane < nreg) {
		b = v[Np + 1 + lane];
		if (lane == 0) hks = prepq[q] * prepq[4 * tq + q];
		else {
			const int l = (lane - 1) % d, p = (lane - 1) / d + 1;
			hks = prepq[p * tq + (long)l * mb + q] * prepq[4 * tq + (long)l * mb + q];
		}
		ahk = Tm[(long)q * ldt + Np + lane];
		rb = R[(long)q * ldr + lane] * b;
		if (store) bkeep[(long)q * 64 + lane] = b;
	}
	double t = 0.0;
	for (int be = 0; be < nreg; be++) {
		const double bb = __shfl(b, be);
		if (lane < nreg) t = fma(Hm[lane * 64 + be], bb, t);
	}
	double p3 = b * hks, p5 = b * ahk, p6 = b * t;
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) {
		ss += __shfl_xor(ss, off);
		p3 += __shfl_xor(p3, off);
		p5 += __shfl_xor(p5, off);
		p6 += __shfl_xor(p6, off);
		rb += __shfl_xor(rb, off);
	}
	if (store && lane == 0) {
		double cross = 0.0;
		for (int tc = 0; tc < ntc; tc++) cross += part[(long)tc * pstride + q];
		const double *x = Xq + (long)q * d;
		const double self = design_pair_product<MEAS>(x, x, d, cst);
		const double n = ((A * A * self + A * A * cross) + 2.0 * A * (p3 - p5)) + p6;
		const double vv = (kappa - ss) + rb;
		gain[q] = vv > 0.0 ? n / vv : 0.0;
		if (num) num[q] = n;
		if (var) var[q] = vv;
	}
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
size_t design_kh_elems(int Np) { return (size_t)Np * ((size_t)Np + 64); }

hipError_t launch_design_kmat(hipStream_t s, const double *X, int N, int Np, int d, int nreg, const double *prep, const double *cst, int meas,
                              double *KH, double *Hm)
{
	if (N < 1 || Np < N || Np % 64 || d < 1 || d > GPEMU_MAX_PARAMS || nreg < 1 || nreg > 63 || meas < 0 || meas > 2) return hipErrorInvalidValue;
	const int nt = Np / 64;
	const dim3 grid(nt * (nt + 1) / 2);
	if (meas == 0) hipLaunchKernelGGL(design_kmat_kernel<0>, grid, dim3(256), 0, s, X, N, Np, d, cst, KH);
	else if (meas == 1) hipLaunchKernelGGL(design_kmat_kernel<1>, grid, dim3(256), 0, s, X, N, Np, d, cst, KH);
	else hipLaunchKernelGGL(design_kmat_kernel<2>, grid, dim3(256), 0, s, X, N, Np, d, cst, KH);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(design_hk_kernel, dim3((Np + 255) / 256, 64), dim3(256), 0, s, prep, N, Np, d, nreg, cst, KH, Hm);
	return hipGetLastError();
}

hipError_t launch_design_kvec(hipStream_t s, const double *X, int N, int Np, int d, const double *cst, double amp, const double *Xq, int mb,
                              int mbp, double *Kq)
{
	if (mb < 1 || mbp < mb || mbp > 65535 || N < 1 || d < 1 || d > GPEMU_MAX_PARAMS) return hipErrorInvalidValue;
	hipLaunchKernelGGL(design_kvec_kernel, dim3((Np + 255) / 256, mbp), dim3(256), 0, s, X, N, Np, d, cst, amp, Xq, mb, Kq);
	return hipGetLastError();
}

template <int MEAS>
static void design_cross_launch(hipStream_t s, dim3 grid, const double *X, int N, int d, const double *Xq, int mb, const double *cst,
                                const double *Am, long lda, const double *Tm, long ldt, double *part, long pstride)
{
	if (d <= 8)
		hipLaunchKernelGGL((design_cross_kernel<8, MEAS>), grid, dim3(256), 0, s, X, N, d, Xq, mb, cst, Am, lda, Tm, ldt, part, pstride);
	else if (d <= 16)
		hipLaunchKernelGGL((design_cross_kernel<16, MEAS>), grid, dim3(256), 0, s, X, N, d, Xq, mb, cst, Am, lda, Tm, ldt, part, pstride);
	else
		hipLaunchKernelGGL((design_cross_kernel<GPEMU_MAX_PARAMS, MEAS>), grid, dim3(256), 0, s, X, N, d, Xq, mb, cst, Am, lda, Tm, ldt, part,
		                   pstride);
}

hipError_t launch_design_cross(hipStream_t s, const double *X, int N, int d, const double *Xq, int mb, const double *cst, int meas,
                               const double *Am, long lda, const double *Tm, long ldt, double *part, long pstride)
{
	if (N < 1 || mb < 1 || pstride < mb || d < 1 || d > GPEMU_MAX_PARAMS || meas < 0 || meas > 2) return hipErrorInvalidValue;
	const dim3 grid((N + 63) / 64, (mb + 63) / 64);
	if (meas == 0) design_cross_launch<0>(s, grid, X, N, d, Xq, mb, cst, Am, lda, Tm, ldt, part, pstride);
	else if (meas == 1) design_cross_launch<1>(s, grid, X, N, d, Xq, mb, cst, Am, lda, Tm, ldt, part, pstride);
	else design_cross_launch<2>(s, grid, X, N, d, Xq, mb, cst, Am, lda, Tm, ldt, part, pstride);
	return hipGetLastError();
}

hipError_t launch_design_finish(hipStream_t s, const double *part, long pstride, int N, const double *V, long ldv, const double *R, long ldr,
                                const double *Tm, long ldt, const double *prepq, const double *Xq, int mb, int Np, int d, int nreg,
                                const double *cst, int meas, const double *Hm, double amp, double kappa, double *gain, double *num, double *var,
                                double *bkeep)
{
	if (mb < 1 || nreg < 1 || nreg > 63 || meas < 0 || meas > 2) return hipErrorInvalidValue;
	const dim3 grid((mb + 3) / 4);
	const int ntc = (N + 63) / 64;
	if (meas == 0)
		hipLaunchKernelGGL(design_finish_kernel<0>, grid, dim3(256), 0, s, part, pstride, ntc, V, ldv, R, ldr, Tm, ldt, prepq, Xq, mb, Np, d, nreg,
		                   cst, Hm, amp, kappa, gain, num, var, bkeep);
	else if (meas == 1)
		hipLaunchKernelGGL(design_finish_kernel<1>, grid, dim3(256), 0, s, part, pstride, ntc, V, ldv, R, ldr, Tm, ldt, prepq, Xq, mb, Np, d, nreg,
		                   cst, Hm, amp, kappa, gain, num, var, bkeep);
	else
		hipLaunchKernelGGL(design_finish_kernel<2>, grid, dim3(256), 0, s, part, pstride, ntc, V, ldv, R, ldr, Tm, ldt, prepq, Xq, mb, Np, d, nreg,
		                   cst, Hm, amp, kappa, gain, num, var, bkeep);
	return hipGetLastError();
}

} // namespace gpemu
