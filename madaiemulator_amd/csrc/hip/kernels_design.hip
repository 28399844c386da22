// kernels_design.hip -- expected reduction of the IMSE by one more run, in closed form (gpemu_design_gain, include/gpemu.h,
// DESIGN.md 4.20).  Conditioning the posterior process on a run at x* is a rank-one update of its covariance, so
//   gain(x*) = E_x[c*(x, x*)^2] / v(x*),   c*(x, x*) = c(x, x*) - k(x)^T a + h(x)^T b,   a = C^-1 k* + W Q r,  b = Q r,
// and the expectation is made of the pair factors II_l of kernels_sens.hip (sens_device.hpp) and its per-point tables:
//   num = A^2 prod_l II_l(x*, x*) - 2 A^2 sum_i a_i w_i + 2 A sum_al b_al HK*_al + A^2 a^T K a - 2 A sum_al b_al (a^T HK_al) + b^T Hm b,
//   K_ii' = prod_l II_l(x_i, x_i'),  w_i = prod_l II_l(x_i, x*),  HK_al,i = E[h_al(x) prod_l k_l(x_il, x_l)],  Hm = E[h h^T].
// K, HK and Hm depend on the design, the lengths and the measure alone: they are built once and kept.  Per block of candidates
// the unclamped k rows, then (in gpemu_api.hip) the prediction's two triangular products for a and T = a [K | HK], then the
// cross sweep for sum_i a_i (T_i - 2 w_i) and the finish.  No atomics, no workgroup waits for another; every sum has one order.
// At the end of the file: the gain over a weighted set of target points (gpemu_design_target_gain), which needs
// no integral in closed form and so serves every covariance function.
#include "gpemu_internal.hpp"
#include "sens_device.hpp"
#include "cov_device.hpp"

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

// ===========================================================================
// Greedy batches of K runs (gpemu_design_batch).  After the first pass above the rows of a, T and b, the
// candidates' tables and num, var stay where they are; the rows of w are written beside them.  Per pick s and context:
//   gather -> column -> update,   then one arg-max launch over the weighted gains of all contexts.
// Per candidate q the state is lambda_q, mu_q (row q of Lam, Mu, ldl wide, entry j written by pick j) and the running
// v_S(q), num_S(q); E (256 x 256, symmetric, both triangles written) is the context's.  The quadratic form is carried forward:
//   lambda^T E lambda grows by 2 lambda_new (e . lambda_old) + E_new,new lambda_new^2,   e_i = E_i,new,
// so a pick costs O(j) per candidate and the first j picks of a longer batch are a batch of j bit for bit.
// ===========================================================================
constexpr int DESIGN_SV_B = 0, DESIGN_SV_H = 64, DESIGN_SV_THK = 128, DESIGN_SV_HKS = 192, DESIGN_SV_HMB = 256, DESIGN_SV_X = 320,
              DESIGN_SV_LAM = 384, DESIGN_SV_E = 640, DESIGN_SV_SC = 896,       // offsets behind the three Np-vectors a_s, w_s, k_s
              DESIGN_SV_ELEMS = 1024;

size_t design_batch_sv_elems(int Np) { return 3 * (size_t)Np + DESIGN_SV_ELEMS; }

// h_al(x): 1, x_l, x_l^2, x_l^3 for al = 1 + (p - 1) d + l, as the prediction's regression row takes it
__device__ __forceinline__ double design_hfun(int a, const double *x, int d)
{
	if (a == 0) return 1.0;
	const int q = (a - 1) / d;
	const double v = x[(a - 1) % d];
	return q == 0 ? v : (q == 1 ? v * v : v * v * v);
}

// HK*_al of candidate q from the block's tables (the expression of design_finish_kernel)
__device__ __forceinline__ double design_hk_own(const double *prepq, int q, int mb, int d, int al)
{
	const long tq = (long)d * mb;
	if (al == 0) return prepq[q] * prepq[4 * tq + q];
	const int l = (al - 1) % d, p = (al - 1) / d + 1;
	return prepq[p * tq + (long)l * mb + q] * prepq[4 * tq + (long)l * mb + q];
}

// wrows: W[q * Np + i] = prod_l II_l(x*_q, x_i), the factor evaluated as the cross sweep evaluates it (candidate first);
// columns i >= N and rows >= mb are 0 (mbp rows: the whole buffer is written)
template <int MEAS>
__global__ __launch_bounds__(256) void design_wrows_kernel(const double *X, int N, int Np, int d, const double *cst, const double *Xq, int mb,
                                                           double *W)
{
	const int col = blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
	if (col >= Np) return;
	W[(long)row * Np + col] = (row < mb && col < N) ? design_pair_product<MEAS>(Xq + (long)row * d, X + (long)col * d, d, cst) : 0.0;
}

// ---------------------------------------------------------------------------
// gather: everything of the pick s = pick[j] that the next two launches read, laid out contiguously in sv:
//   a_s, w_s (rows s of Am and W; a_s zero from N on), k_s fresh and unclamped (design_kvec_kernel's expression), then 64 each
//   of b_s, h_s, T^HK_s, HK*_s, Hm b_s and x_s, lambda_s (j), e (j: the new column of E), and rho, E_new,new, valid.
// Workgroup 0 does the short vectors and extends E: e_i = (mu_s,i - (E lambda_s)_i) / rho, E_jj = num_S(s) / v_S(s).  A pick
// whose v_S rounds to <= 0 carries no information: valid = 0, and its column of E, lambda and mu are 0.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void design_gather_kernel(const int *pick, int j, const double *X, int N, int Np, int d, int nreg,
                                                            const double *cst, double A, const double *Xq, int mb, const double *Am,
                                                            const double *Tm, long ldt, const double *Wm, const double *Bm,
                                                            const double *prepq, const double *Hm, const double *Lam, const double *Mu,
                                                            long ldl, const double *vS, const double *numS, double *E, double *sv)
{
	__shared__ double b_sh[64], lam_sh[256], mu_sh[256];
	const int s = pick[j], tid = threadIdx.x;
	const double *xs = Xq + (long)s * d;
	const int i = blockIdx.x * 256 + tid;
	if (i < Np) {
		double k = 0.0;
		if (i < N) {
			double e = 0.0;
			for (int l = 0; l < d; l++) {
				const double dx = xs[l] - X[(long)i * d + l];
				e = fma(cst[SENS_CST_S * GPEMU_MAX_PARAMS + l] * dx, dx, e);
			}
			k = A * exp(-0.5 * e);
		}
		sv[i] = i < N ? Am[(long)s * Np + i] : 0.0;
		sv[Np + i] = Wm[(long)s * Np + i];
		sv[2 * (long)Np + i] = k;
	}
	if (blockIdx.x != 0) return;
	double *o = sv + 3 * (long)Np;
	if (tid < 64) {
		const bool v = tid < nreg;
		const double b = v ? Bm[(long)s * 64 + tid] : 0.0;
		b_sh[tid] = b;
		o[DESIGN_SV_B + tid] = b;
		o[DESIGN_SV_H + tid] = v ? design_hfun(tid, xs, d) : 0.0;
		o[DESIGN_SV_THK + tid] = v ? Tm[(long)s * ldt + Np + tid] : 0.0;
		o[DESIGN_SV_HKS + tid] = v ? design_hk_own(prepq, s, mb, d, tid) : 0.0;
		o[DESIGN_SV_X + tid] = tid < d ? xs[tid] : 0.0;
	}
	lam_sh[tid] = tid < j ? Lam[(long)s * ldl + tid] : 0.0;
	mu_sh[tid] = tid < j ? Mu[(long)s * ldl + tid] : 0.0;
	__syncthreads();
	if (tid < 64) {
		double t = 0.0;
		if (tid < nreg)
			for (int be = 0; be < nreg; be++) t = fma(Hm[tid * 64 + be], b_sh[be], t);
		o[DESIGN_SV_HMB + tid] = t;
	}
	const double v = vS[s], n = numS[s];
	const bool valid = v > 0.0;
	const double rho = valid ? sqrt(v) : 1.0;
	o[DESIGN_SV_LAM + tid] = lam_sh[tid];
	double e = 0.0;
	if (tid < j && valid) {
		double t = 0.0;
		for (int k = 0; k < j; k++) t = fma(E[(long)k * 256 + tid], lam_sh[k], t);          // (E is symmetric: column tid of row k)
		e = (mu_sh[tid] - t) / rho;
	}
	o[DESIGN_SV_E + tid] = e;
	__syncthreads();                                                                      // every read of E above before its new entries
	if (tid < j) {
		E[(long)tid * 256 + j] = e;
		E[(long)j * 256 + tid] = e;
	}
	if (tid == 0) {
		const double enn = valid ? n / v : 0.0;
		E[(long)j * 256 + j] = enn;
		o[DESIGN_SV_SC + 0] = rho;
		o[DESIGN_SV_SC + 1] = enn;
		o[DESIGN_SV_SC + 2] = valid ? 1.0 : 0.0;
	}
}

// ---------------------------------------------------------------------------
// column: the four N-length dots of every candidate with the pick's vectors,
//   dots[0] = a_q . k_s,  dots[1] = a_q . w_s,  dots[2] = w_q . a_s,  dots[3] = T^K_q . a_s     (dstride apart).
// A workgroup owns 16 candidates, a wave four of them at once: the three rows of a candidate are streamed once, 16 bytes per
// lane (eight lanes a 128-byte row piece), and each piece of the pick's vectors (from the caches: every workgroup reads the
// same 24 Np bytes) serves four rows.  A lane adds its columns in ascending order, then the wave's butterfly: one order.  A
// row past the last candidate repeats the last one and stores nothing.  No LDS, no atomics.  The rows are read unmasked out to
// Np (design_cross_kernel masks col < N): the columns N .. Np - 1 of a, T^K and w meet zeros of the pick's vectors, so they must
// be FINITE -- a's and T^K's come finite out of the products with the zero-padded L^-T and K, w's are written as zeros; the
// cases with N = 1, 63, 65, 130, 200 of the tests would show a NaN.
// ---------------------------------------------------------------------------
constexpr int DESIGN_COL_ROWS = 4;

__global__ __launch_bounds__(256) void design_column_kernel(const double *Am, const double *Tm, long ldt, const double *Wm, int Np, int mb,
                                                            const double *sv, double *dots, long dstride)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int q0 = (blockIdx.x * 4 + wave) * DESIGN_COL_ROWS;
	const double *as = sv, *ws = sv + Np, *ks = sv + 2 * (long)Np;
	const double *ar[DESIGN_COL_ROWS], *tr[DESIGN_COL_ROWS], *wr[DESIGN_COL_ROWS];
	double acc[DESIGN_COL_ROWS][4];
#pragma unroll
	for (int r = 0; r < DESIGN_COL_ROWS; r++) {
		const long q = min(q0 + r, mb - 1);
		ar[r] = Am + q * Np;
		tr[r] = Tm + q * ldt;
		wr[r] = Wm + q * Np;
		acc[r][0] = acc[r][1] = acc[r][2] = acc[r][3] = 0.0;
	}
	for (int i = lane * 2; i < Np; i += 128) {
		const double2 a_s = *reinterpret_cast<const double2 *>(as + i);
		const double2 w_s = *reinterpret_cast<const double2 *>(ws + i);
		const double2 k_s = *reinterpret_cast<const double2 *>(ks + i);
#pragma unroll
		for (int r = 0; r < DESIGN_COL_ROWS; r++) {
			const double2 a = *reinterpret_cast<const double2 *>(ar[r] + i);
			const double2 t = *reinterpret_cast<const double2 *>(tr[r] + i);
			const double2 w = *reinterpret_cast<const double2 *>(wr[r] + i);
			acc[r][0] = fma(a.y, k_s.y, fma(a.x, k_s.x, acc[r][0]));
			acc[r][1] = fma(a.y, w_s.y, fma(a.x, w_s.x, acc[r][1]));
			acc[r][2] = fma(w.y, a_s.y, fma(w.x, a_s.x, acc[r][2]));
			acc[r][3] = fma(t.y, a_s.y, fma(t.x, a_s.x, acc[r][3]));
		}
	}
#pragma unroll
	for (int r = 0; r < DESIGN_COL_ROWS; r++)
#pragma unroll
		for (int k = 0; k < 4; k++) {
			double v = acc[r][k];
#pragma unroll
			for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
			if (lane == 0 && q0 + r < mb) dots[k * dstride + q0 + r] = v;
		}
}

// ---------------------------------------------------------------------------
// update: one wave per candidate q.  Lane al holds b_q, T^HK_q, HK*_q of basis function al and the six short products with the
// pick's vectors; lane l the pair factor II_l(x*_q, x*_s) and the exponent term of coordinate l, multiplied and added by lane
// order; lanes stride over the j entries of lambda_q, mu_q for lambda_q . lambda_s, mu_q . lambda_s and e . lambda_q.  Then
//   Sigma = (A k(x_q, x_s) - a_q . k_s) + b_q . h_s
//   G     = (A^2 (((II - w_q . a_s) - a_q . w_s) + T^K_q . a_s) + A ((HK*_q . b_s + HK*_s . b_q) - (T^HK_q . b_s + b_q . T^HK_s))) + b_q . Hm b_s
//   lambda_new = (Sigma - lambda_q . lambda_s) / rho,   mu_new = (G - mu_q . lambda_s) / rho        (0 for a pick that is not valid)
//   v_S -= lambda_new^2,   num_S += -2 lambda_new mu_new + 2 lambda_new (e . lambda_q) + E_new,new lambda_new^2,
//   gain = v_S > 0 ? num_S / v_S : 0.
// ---------------------------------------------------------------------------
template <int MEAS>
__global__ __launch_bounds__(256) void design_update_kernel(int j, const double *Xq, int mb, int Np, int d, int nreg, const double *cst,
                                                            double A, const double *Tm, long ldt, const double *Bm, const double *prepq,
                                                            const double *sv, const double *dots, long dstride, double *Lam, double *Mu,
                                                            long ldl, double *vS, double *numS, double *gain)
{
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int q = min(blockIdx.x * 4 + wave, mb - 1);
	const bool store = blockIdx.x * 4 + wave < mb;
	const double *o = sv + 3 * (long)Np;
	double pbh = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0, p4 = 0.0, p5 = 0.0;
	if (lane < nreg) {
		const double bq = Bm[(long)q * 64 + lane], thk = Tm[(long)q * ldt + Np + lane], hk = design_hk_own(prepq, q, mb, d, lane);
		const double bs = o[DESIGN_SV_B + lane];
		pbh = bq * o[DESIGN_SV_H + lane];
		p1 = hk * bs;
		p2 = o[DESIGN_SV_HKS + lane] * bq;
		p3 = thk * bs;
		p4 = bq * o[DESIGN_SV_THK + lane];
		p5 = bq * o[DESIGN_SV_HMB + lane];
	}
	double ll = 0.0, ml = 0.0, el = 0.0;
	for (int i = lane; i < j; i += 64) {
		const double lq = Lam[(long)q * ldl + i], ls = o[DESIGN_SV_LAM + i];
		ll = fma(lq, ls, ll);
		ml = fma(Mu[(long)q * ldl + i], ls, ml);
		el = fma(lq, o[DESIGN_SV_E + i], el);
	}
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) {
		pbh += __shfl_xor(pbh, off);
		p1 += __shfl_xor(p1, off);
		p2 += __shfl_xor(p2, off);
		p3 += __shfl_xor(p3, off);
		p4 += __shfl_xor(p4, off);
		p5 += __shfl_xor(p5, off);
		ll += __shfl_xor(ll, off);
		ml += __shfl_xor(ml, off);
		el += __shfl_xor(el, off);
	}
	double f = 1.0, ex = 0.0;
	if (lane < d) {
		const double xa = Xq[(long)q * d + lane], xb = o[DESIGN_SV_X + lane];
		f = sens_pair_factor<MEAS>(xa, xb, cst[0 * GPEMU_MAX_PARAMS + lane], cst[1 * GPEMU_MAX_PARAMS + lane], cst[2 * GPEMU_MAX_PARAMS + lane],
		                           cst[3 * GPEMU_MAX_PARAMS + lane], cst[4 * GPEMU_MAX_PARAMS + lane], cst[5 * GPEMU_MAX_PARAMS + lane],
		                           cst[6 * GPEMU_MAX_PARAMS + lane], MEAS == 2 ? cst[SENS_CST_KIND * GPEMU_MAX_PARAMS + lane] : 0.0);
		const double dx = xa - xb;
		ex = cst[SENS_CST_S * GPEMU_MAX_PARAMS + lane] * dx * dx;
	}
	double pi = 1.0, es = 0.0;
	for (int l = 0; l < d; l++) {
		pi *= __shfl(f, l);
		es += __shfl(ex, l);
	}
	if (!store || lane != 0) return;
	const double rho = o[DESIGN_SV_SC + 0], enn = o[DESIGN_SV_SC + 1];
	const bool valid = o[DESIGN_SV_SC + 2] != 0.0;
	const double d1 = dots[q], d2 = dots[dstride + q], d3 = dots[2 * dstride + q], d4 = dots[3 * dstride + q];
	const double sig = (A * exp(-0.5 * es) - d1) + pbh;
	const double g = (A * A * (((pi - d3) - d2) + d4) + A * ((p1 + p2) - (p3 + p4))) + p5;
	const double ln = valid ? (sig - ll) / rho : 0.0, mn = valid ? (g - ml) / rho : 0.0;
	Lam[(long)q * ldl + j] = ln;
	Mu[(long)q * ldl + j] = mn;
	const double v = vS[q] - ln * ln;
	const double n = numS[q] + ((2.0 * ln * (el - mn)) + enn * ln * ln);
	vS[q] = v;
	numS[q] = n;
	gain[q] = v > 0.0 ? n / v : 0.0;
}

// ---------------------------------------------------------------------------
// argmax: one workgroup over all candidates.  wsum_q = sum_c weight_c gain_c(q) in context order (the first term is the product
// itself: one context with weight 1 keeps the bits of its gain); wout (optional) receives it, -inf for a candidate already
// picked.  slot >= 0: the arg-max over the candidates not yet picked -- a thread over its candidates in ascending order, then
// a fixed tree; a larger value wins, equal values go to the lower index, NaN counts as -inf -- goes to pick[slot], its weighted
// gain to pick_gain[slot], the contexts' to pick_gain_ctx[slot * nctx ..], and the candidate is marked picked.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void design_argmax_kernel(const double *const *gains, const double *weight, int nctx, int M, int *picked,
                                                            int slot, int *pick, double *pick_gain, double *pick_gain_ctx, double *wout)
{
	__shared__ double val_s[256];
	__shared__ int idx_s[256];
	const int tid = threadIdx.x;
	double best = 0.0;
	int bi = -1;
	for (int q = tid; q < M; q += 256) {
		double ws = weight[0] * gains[0][q];
		for (int c = 1; c < nctx; c++) ws = fma(weight[c], gains[c][q], ws);
		const bool taken = picked[q] != 0;
		if (wout) wout[q] = taken ? -INFINITY : ws;
		if (taken) continue;
		const double v = ws != ws ? -INFINITY : ws;
		if (bi < 0 || v > best) {
			best = v;
			bi = q;
		}
	}
	if (slot < 0) return;
	val_s[tid] = best;
	idx_s[tid] = bi;
	__syncthreads();
	for (int off = 128; off > 0; off >>= 1) {
		if (tid < off) {
			const int oi = idx_s[tid + off], mi = idx_s[tid];
			const double ov = val_s[tid + off], mv = val_s[tid];
			if (oi >= 0 && (mi < 0 || ov > mv || (ov == mv && oi < mi))) {
				val_s[tid] = ov;
				idx_s[tid] = oi;
			}
		}
		__syncthreads();
	}
	if (tid == 0) {
		const int s = idx_s[0];                                                       // (>= 0: the entry admits no more picks than candidates)
		pick[slot] = s;
		picked[s] = 1;
		double ws = weight[0] * gains[0][s];
		for (int c = 1; c < nctx; c++) ws = fma(weight[c], gains[c][s], ws);
		pick_gain[slot] = ws;
		if (pick_gain_ctx)
			for (int c = 0; c < nctx; c++) pick_gain_ctx[(long)slot * nctx + c] = gains[c][s];
	}
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
hipError_t launch_design_wrows(hipStream_t s, const double *X, int N, int Np, int d, const double *cst, int meas, const double *Xq, int mb,
                               int mbp, double *W)
{
	if (mb < 1 || mbp < mb || mbp > 65535 || N < 1 || d < 1 || d > GPEMU_MAX_PARAMS || meas < 0 || meas > 2) return hipErrorInvalidValue;
	const dim3 grid((Np + 255) / 256, mbp);
	if (meas == 0) hipLaunchKernelGGL(design_wrows_kernel<0>, grid, dim3(256), 0, s, X, N, Np, d, cst, Xq, mb, W);
	else if (meas == 1) hipLaunchKernelGGL(design_wrows_kernel<1>, grid, dim3(256), 0, s, X, N, Np, d, cst, Xq, mb, W);
	else hipLaunchKernelGGL(design_wrows_kernel<2>, grid, dim3(256), 0, s, X, N, Np, d, cst, Xq, mb, W);
	return hipGetLastError();
}

hipError_t launch_design_gather(hipStream_t s, const int *pick, int j, const double *X, int N, int Np, int d, int nreg, const double *cst,
                                double amp, const double *Xq, int mb, const double *Am, const double *Tm, long ldt, const double *Wm,
                                const double *Bm, const double *prepq, const double *Hm, const double *Lam, const double *Mu, long ldl,
                                const double *vS, const double *numS, double *E, double *sv)
{
	if (j < 0 || j >= 256 || ldl <= j || mb < 1 || Np % 64 || nreg < 1 || nreg > 63 || d < 1 || d > GPEMU_MAX_PARAMS) return hipErrorInvalidValue;
	hipLaunchKernelGGL(design_gather_kernel, dim3((Np + 255) / 256), dim3(256), 0, s, pick, j, X, N, Np, d, nreg, cst, amp, Xq, mb, Am, Tm, ldt,
	                   Wm, Bm, prepq, Hm, Lam, Mu, ldl, vS, numS, E, sv);
	return hipGetLastError();
}

hipError_t launch_design_column(hipStream_t s, const double *Am, const double *Tm, long ldt, const double *Wm, int Np, int mb, const double *sv,
                                double *dots, long dstride)
{
	if (mb < 1 || Np < 64 || Np % 64 || ldt % 2 || dstride < mb) return hipErrorInvalidValue;
	const int per = 4 * DESIGN_COL_ROWS;
	hipLaunchKernelGGL(design_column_kernel, dim3((mb + per - 1) / per), dim3(256), 0, s, Am, Tm, ldt, Wm, Np, mb, sv, dots, dstride);
	return hipGetLastError();
}

hipError_t launch_design_update(hipStream_t s, int j, const double *Xq, int mb, int Np, int d, int nreg, const double *cst, int meas, double amp,
                                const double *Tm, long ldt, const double *Bm, const double *prepq, const double *sv, const double *dots,
                                long dstride, double *Lam, double *Mu, long ldl, double *vS, double *numS, double *gain)
{
	if (j < 0 || j >= 256 || ldl <= j || mb < 1 || nreg < 1 || nreg > 63 || d < 1 || d > GPEMU_MAX_PARAMS || meas < 0 || meas > 2)
		return hipErrorInvalidValue;
	const dim3 grid((mb + 3) / 4);
	if (meas == 0)
		hipLaunchKernelGGL(design_update_kernel<0>, grid, dim3(256), 0, s, j, Xq, mb, Np, d, nreg, cst, amp, Tm, ldt, Bm, prepq, sv, dots, dstride,
		                   Lam, Mu, ldl, vS, numS, gain);
	else if (meas == 1)
		hipLaunchKernelGGL(design_update_kernel<1>, grid, dim3(256), 0, s, j, Xq, mb, Np, d, nreg, cst, amp, Tm, ldt, Bm, prepq, sv, dots, dstride,
		                   Lam, Mu, ldl, vS, numS, gain);
	else
		hipLaunchKernelGGL(design_update_kernel<2>, grid, dim3(256), 0, s, j, Xq, mb, Np, d, nreg, cst, amp, Tm, ldt, Bm, prepq, sv, dots, dstride,
		                   Lam, Mu, ldl, vS, numS, gain);
	return hipGetLastError();
}

hipError_t launch_design_argmax(hipStream_t s, const double *const *gains, const double *weight, int nctx, int M, int *picked, int slot,
                                int *pick, double *pick_gain, double *pick_gain_ctx, double *wout)
{
	if (nctx < 1 || M < 1 || slot >= 256) return hipErrorInvalidValue;
	hipLaunchKernelGGL(design_argmax_kernel, dim3(1), dim3(256), 0, s, gains, weight, nctx, M, picked, slot, pick, pick_gain, pick_gain_ctx,
	                   wout);
	return hipGetLastError();
}

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

// ---------------------------------------------------------------------------
// Gain over a weighted set of target points (gpemu_design_target_gain, include/gpemu.h):
//   num(x*) = sum_s w_s c*(x_s, x*)^2,   c*(x_s, x*) = c(x_s, x*) - u_s . u_* + r_* . (Q r)_s.
// target sweep: one workgroup per tile of 64 candidates (rows, blockIdx.y) x 64 targets (columns, tile blockIdx.x of the
// panel, tile t0 + blockIdx.x of the set).  c is the element of the unclamped fill (cov_tile_values, mode 0, a CovParams whose
// nugget is 0: the bare kernel value wherever the two points lie); P = U_q U_t^T (the panel the GEMM left, row pieces of 64
// consecutive targets: whole 512-byte pieces per wave) is read where the thread holds its elements; r of the 64 candidates
// and Q r of the 64 targets are staged in LDS as predict_cov_prior_kernel stages them.  w_s c*^2 goes into an LDS tile; then
// thread (row = tid / 4, quarter = tid % 4) adds its 16 columns in index order and the four quarters are added in order:
// one partial per candidate and target tile, part[tile of the panel * pstride + q].  Rows >= mb and columns >= S give 0.
// No atomics, no workgroup waits for another.  Dynamic LDS: 2 * 64 * nreg doubles.
// ---------------------------------------------------------------------------
constexpr int TGT_LD = FT + 1;

template <int KIND>
__global__ __launch_bounds__(256) void design_target_sweep_kernel(const double *Xq, int mb, const double *Xt, int S, int t0, int d, CovParams p,
                                                                  const double *P, long ldp, const double *Rq, long ldr, const double *QRt,
                                                                  long ldq, const double *wt, int nreg, double *part, long pstride)
{
	extern __shared__ double tgt_reg_s[];
	__shared__ double c_s[FT * TGT_LD];
	double *r_s = tgt_reg_s;                    // [candidate of the tile][a]
	double *qr_s = tgt_reg_s + FT * nreg;       // [a][target of the tile]
	__builtin_assume(p.kind == KIND);           // (the launch picks the instantiation by p.kind; p stays in the kernel's arguments)
	const int tid = threadIdx.x;
	const int tr = blockIdx.y, tl = blockIdx.x, tc = t0 + tl;
	for (int e = tid; e < FT * nreg; e += 256) {
		const int i = e / nreg, a = e % nreg;
		const int gr = tr * FT + i, gc = tc * FT + i;
		r_s[i * nreg + a] = gr < mb ? Rq[(long)gr * ldr + a] : 0.0;
		qr_s[a * FT + i] = gc < S ? QRt[(long)gc * ldq + 1 + a] : 0.0;
	}
	double v[16];
	cov_tile_values(Xq, mb, Xt, S, d, p, 0, tr, tc, [&](int t, int, int, double c) { v[t] = c; });       // (its barrier also covers the staging above)
	const int cl = tid & 63, rsub = tid >> 6;
	double reg[16];
#pragma unroll
	for (int t = 0; t < 16; t++) reg[t] = 0.0;
	for (int a = 0; a < nreg; a++) {
		const double qr = qr_s[a * FT + cl];
#pragma unroll
		for (int t = 0; t < 16; t++) reg[t] = fma(r_s[(rsub + 4 * t) * nreg + a], qr, reg[t]);
	}
	const int col = tc * FT + cl;
	const bool colv = col < S;
	const double w = colv ? wt[col] : 0.0;
	const double *pcol = P + tl * FT + cl;
#pragma unroll
	for (int t = 0; t < 16; t++) {
		const int row = tr * FT + rsub + 4 * t;
		const double pe = (colv && row < mb) ? pcol[(long)row * ldp] : 0.0;
		const double cs = (v[t] - pe) + reg[t];
		c_s[(rsub + 4 * t) * TGT_LD + cl] = w * (cs * cs);
	}
	__syncthreads();
	const int i = tid >> 2, qd = tid & 3;
	double s = 0.0;
#pragma unroll
	for (int c = 0; c < 16; c++) s += c_s[i * TGT_LD + 16 * qd + c];
	const double s1 = __shfl_down(s, 1), s2 = __shfl_down(s, 2), s3 = __shfl_down(s, 3);
	const int q = tr * FT + i;
	if (qd == 0 && q < mb) part[(long)tl * pstride + q] = ((s + s1) + s2) + s3;
}

// target finish: candidate q adds the partials of a panel in ascending tile order to its running num (started at 0 by the
// first panel), and behind the last panel forms gain = num / var (0 where var rounds to <= 0).  The sum over the targets has
// one order whatever the panel width; the partials of a tile lie side by side over q, so a thread takes a candidate and a
// wave reads whole row pieces.
__global__ __launch_bounds__(256) void design_target_finish_kernel(const double *part, long pstride, int ntile, int mb, int first, int last,
                                                                   const double *var, double *num, double *gain)
{
	const int q = blockIdx.x * 256 + threadIdx.x;
	if (q >= mb) return;
	double s = first ? 0.0 : num[q];
	for (int t = 0; t < ntile; t++) s += part[(long)t * pstride + q];
	num[q] = s;
	if (last) {
		const double v = var[q];
		gain[q] = v > 0.0 ? s / v : 0.0;
	}
}

// target_var = sum_s w_s v(x_s) in one fixed order: thread t of the one workgroup adds s = t, t + 256, ... in index order,
// then the 256 sums are halved eight times through LDS
__global__ __launch_bounds__(256) void design_target_var_kernel(const double *wt, const double *vt, int S, double *out)
{
	__shared__ double red[256];
	double s = 0.0;
	for (int i = threadIdx.x; i < S; i += 256) s += wt[i] * vt[i];
	red[threadIdx.x] = s;
	__syncthreads();
	for (int h = 128; h > 0; h >>= 1) {
		if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
		__syncthreads();
	}
	if (threadIdx.x == 0) out[0] = red[0];
}

hipError_t launch_design_target_sweep(hipStream_t s, const double *Xq, int mb, const double *Xt, int S, int s0, int ns, int d,
                                      const CovParams &p, const double *P, long ldp, const double *Rq, long ldr, const double *QRt, long ldq,
                                      const double *wt, int nreg, double *part, long pstride)
{
	if (mb < 1 || mb > 64 * 65535 || S < 1 || s0 < 0 || s0 % FT || ns < 1 || s0 + ns > S || ldp < ns || pstride < mb || d < 1 || d > GPEMU_MAX_PARAMS ||
	    nreg < 1 || nreg > 63 || ldr < nreg || ldq < nreg + 1)
		return hipErrorInvalidValue;
	const dim3 grid((ns + FT - 1) / FT, (mb + FT - 1) / FT);
	const size_t dyn = 2 * FT * nreg * sizeof(double);
	if (p.kind == GPEMU_POWEREXP)
		hipLaunchKernelGGL(design_target_sweep_kernel<GPEMU_POWEREXP>, grid, dim3(256), dyn, s, Xq, mb, Xt, S, s0 / FT, d, p, P, ldp, Rq, ldr, QRt,
		                   ldq, wt, nreg, part, pstride);
	else if (p.kind == GPEMU_MATERN32)
		hipLaunchKernelGGL(design_target_sweep_kernel<GPEMU_MATERN32>, grid, dim3(256), dyn, s, Xq, mb, Xt, S, s0 / FT, d, p, P, ldp, Rq, ldr, QRt,
		                   ldq, wt, nreg, part, pstride);
	else if (p.kind == GPEMU_MATERN52)
		hipLaunchKernelGGL(design_target_sweep_kernel<GPEMU_MATERN52>, grid, dim3(256), dyn, s, Xq, mb, Xt, S, s0 / FT, d, p, P, ldp, Rq, ldr, QRt,
		                   ldq, wt, nreg, part, pstride);
	else
		return hipErrorInvalidValue;
	return hipGetLastError();
}

hipError_t launch_design_target_finish(hipStream_t s, const double *part, long pstride, int ntile, int mb, bool first, bool last,
                                       const double *var, double *num, double *gain)
{
	if (mb < 1 || ntile < 1 || pstride < mb) return hipErrorInvalidValue;
	hipLaunchKernelGGL(design_target_finish_kernel, dim3((mb + 255) / 256), dim3(256), 0, s, part, pstride, ntile, mb, first ? 1 : 0, last ? 1 : 0,
	                   var, num, gain);
	return hipGetLastError();
}

hipError_t launch_design_target_var(hipStream_t s, const double *wt, const double *vt, int S, double *out)
{
	if (S < 1) return hipErrorInvalidValue;
	hipLaunchKernelGGL(design_target_var_kernel, dim3(1), dim3(256), 0, s, wt, vt, S, out);
	return hipGetLastError();
}

} // namespace gpemu
