// kernels_calib.hip -- implausibility and calibration likelihood against observations (gpemu.h).
//
// Host part: gpemu_calib_project, the once-per-observation-set arithmetic in fp64 (no device), and the layout of the device
// table it feeds.  Device part: the evaluation kernel (one lane owns one query: an r x r Cholesky in registers for the joint
// statistics, the per-output implausibilities from table rows streamed through LDS), the three launches of the selection
// (per-workgroup counts, their scan, the ordered scatter: no atomics, a call repeated returns the same bits) and the gradient
// of chi2 and logpdf with respect to the query's coordinates (the same Cholesky per lane, then the workgroup's
// lanes over the flat tile of outputs).
#include "gpemu_internal.hpp"

#include <cmath>
#include <cfloat>

namespace gpemu {

// ---------------------------------------------------------------------------
// the device table of one observation set, R = nr rounded up to 4 (the kernel's instantiation):
//   [0, 4)                    c_perp, log|S| + log|G| + nt log 2 pi, spare, spare
//   [4, 4 + R)                m_hat, 0 beyond nr
//   [4 + R, .. + R (R+1) / 2) lower triangle of Sigma_z by rows, the identity beyond nr
//   then nt rows of 4 + 2 R:  ybar_t, z_t, S_tt, rel_t, A_t0 .. (0 beyond nr), A_t0^2 ..
// ---------------------------------------------------------------------------
int calib_pad(int nr) { return (nr + 3) / 4 * 4; }
size_t calib_row_elems(int R) { return (size_t)(4 + 2 * R); }
size_t calib_head_elems(int R) { return (size_t)(4 + R + R * (R + 1) / 2); }
size_t calib_table_elems(int nt, int nr)
{
	const int R = calib_pad(nr);
	return calib_head_elems(R) + (size_t)nt * calib_row_elems(R);
}

void calib_fill_table(int nt, int nr, const double *ybar, const double *A, const double *z, const double *sdiag, const double *rel,
                      const double *mhat, const double *sigz, const double *consts, double *tab)
{
	const int R = calib_pad(nr);
	tab[0] = consts[0];
	tab[1] = consts[1] + consts[2] + (double)nt * 1.8378770664093454835606594728112;   // log 2 pi
	tab[2] = 0.0; tab[3] = 0.0;
	double *mh = tab + 4, *sg = mh + R, *rows = tab + calib_head_elems(R);
	for (int c = 0; c < R; c++) mh[c] = c < nr ? mhat[c] : 0.0;
	for (int i = 0, k = 0; i < R; i++)
		for (int j = 0; j <= i; j++, k++) sg[k] = (i < nr) ? sigz[(size_t)i * nr + j] : (i == j ? 1.0 : 0.0);
	for (int t = 0; t < nt; t++) {
		double *r = rows + (size_t)t * calib_row_elems(R);
		r[0] = ybar[t]; r[1] = z[t]; r[2] = sdiag[t]; r[3] = rel ? rel[t] : 0.0;
		for (int c = 0; c < R; c++) {
			const double a = c < nr ? A[(size_t)t * nr + c] : 0.0;
			r[4 + c] = a;
			r[4 + R + c] = a * a;
		}
	}
}

// lower Cholesky in place (row-major, leading dimension n, the lower triangle read and written); a pivot that is not above
// 64 eps times its own diagonal element counts as not positive: returns its 1-based index, 0 when factored
static int host_cholesky(double *a, int n, double *logdet)
{
	double ld = 0.0;
	for (int j = 0; j < n; j++) {
		const double ajj = a[(size_t)j * n + j];
		double p = ajj;
		for (int k = 0; k < j; k++) p -= a[(size_t)j * n + k] * a[(size_t)j * n + k];
		if (!(p > 64.0 * DBL_EPSILON * fabs(ajj)) || !std::isfinite(p)) return j + 1;
		const double d = sqrt(p);
		a[(size_t)j * n + j] = d;
		ld += log(p);
		for (int i = j + 1; i < n; i++) {
			double s = a[(size_t)i * n + j];
			for (int k = 0; k < j; k++) s -= a[(size_t)i * n + k] * a[(size_t)j * n + k];
			a[(size_t)i * n + j] = s / d;
		}
	}
	*logdet = ld;
	return 0;
}

static bool all_finite(const double *p, size_t n)
{
	for (size_t i = 0; i < n; i++)
		if (!std::isfinite(p[i])) return false;
	return true;
}

} // namespace gpemu

using namespace gpemu;

extern "C" int gpemu_calib_project(int nt, int nr, const double *ybar, const double *A, const double *z, const double *S,
                                   const double *sd, double *mhat, double *sigz, double *consts, int *info)
{
	if (info) *info = 0;
	if (!ybar || !A || !z || !mhat || !sigz || !consts || !info) return GPEMU_ERR_ARG;
	if ((S == nullptr) == (sd == nullptr)) return GPEMU_ERR_ARG;
	if (nt < 1 || nt > GPEMU_CALIB_MAX_NT || nr < 1 || nr > GPEMU_CALIB_MAX_R || nr > nt) return GPEMU_ERR_ARG;
	if (!all_finite(ybar, nt) || !all_finite(z, nt) || !all_finite(A, (size_t)nt * nr)) return GPEMU_ERR_ARG;
	if (S && !all_finite(S, (size_t)nt * nt)) return GPEMU_ERR_ARG;
	if (sd) {
		if (!all_finite(sd, nt)) return GPEMU_ERR_ARG;
		for (int t = 0; t < nt; t++)
			if (!(sd[t] > 0.0)) return GPEMU_ERR_ARG;
	}
	for (int c = 0; c < nr; c++) mhat[c] = NAN;
	for (int k = 0; k < nr * nr; k++) sigz[k] = NAN;
	consts[0] = consts[1] = consts[2] = NAN;

	// B = L_S^-1 A and w = L_S^-1 (z - ybar): S = L_S L_S^T, or L_S = diag(sd)
	std::vector<double> B((size_t)nt * nr), w(nt);
	double logS = 0.0;
	if (S) {
		std::vector<double> L(S, S + (size_t)nt * nt);
		const int piv = host_cholesky(L.data(), nt, &logS);
		if (piv) { *info = piv; return GPEMU_ERR_NOT_PD; }
		for (int t = 0; t < nt; t++) {
			const double *lt = L.data() + (size_t)t * nt;
			for (int c = 0; c < nr; c++) {
				double s = A[(size_t)t * nr + c];
				for (int k = 0; k < t; k++) s -= lt[k] * B[(size_t)k * nr + c];
				B[(size_t)t * nr + c] = s / lt[t];
			}
			double s = z[t] - ybar[t];
			for (int k = 0; k < t; k++) s -= lt[k] * w[k];
			w[t] = s / lt[t];
		}
	} else {
		for (int t = 0; t < nt; t++) {
			for (int c = 0; c < nr; c++) B[(size_t)t * nr + c] = A[(size_t)t * nr + c] / sd[t];
			w[t] = (z[t] - ybar[t]) / sd[t];
			logS += 2.0 * log(sd[t]);
		}
	}
	// G = B^T B = L_G L_G^T
	std::vector<double> G((size_t)nr * nr), b(nr);
	for (int i = 0; i < nr; i++) {
		for (int j = 0; j <= i; j++) {
			double s = 0.0;
			for (int t = 0; t < nt; t++) s += B[(size_t)t * nr + i] * B[(size_t)t * nr + j];
			G[(size_t)i * nr + j] = s;
		}
		double s = 0.0;
		for (int t = 0; t < nt; t++) s += B[(size_t)t * nr + i] * w[t];
		b[i] = s;
	}
	double logG = 0.0;
	const int piv = host_cholesky(G.data(), nr, &logG);
	if (piv) { *info = piv; return GPEMU_ERR_NOT_PD; }
	// m_hat = G^-1 B^T w
	std::vector<double> y(nr);
	for (int i = 0; i < nr; i++) {
		double s = b[i];
		for (int k = 0; k < i; k++) s -= G[(size_t)i * nr + k] * y[k];
		y[i] = s / G[(size_t)i * nr + i];
	}
	for (int i = nr - 1; i >= 0; i--) {
		double s = y[i];
		for (int k = i + 1; k < nr; k++) s -= G[(size_t)k * nr + i] * mhat[k];
		mhat[i] = s / G[(size_t)i * nr + i];
	}
	// Sigma_z = G^-1 = L_G^-T L_G^-1: the inverse factor by columns, then the lower triangle, mirrored
	std::vector<double> Li((size_t)nr * nr, 0.0);
	for (int j = 0; j < nr; j++)
		for (int i = j; i < nr; i++) {
			double s = (i == j) ? 1.0 : 0.0;
			for (int k = j; k < i; k++) s -= G[(size_t)i * nr + k] * Li[(size_t)k * nr + j];
			Li[(size_t)i * nr + j] = s / G[(size_t)i * nr + i];
		}
	for (int i = 0; i < nr; i++)
		for (int j = 0; j <= i; j++) {
			double s = 0.0;
			for (int k = i; k < nr; k++) s += Li[(size_t)k * nr + i] * Li[(size_t)k * nr + j];
			sigz[(size_t)i * nr + j] = s;
			sigz[(size_t)j * nr + i] = s;
		}
	// c_perp = |w - B m_hat|^2
	double cp = 0.0;
	for (int t = 0; t < nt; t++) {
		double s = w[t];
		for (int c = 0; c < nr; c++) s -= B[(size_t)t * nr + c] * mhat[c];
		cp += s * s;
	}
	consts[0] = cp; consts[1] = logS; consts[2] = logG;
	return GPEMU_OK;
}

namespace gpemu {

// ---------------------------------------------------------------------------
// evaluation: one lane, one query.  R: nr rounded up to 4 (T padded with the identity, delta with 0: exact zeros in both
// sums), every index static.  The table's head is read at wave-uniform addresses; its per-output rows go through LDS in chunks
// of CALIB_CHUNK outputs, every lane of a wave reading the same address (a broadcast).
// ---------------------------------------------------------------------------
constexpr int CALIB_CHUNK = 64;

template <int R, int BLOCK>
__global__ __launch_bounds__(BLOCK) void calib_eval_kernel(const double *__restrict__ tab, int nt, int nr, int M,
                                                           const double *__restrict__ mean, const double *__restrict__ var, long ld,
                                                           double *__restrict__ stat, int *__restrict__ worst)
{
	constexpr int ROW = 4 + 2 * R;
	__shared__ double rows[CALIB_CHUNK * ROW];
	const long q = (long)blockIdx.x * BLOCK + threadIdx.x;
	const bool live = q < M;
	const long qq = live ? q : (long)M - 1;     // a lane beyond M repeats the last query (it takes part in the staging and stores nothing)
	const double *mh = tab + 4, *sg = tab + 4 + R;

	double m[R], v[R];
#pragma unroll
	for (int c = 0; c < R; c++) {
		m[c] = 0.0; v[c] = 0.0;
		if (c < nr) {
			m[c] = mean[(long)c * ld + qq];
			const double x = var[(long)c * ld + qq];
			v[c] = x < 0.0 ? 0.0 : x;         // (keeps a NaN)
		}
	}

	// ---- joint part: T = Sigma_z + D = L L^T, y = L^-1 delta, chi2 = c_perp + |y|^2, log|T| = sum log pivots
	double chi2, logpdf;
	{
		double T[R * (R + 1) / 2], y[R];
#pragma unroll
		for (int i = 0, k = 0; i < R; i++) {
#pragma unroll
			for (int j = 0; j <= i; j++, k++) T[k] = sg[k] + (i == j ? v[i] : 0.0);
			y[i] = m[i] - mh[i];
		}
		double quad = 0.0, logT = 0.0;
		bool bad = false;
#pragma unroll
		for (int j = 0; j < R; j++) {
			const int jj = j * (j + 1) / 2;
			double p = T[jj + j], yj = y[j];
#pragma unroll
			for (int k = 0; k < j; k++) {
				p -= T[jj + k] * T[jj + k];
				yj -= T[jj + k] * y[k];
			}
			bad = bad || !(p > 0.0);
			const double inv = 1.0 / sqrt(p);
			logT += log(p);
			yj *= inv;
			y[j] = yj;
			quad += yj * yj;
#pragma unroll
			for (int i = j + 1; i < R; i++) {
				const int ii = i * (i + 1) / 2;
				double s = T[ii + j];
#pragma unroll
				for (int k = 0; k < j; k++) s -= T[ii + k] * T[jj + k];
				T[ii + j] = s * inv;
			}
		}
		chi2 = tab[0] + quad;
		logpdf = -0.5 * (chi2 + (tab[1] + logT));
		if (bad) { chi2 = NAN; logpdf = NAN; }
	}

	// ---- per-output part: I_t = |z_t - y_t| / sqrt(sum_c A_tc^2 v_c + S_tt + (rel_t y_t)^2), the running top three
	double i1 = -1.0, i2 = -1.0, i3 = -1.0;
	int w = 0;
	bool nan = false;
	const double *trows = tab + 4 + R + R * (R + 1) / 2;
	for (int t0 = 0; t0 < nt; t0 += CALIB_CHUNK) {
		const int tc = min(CALIB_CHUNK, nt - t0);
		__syncthreads();
		for (int e = threadIdx.x; e < tc * ROW; e += BLOCK) rows[e] = trows[(long)t0 * ROW + e];
		__syncthreads();
		for (int t = 0; t < tc; t++) {
			const double *r = rows + t * ROW;
			double yt = 0.0, den = 0.0;
#pragma unroll
			for (int c = 0; c < R; c++) {
				yt += r[4 + c] * m[c];
				den += r[4 + R + c] * v[c];
			}
			yt = r[0] + yt;
			const double ry = r[3] * yt;
			den = den + r[2] + ry * ry;
			const double I = fabs(r[1] - yt) / sqrt(den);
			nan = nan || (I != I);
			if (I > i1) { i3 = i2; i2 = i1; i1 = I; w = t0 + t; }
			else if (I > i2) { i3 = i2; i2 = I; }
			else if (I > i3) i3 = I;
		}
	}
	if (live) {
		stat[q] = chi2;
		stat[(long)M + q] = logpdf;
		stat[2L * M + q] = nan ? NAN : (i1 < 0.0 ? 0.0 : i1);
		stat[3L * M + q] = nan ? NAN : (i2 < 0.0 ? 0.0 : i2);
		stat[4L * M + q] = nan ? NAN : (i3 < 0.0 ? 0.0 : i3);
		worst[q] = nan ? -1 : w;
	}
}

hipError_t launch_calib_eval(hipStream_t s, const double *tab, int nt, int nr, int M, const double *mean, const double *var, long ld,
                             double *stat, int *worst)
{
	const int R = calib_pad(nr);
	if (R == 4)
		hipLaunchKernelGGL((calib_eval_kernel<4, 256>), dim3((M + 255) / 256), dim3(256), 0, s, tab, nt, nr, M, mean, var, ld, stat, worst);
	else if (R == 8)
		hipLaunchKernelGGL((calib_eval_kernel<8, 256>), dim3((M + 255) / 256), dim3(256), 0, s, tab, nt, nr, M, mean, var, ld, stat, worst);
	else if (R == 12)
		hipLaunchKernelGGL((calib_eval_kernel<12, 64>), dim3((M + 63) / 64), dim3(64), 0, s, tab, nt, nr, M, mean, var, ld, stat, worst);
	else if (R == 16)
		hipLaunchKernelGGL((calib_eval_kernel<16, 64>), dim3((M + 63) / 64), dim3(64), 0, s, tab, nt, nr, M, mean, var, ld, stat, worst);
	else
		return hipErrorInvalidValue;
	return hipGetLastError();
}

// ---------------------------------------------------------------------------
// gradient of chi2 and logpdf with respect to the query's coordinates.  With u = T^-1 delta and
// tau_c = (T^-1)_cc:   d chi2 / dx_j = 2 sum_c u_c dm_c/dx_j - sum_c u_c^2 dv_c/dx_j,
//                      d logpdf / dx_j = - sum_c u_c dm_c/dx_j + 1/2 sum_c (u_c^2 - tau_c) dv_c/dx_j.
// Phase 1, one lane one query: the Cholesky of calib_eval_kernel with the inverse pivots kept on the diagonal, u by the
// forward and the back solve, tau_c as the squared norm of column c of L^-1, one column at a time (R registers, never L^-1
// whole).  Two weights per component go to LDS, [c][lane]: u_c and tau_c; tau_c = -1 (it is > 0 otherwise) marks a variance
// below 0, whose dv_c has weight 0 in both sums; a NaN input or a pivot <= 0 makes all of the point's weights NaN.
// Phase 2, the workgroup's lanes over the flat tile of its queries' nq * d outputs: element e is query e / d, coordinate e % d,
// at offset q0 * d + e in every component's block and in both outputs: unit stride across the wave for any d.  The sums over
// c run in index order from 0.0 and are the same instructions whichever outputs are asked for; components >= nr are not read.
// ---------------------------------------------------------------------------
template <int R, int BLOCK>
__global__ __launch_bounds__(BLOCK) void calib_grad_kernel(const double *__restrict__ tab, int nr, int M, int d,
                                                           const double *__restrict__ mean, const double *__restrict__ var, long ld,
                                                           const double *__restrict__ gmean, const double *__restrict__ gvar, long ldg,
                                                           double *__restrict__ gchi2, double *__restrict__ glogpdf)
{
	__shared__ double wu[R * BLOCK], wt[R * BLOCK];
	const long q0 = (long)blockIdx.x * BLOCK;
	const long q = q0 + threadIdx.x;
	const long qq = q < M ? q : (long)M - 1;     // a lane beyond M repeats the last query; nothing reads its weights
	const double *mh = tab + 4, *sg = tab + 4 + R;
	{
		double T[R * (R + 1) / 2], y[R];
		unsigned neg = 0;
		bool bad = false;
#pragma unroll
		for (int i = 0, k = 0; i < R; i++) {
			double m = 0.0, v = 0.0;
			if (i < nr) {
				m = mean[(long)i * ld + qq];
				const double x = var[(long)i * ld + qq];
				if (x < 0.0) neg |= 1u << i;
				v = x < 0.0 ? 0.0 : x;            // (keeps a NaN)
			}
			bad = bad || (m != m) || (v != v);
#pragma unroll
			for (int j = 0; j <= i; j++, k++) T[k] = sg[k] + (i == j ? v : 0.0);
			y[i] = m - mh[i];
		}
		// T = L L^T in place, 1 / L_jj on the diagonal; y = L^-1 delta
#pragma unroll
		for (int j = 0; j < R; j++) {
			const int jj = j * (j + 1) / 2;
			double p = T[jj + j], yj = y[j];
#pragma unroll
			for (int k = 0; k < j; k++) {
				p -= T[jj + k] * T[jj + k];
				yj -= T[jj + k] * y[k];
			}
			bad = bad || !(p > 0.0);
			const double inv = 1.0 / sqrt(p);
			T[jj + j] = inv;
			y[j] = yj * inv;
#pragma unroll
			for (int i = j + 1; i < R; i++) {
				const int ii = i * (i + 1) / 2;
				double s = T[ii + j];
#pragma unroll
				for (int k = 0; k < j; k++) s -= T[ii + k] * T[jj + k];
				T[ii + j] = s * inv;
			}
		}
		// u = L^-T y, in place
#pragma unroll
		for (int i = R - 1; i >= 0; i--) {
			double s = y[i];
#pragma unroll
			for (int k = i + 1; k < R; k++) s -= T[k * (k + 1) / 2 + i] * y[k];
			y[i] = s * T[i * (i + 1) / 2 + i];
		}
		// tau_c = |column c of L^-1|^2: x_c = 1 / L_cc, x_i = -(sum_{c <= k < i} L_ik x_k) / L_ii
#pragma unroll
		for (int c = 0; c < R; c++) {
			double x[R];
			x[c] = T[c * (c + 1) / 2 + c];
			double tau = x[c] * x[c];
#pragma unroll
			for (int i = c + 1; i < R; i++) {
				const int ii = i * (i + 1) / 2;
				double s = 0.0;
#pragma unroll
				for (int k = c; k < i; k++) s -= T[ii + k] * x[k];
				x[i] = s * T[ii + i];
				tau += x[i] * x[i];
			}
			if ((neg >> c) & 1u) tau = -1.0;
			wu[c * BLOCK + threadIdx.x] = bad ? NAN : y[c];
			wt[c * BLOCK + threadIdx.x] = bad ? NAN : tau;
		}
	}
	__syncthreads();
	const long rest = (long)M - q0;
	const int nq = rest < BLOCK ? (int)rest : BLOCK;
	const long base = q0 * d;
	for (int e = threadIdx.x; e < nq * d; e += BLOCK) {        // nq * d <= 256 * d: inside an int for every d the library takes
		const int ql = e / d;
		double sm = 0.0, s2 = 0.0, sb = 0.0;
#pragma unroll
		for (int c = 0; c < R; c++)
			if (c < nr) {
				const double u = wu[c * BLOCK + ql], tau = wt[c * BLOCK + ql];
				const double gm = gmean[(long)c * ldg + base + e], gv = gvar[(long)c * ldg + base + e];
				const double u2 = u * u;
				const bool off = tau < 0.0;
				sm += u * gm;
				s2 += (off ? 0.0 : u2) * gv;
				sb += (off ? 0.0 : u2 - tau) * gv;
			}
		if (gchi2) gchi2[base + e] = 2.0 * sm - s2;
		if (glogpdf) glogpdf[base + e] = 0.5 * sb - sm;
	}
}

hipError_t launch_calib_grad(hipStream_t s, const double *tab, int nr, int M, int d, const double *mean, const double *var, long ld,
                             const double *gmean, const double *gvar, long ldg, double *gchi2, double *glogpdf)
{
	const int R = calib_pad(nr);
	if (R == 4)
		hipLaunchKernelGGL((calib_grad_kernel<4, 256>), dim3((M + 255) / 256), dim3(256), 0, s, tab, nr, M, d, mean, var, ld, gmean, gvar, ldg, gchi2, glogpdf);
	else if (R == 8)
		hipLaunchKernelGGL((calib_grad_kernel<8, 256>), dim3((M + 255) / 256), dim3(256), 0, s, tab, nr, M, d, mean, var, ld, gmean, gvar, ldg, gchi2, glogpdf);
	else if (R == 12)
		hipLaunchKernelGGL((calib_grad_kernel<12, 64>), dim3((M + 63) / 64), dim3(64), 0, s, tab, nr, M, d, mean, var, ld, gmean, gvar, ldg, gchi2, glogpdf);
	else if (R == 16)
		hipLaunchKernelGGL((calib_grad_kernel<16, 64>), dim3((M + 63) / 64), dim3(64), 0, s, tab, nr, M, d, mean, var, ld, gmean, gvar, ldg, gchi2, glogpdf);
	else
		return hipErrorInvalidValue;
	return hipGetLastError();
}

// ---------------------------------------------------------------------------
// selection: point q is kept iff chi2 <= cut_chi2 and the level-th largest implausibility <= cut_I (a NaN fails both).
// A workgroup owns CALIB_SEL_ITEMS consecutive points.  count: how many it keeps; scan: the exclusive prefix sums of the
// counts in workgroup order by ONE workgroup, and the total; scatter: the kept q at prefix + rank inside the workgroup, the
// rank from the lanes' ballot and the waves' counts in order.  No atomics: an output position depends on the data alone.
// ---------------------------------------------------------------------------
constexpr int CALIB_SEL_BLOCK = 256, CALIB_SEL_ROUNDS = 4, CALIB_SEL_ITEMS = CALIB_SEL_BLOCK * CALIB_SEL_ROUNDS;

__device__ inline bool calib_keep(const double *stat, long M, long q, double cut_chi2, int level, double cut_I)
{
	return q < M && stat[q] <= cut_chi2 && stat[(long)(1 + level) * M + q] <= cut_I;
}

// the rank of a kept lane among the kept lanes of its workgroup in this round (lanes in order), and the round's count
__device__ inline int calib_block_rank(bool keep, int *wave_cnt, int *total)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const unsigned long long b = __ballot(keep);
	__syncthreads();
	if (lane == 0) wave_cnt[wave] = __popcll(b);
	__syncthreads();
	int before = 0, all = 0;
#pragma unroll
	for (int k = 0; k < CALIB_SEL_BLOCK / 64; k++) {
		const int c = wave_cnt[k];
		before += k < wave ? c : 0;
		all += c;
	}
	*total = all;
	return before + __popcll(b & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(CALIB_SEL_BLOCK) void calib_count_kernel(const double *__restrict__ stat, long M, double cut_chi2, int level,
                                                                      double cut_I, int *__restrict__ counts)
{
	__shared__ int wave_cnt[CALIB_SEL_BLOCK / 64];
	int n = 0;
	for (int r = 0; r < CALIB_SEL_ROUNDS; r++) {
		const long q = (long)blockIdx.x * CALIB_SEL_ITEMS + r * CALIB_SEL_BLOCK + threadIdx.x;
		int tot;
		calib_block_rank(calib_keep(stat, M, q, cut_chi2, level, cut_I), wave_cnt, &tot);
		n += tot;
	}
	if (threadIdx.x == 0) counts[blockIdx.x] = n;
}

// counts[b] becomes the number kept by the workgroups before b; counts[nblocks] the total
__global__ __launch_bounds__(CALIB_SEL_BLOCK) void calib_scan_kernel(int *__restrict__ counts, int nblocks)
{
	__shared__ int wave_sum[CALIB_SEL_BLOCK / 64];
	__shared__ int carry_s;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	if (threadIdx.x == 0) carry_s = 0;
	__syncthreads();
	for (int b0 = 0; b0 < nblocks; b0 += CALIB_SEL_BLOCK) {
		const int b = b0 + threadIdx.x;
		const int c = b < nblocks ? counts[b] : 0;
		int incl = c;                                   // inclusive scan inside the wave
#pragma unroll
		for (int o = 1; o < 64; o <<= 1) {
			const int up = __shfl_up(incl, o, 64);
			if (lane >= o) incl += up;
		}
		if (lane == 63) wave_sum[wave] = incl;
		__syncthreads();
		int before = carry_s, all = 0;
#pragma unroll
		for (int k = 0; k < CALIB_SEL_BLOCK / 64; k++) {
			before += k < wave ? wave_sum[k] : 0;
			all += wave_sum[k];
		}
		if (b < nblocks) counts[b] = before + incl - c;
		__syncthreads();
		if (threadIdx.x == 0) carry_s += all;
		__syncthreads();
	}
	if (threadIdx.x == 0) counts[nblocks] = carry_s;
}

__global__ __launch_bounds__(CALIB_SEL_BLOCK) void calib_scatter_kernel(const double *__restrict__ stat, long M, double cut_chi2, int level,
                                                                        double cut_I, const int *__restrict__ offsets, int *__restrict__ idx)
{
	__shared__ int wave_cnt[CALIB_SEL_BLOCK / 64];
	long pos = offsets[blockIdx.x];
	for (int r = 0; r < CALIB_SEL_ROUNDS; r++) {
		const long q = (long)blockIdx.x * CALIB_SEL_ITEMS + r * CALIB_SEL_BLOCK + threadIdx.x;
		const bool keep = calib_keep(stat, M, q, cut_chi2, level, cut_I);
		int tot;
		const int rank = calib_block_rank(keep, wave_cnt, &tot);
		if (keep) idx[pos + rank] = (int)q;      // pos + rank < the total kept <= M: inside idx
		pos += tot;
	}
}

// the kept points' statistics, point-major: out[k * 5 + s] = stat[s][idx[k]], wout[k] = worst[idx[k]] (wout may be null)
__global__ __launch_bounds__(256) void calib_gather_kernel(const double *__restrict__ stat, const int *__restrict__ worst, long M, int count,
                                                           const int *__restrict__ idx, double *__restrict__ out, int *__restrict__ wout)
{
	const int k = blockIdx.x * 256 + threadIdx.x;
	if (k >= count) return;
	const long q = idx[k];
	if (q < 0 || q >= M) return;                  // (idx comes from the selection: always inside; a caller's own list must not read outside)
#pragma unroll
	for (int s = 0; s < 5; s++) out[(long)k * 5 + s] = stat[s * M + q];
	if (wout) wout[k] = worst[q];
}

hipError_t launch_calib_gather(hipStream_t s, const double *stat, const int *worst, int M, int count, const int *idx, double *out, int *wout)
{
	hipLaunchKernelGGL(calib_gather_kernel, dim3((count + 255) / 256), dim3(256), 0, s, stat, worst, (long)M, count, idx, out, wout);
	return hipGetLastError();
}

int calib_select_blocks(int M) { return (M + CALIB_SEL_ITEMS - 1) / CALIB_SEL_ITEMS; }

// counts: calib_select_blocks(M) + 1 ints (the total is left in the last one); idx: M ints
hipError_t launch_calib_select(hipStream_t s, const double *stat, int M, double cut_chi2, int level, double cut_I, int *counts, int *idx)
{
	const int nb = calib_select_blocks(M);
	hipLaunchKernelGGL(calib_count_kernel, dim3(nb), dim3(CALIB_SEL_BLOCK), 0, s, stat, (long)M, cut_chi2, level, cut_I, counts);
	hipLaunchKernelGGL(calib_scan_kernel, dim3(1), dim3(CALIB_SEL_BLOCK), 0, s, counts, nb);
	hipLaunchKernelGGL(calib_scatter_kernel, dim3(nb), dim3(CALIB_SEL_BLOCK), 0, s, stat, (long)M, cut_chi2, level, cut_I, counts, idx);
	return hipGetLastError();
}

} // namespace gpemu
