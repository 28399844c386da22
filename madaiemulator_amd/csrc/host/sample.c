/*
 * sample.c -- posterior samples of the parameters of a multi-output emulator against an observation set (libemu.h;
 * gpemu_calib_sample in gpemu.h): the default starts, the run through device_bridge.c, and the summary of the
 * recorded samples -- mean, standard deviation, quantiles, integrated autocorrelation time.  Host arithmetic only; the chain
 * itself never leaves the device.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "libemu.h"
#include "gpemu.h"

static const char who[] = "emulate_sample_posterior_multi";

/* the records of a run: global steps g = first_step .. first_step + nsteps - 1 with g >= burn and (g + 1) % thin == 0 */
int gpemu_host_sample_nrec(const gpemu_host_sample_args *a)
{
	if (!a || a->nsteps < 1 || a->thin < 1 || a->burn < 0) return 0;
	int n = 0;
	for (int t = 0; t < a->nsteps; t++) {
		const unsigned long long g = a->first_step + (unsigned long long)t;
		n += g >= (unsigned long long)a->burn && (g + 1) % (unsigned long long)a->thin == 0;
	}
	return n;
}

/* the sampler's uniform of two generator words (gpemu.h): ((a << 20 | b >> 12) + 0.5) 2^-52 */
static double uniform_of(unsigned a, unsigned b)
{
	const unsigned long long n = ((unsigned long long)a << 20) | (unsigned long long)(b >> 12);
	return (double)(2 * n + 1) * 0x1p-53;
}

void gpemu_host_sample_starts(unsigned long long seed, int W, int d, const int *kind, const double *lo, const double *hi, double *x0)
{
	const unsigned key[2] = {(unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32)};
	for (int k = 0; k < W; k++)
		for (int j = 0; j < d; j++) {
			const unsigned ctr[4] = {(unsigned)k, (unsigned)j, 0u, 2u};
			unsigned w[4];
			gpemu_philox4x32(ctr, key, w);
			const double u1 = uniform_of(w[0], w[1]), u2 = uniform_of(w[2], w[3]);
			x0[(size_t)k * d + j] = (kind && kind[j]) ? lo[j] + hi[j] * (sqrt(-2.0 * log(u1)) * cos(2.0 * M_PI * u2))
			                                           : lo[j] + u1 * (hi[j] - lo[j]);
		}
}

int gpemu_host_autocorr_time(const double *s, int n, double *tau)
{
	if (tau) *tau = NAN;
	if (!s || !tau || n < 1) return 1;
	double mean = 0.0, c0 = 0.0;
	for (int i = 0; i < n; i++) mean += s[i];
	mean /= n;
	for (int i = 0; i < n; i++) c0 += (s[i] - mean) * (s[i] - mean);
	*tau = 1.0;
	if (n < 2 || !(c0 > 0.0)) return 0;
	for (int M = 1; M < n; M++) {
		double c = 0.0;
		for (int i = 0; i + M < n; i++) c += (s[i] - mean) * (s[i + M] - mean);
		*tau += 2.0 * c / c0;
		if ((double)M >= 5.0 * *tau) break;
	}
	return 0;
}

static int by_value(const void *a, const void *b)
{
	const double x = *(const double *)a, y = *(const double *)b;
	return x < y ? -1 : (x > y);
}

/* the q-quantile of n sorted values, linear between the order statistics around q (n - 1) */
static double quantile_sorted(const double *v, size_t n, double q)
{
	const double pos = q * (double)(n - 1);
	size_t i = (size_t)pos;
	if (i >= n - 1) return v[n - 1];
	const double g = pos - (double)i;
	return v[i] + (v[i + 1] - v[i]) * g;
}

void emulate_sample_posterior_multi(multi_emulator *emu, gpemu_observations *obs, const double *lo, const double *hi, const int *kind,
                                    const gpemu_host_sample_args *args, const double *x0, double *trace_x, double *trace_lp,
                                    double *x_end, double *accept_out, double *summary_out)
{
	if (!emu || !obs || !lo || !hi || !args || !trace_x || !trace_lp) gpemu_host_fatal("%s: a NULL argument\n", who);
	const int d = emu->nparams, W = args->nwalkers;
	if (W < 2 || (W & 1)) gpemu_host_fatal("%s: the number of walkers must be even (it is %d)\n", who, W);
	if (W / 2 < d + 1) gpemu_host_fatal("%s: %d walkers for %d parameters: each half of the walkers needs at least nparams + 1\n", who, W, d);
	if (args->nsteps < 1 || args->burn < 0 || args->thin < 1) gpemu_host_fatal("%s: nsteps >= 1, burn >= 0 and thin >= 1 are needed\n", who);
	if (!(args->a > 1.0) || !isfinite(args->a)) gpemu_host_fatal("%s: the stretch scale must be a finite number > 1\n", who);
	for (int j = 0; j < d; j++) {
		const int g = kind && kind[j];
		if (kind && kind[j] != 0 && kind[j] != 1) gpemu_host_fatal("%s: a prior kind is 0 (uniform) or 1 (Gaussian)\n", who);
		if (!isfinite(lo[j]) || !isfinite(hi[j]) || (g ? !(hi[j] > 0.0) : !(hi[j] > lo[j])))
			gpemu_host_fatal("%s: parameter %d: a uniform prior needs finite lo < hi, a Gaussian one a finite mean and sd > 0\n", who, j);
	}
	const size_t wd = (size_t)W * (size_t)d;
	double *start = (double *)malloc(sizeof(double) * wd), *xe = (double *)malloc(sizeof(double) * wd);
	double *lpe = (double *)malloc(sizeof(double) * (size_t)W);
	int *nacc = (int *)malloc(sizeof(int) * (size_t)W), nrec = 0;
	if (x0) memcpy(start, x0, sizeof(double) * wd);
	else gpemu_host_sample_starts(args->seed, W, d, kind, lo, hi, start);
	gpemu_host_calib_sample(obs, emu->emu_struct_array, emu->nr, d, kind, lo, hi, args, start, trace_x, trace_lp, xe, lpe, nacc, &nrec);
	if (x_end) memcpy(x_end, xe, sizeof(double) * wd);
	if (accept_out) {
		double s = 0.0;
		for (int k = 0; k < W; k++) s += nacc[k];
		*accept_out = s / ((double)W * (double)args->nsteps);
	}
	if (summary_out) {
		const size_t n = (size_t)nrec * (size_t)W;
		double *v = (double *)malloc(sizeof(double) * (n ? n : 1)), *em = (double *)malloc(sizeof(double) * (size_t)(nrec ? nrec : 1));
		for (int j = 0; j < d; j++) {
			double *row = summary_out;
			if (!n) { for (int s = 0; s < 6; s++) row[(size_t)s * d + j] = NAN; continue; }
			double mean = 0.0, ss = 0.0;
			for (size_t i = 0; i < n; i++) { v[i] = trace_x[i * d + j]; mean += v[i]; }
			mean /= (double)n;
			for (size_t i = 0; i < n; i++) ss += (v[i] - mean) * (v[i] - mean);
			for (int t = 0; t < nrec; t++) {
				double m = 0.0;
				for (int k = 0; k < W; k++) m += trace_x[((size_t)t * W + k) * d + j];
				em[t] = m / W;
			}
			qsort(v, n, sizeof(double), by_value);
			row[j] = mean;
			row[(size_t)d + j] = sqrt(ss / (double)n);
			row[2 * (size_t)d + j] = quantile_sorted(v, n, 0.025);
			row[3 * (size_t)d + j] = quantile_sorted(v, n, 0.5);
			row[4 * (size_t)d + j] = quantile_sorted(v, n, 0.975);
			gpemu_host_autocorr_time(em, nrec, &row[5 * (size_t)d + j]);
		}
		free(v); free(em);
	}
	free(start); free(xe); free(lpe); free(nacc);
}
