/* Drives the calibration entries of the host-side libEmu mirror (csrc/host/libemu.h: alloc_observations,
 * emulate_points_multi_implausibility, emulate_points_multi_nonimplausible), for tests/test_host_calib.py.
 *
 *   host_calib_driver MODEL_SNAPSHOT_FILE QUERY_FILE OBS_FILE cut_chi2 level cut_I
 *       OBS_FILE: "full hasrel", then nt values z, then nt standard deviations (full = 0) or nt x nt covariances (full = 1),
 *       then nt relative errors if hasrel.  cut_chi2 / cut_I: a number or "inf".
 *       Lines: "misfit c_perp dof"; "ybar .." and per component "acol .." (ybar and the columns of A as the library's
 *       back-projection holds them); per query "pca_m ..", "pca_v .." (emulate_points_multi in PCA space), "obs_m ..",
 *       "obs_v .." (observable space), "stat chi2 logpdf I1 I2 I3 worst"; "nkeep n" and per kept point "keep idx chi2 logpdf I1
 *       I2 I3"; "same n": how many values of a second call of either entry differ from the first in any bit (0 expected).
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "libemu.h"

static gsl_matrix *read_queries(const char *name, int d)
{
	FILE *in = fopen(name, "r");
	if (!in) return NULL;
	size_t cap = 1024, n = 0;
	double *v = (double *)malloc(sizeof(double) * cap), t;
	while (fscanf(in, "%lf", &t) == 1) {
		if (n == cap) v = (double *)realloc(v, sizeof(double) * (cap *= 2));
		v[n++] = t;
	}
	fclose(in);
	if (n == 0 || n % (size_t)d) return NULL;
	gsl_matrix *q = gsl_matrix_alloc(n / (size_t)d, d);
	for (size_t i = 0; i < n; i++) *gsl_matrix_ptr(q, i / (size_t)d, i % (size_t)d) = v[i];
	free(v);
	return q;
}

static double *vec(size_t n) { return (double *)malloc(sizeof(double) * (n ? n : 1)); }
static int read_vec(FILE *in, double *v, size_t n)
{
	for (size_t i = 0; i < n; i++) if (fscanf(in, "%lf", v + i) != 1) return 0;
	return 1;
}
static double cut_of(const char *s) { return !strcmp(s, "inf") ? INFINITY : atof(s); }
static void print_rows(const char *tag, const double *v, int rows, int n)
{
	for (int i = 0; i < rows; i++) {
		printf("%s", tag);
		for (int j = 0; j < n; j++) printf(" %.17g", v[(size_t)i * n + j]);
		printf("\n");
	}
}

int main(int argc, char **argv)
{
	if (argc != 7) return 2;
	FILE *in = fopen(argv[1], "r");
	if (!in) return 3;
	multi_modelstruct *model = load_multi_modelstruct(in);
	fclose(in);
	const int nt = model->nt, nr = model->nr;
	gsl_matrix *q = read_queries(argv[2], model->nparams);
	if (!q) return 5;
	const int M = (int)q->size1;
	int full = 0, hasrel = 0;
	in = fopen(argv[3], "r");
	if (!in || fscanf(in, "%d %d", &full, &hasrel) != 2) return 6;
	double *z = vec(nt), *s = vec(full ? (size_t)nt * nt : (size_t)nt), *rel = vec(nt);
	if (!read_vec(in, z, nt) || !read_vec(in, s, full ? (size_t)nt * nt : (size_t)nt) || (hasrel && !read_vec(in, rel, nt))) return 7;
	fclose(in);
	const double cut_chi2 = cut_of(argv[4]), cut_I = cut_of(argv[6]);
	const int level = atoi(argv[5]);

	multi_emulator *emu = alloc_multi_emulator(model);
	gpemu_observations *obs = alloc_observations(model, z, full ? NULL : s, full ? s : NULL, hasrel ? rel : NULL);
	double c_perp; int dof;
	gpemu_host_observations_misfit(obs, &c_perp, &dof);
	printf("misfit %.17g %d\n", c_perp, dof);
	{
		/* ybar and A as the library holds them: the back-projection of zeros with the mean, of unit vectors without */
		double *in0 = (double *)calloc((size_t)nr * nr, sizeof(double)), *o = vec((size_t)nr * nt);
		gpemu_host_backproject(model, 0, 1, 1, 1, in0, o);
		print_rows("ybar", o, 1, nt);
		for (int c = 0; c < nr; c++) in0[c * nr + c] = 1.0;
		gpemu_host_backproject(model, 0, 0, (size_t)nr, 1, in0, o);
		print_rows("acol", o, nr, nt);
		free(in0); free(o);
	}

	double *stat = vec((size_t)M * 5), *stat2 = vec((size_t)M * 5), *kst = vec((size_t)M * 5), *kst2 = vec((size_t)M * 5);
	int *worst = (int *)malloc(sizeof(int) * M), *worst2 = (int *)malloc(sizeof(int) * M);
	int *idx = (int *)malloc(sizeof(int) * M), *idx2 = (int *)malloc(sizeof(int) * M), nkeep = -1, nkeep2 = -1;
	emulate_points_multi_implausibility(emu, obs, q, stat, worst);      /* first: before any other path has allocated anything */
	emulate_points_multi_nonimplausible(emu, obs, q, cut_chi2, level, cut_I, idx, kst, &nkeep);

	double *mp = vec((size_t)M * nr), *vp = vec((size_t)M * nr), *mo = vec((size_t)M * nt), *vo = vec((size_t)M * nt);
	emulate_points_multi(emu, q, 1, mp, vp);
	emulate_points_multi(emu, q, 0, mo, vo);
	print_rows("pca_m", mp, M, nr);
	print_rows("pca_v", vp, M, nr);
	print_rows("obs_m", mo, M, nt);
	print_rows("obs_v", vo, M, nt);
	for (int p = 0; p < M; p++)
		printf("stat %.17g %.17g %.17g %.17g %.17g %d\n", stat[p * 5], stat[p * 5 + 1], stat[p * 5 + 2], stat[p * 5 + 3], stat[p * 5 + 4], worst[p]);
	printf("nkeep %d\n", nkeep);
	for (int k = 0; k < nkeep; k++)
		printf("keep %d %.17g %.17g %.17g %.17g %.17g\n", idx[k], kst[k * 5], kst[k * 5 + 1], kst[k * 5 + 2], kst[k * 5 + 3], kst[k * 5 + 4]);

	int bad = 0;
	emulate_points_multi_implausibility(emu, obs, q, stat2, worst2);    /* after the other entries have run: the same bits */
	emulate_points_multi_nonimplausible(emu, obs, q, cut_chi2, level, cut_I, idx2, kst2, &nkeep2);
	bad += memcmp(stat, stat2, sizeof(double) * 5 * M) != 0;
	bad += memcmp(worst, worst2, sizeof(int) * M) != 0;
	bad += nkeep != nkeep2 || memcmp(idx, idx2, sizeof(int) * (nkeep > 0 ? nkeep : 0)) != 0
	       || memcmp(kst, kst2, sizeof(double) * 5 * (nkeep > 0 ? nkeep : 0)) != 0;
	emulate_points_multi_implausibility(emu, obs, q, stat2, NULL);      /* worst may be NULL */
	bad += memcmp(stat, stat2, sizeof(double) * 5 * M) != 0;
	printf("same %d\n", bad);
	free_observations(obs);
	free_multi_emulator(emu);
	return 0;
}
