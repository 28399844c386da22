/* Drives emulate_points_multi_logpdf_grad of the host-side libEmu mirror (csrc/host/libemu.h), for
 * tests/test_host_calib_grad.py.
 *
 *   host_calib_grad_driver MODEL_SNAPSHOT_FILE QUERY_FILE OBS_FILE FD_QUERY_FILE
 *       OBS_FILE as host_calib_driver reads it.  Lines: "ybar ..", per component "acol .." (as the library's back-projection
 *       holds them); per query "pca_m", "pca_v" (nr values), "pca_gm", "pca_gv" (nr x nparams values, component-major:
 *       emulate_points_multi_grad in PCA space), "stat" (5 values, from the gradient entry), "ref" (5 values, from
 *       emulate_points_multi_implausibility), "glog", "gchi" (nparams values); per point of FD_QUERY_FILE "fd logpdf";
 *       "same n": how many of the repeated or reduced calls differ from the first in any bit (0 expected).
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
	if (argc != 5) return 2;
	FILE *in = fopen(argv[1], "r");
	if (!in) return 3;
	multi_modelstruct *model = load_multi_modelstruct(in);
	fclose(in);
	const int nt = model->nt, nr = model->nr, d = model->nparams;
	gsl_matrix *q = read_queries(argv[2], d), *fq = read_queries(argv[4], d);
	if (!q || !fq) return 5;
	const int M = (int)q->size1, F = (int)fq->size1;
	int full = 0, hasrel = 0;
	in = fopen(argv[3], "r");
	if (!in || fscanf(in, "%d %d", &full, &hasrel) != 2) return 6;
	double *z = vec(nt), *s = vec(full ? (size_t)nt * nt : (size_t)nt), *rel = vec(nt);
	if (!read_vec(in, z, nt) || !read_vec(in, s, full ? (size_t)nt * nt : (size_t)nt) || (hasrel && !read_vec(in, rel, nt))) return 7;
	fclose(in);

	multi_emulator *emu = alloc_multi_emulator(model);
	gpemu_observations *obs = alloc_observations(model, z, full ? NULL : s, full ? s : NULL, hasrel ? rel : NULL);
	{
		double *in0 = (double *)calloc((size_t)nr * nr, sizeof(double)), *o = vec((size_t)nr * nt);
		gpemu_host_backproject(model, 0, 1, 1, 1, in0, o);
		print_rows("ybar", o, 1, nt);
		for (int c = 0; c < nr; c++) in0[c * nr + c] = 1.0;
		gpemu_host_backproject(model, 0, 0, (size_t)nr, 1, in0, o);
		print_rows("acol", o, nr, nt);
		free(in0); free(o);
	}
	const size_t md = (size_t)M * d;
	double *stat = vec((size_t)M * 5), *ref = vec((size_t)M * 5), *gl = vec(md), *gc = vec(md), *gl2 = vec(md), *gc2 = vec(md);
	double *stat2 = vec((size_t)M * 5);
	emulate_points_multi_logpdf_grad(emu, obs, q, stat, gl, gc);        /* first: before any other path has allocated anything */
	emulate_points_multi_implausibility(emu, obs, q, ref, NULL);

	double *mp = vec((size_t)M * nr), *vp = vec((size_t)M * nr), *gm = vec(md * nr), *gv = vec(md * nr);
	emulate_points_multi_grad(emu, q, 1, mp, vp, gm, gv);
	print_rows("pca_m", mp, M, nr);
	print_rows("pca_v", vp, M, nr);
	print_rows("pca_gm", gm, M, nr * d);
	print_rows("pca_gv", gv, M, nr * d);
	print_rows("stat", stat, M, 5);
	print_rows("ref", ref, M, 5);
	print_rows("glog", gl, M, d);
	print_rows("gchi", gc, M, d);

	double *fst = vec((size_t)F * 5);
	emulate_points_multi_implausibility(emu, obs, fq, fst, NULL);
	for (int p = 0; p < F; p++) printf("fd %.17g\n", fst[p * 5 + 1]);

	int bad = 0;
	emulate_points_multi_logpdf_grad(emu, obs, q, stat2, gl2, gc2);     /* after the other entries have run: the same bits */
	bad += memcmp(stat, stat2, sizeof(double) * 5 * M) != 0;
	bad += memcmp(gl, gl2, sizeof(double) * md) != 0;
	bad += memcmp(gc, gc2, sizeof(double) * md) != 0;
	memset(gl2, 0, sizeof(double) * md);
	emulate_points_multi_logpdf_grad(emu, obs, q, NULL, gl2, NULL);     /* stat and the chi2 gradient may be NULL */
	bad += memcmp(gl, gl2, sizeof(double) * md) != 0;
	printf("same %d\n", bad);
	free_observations(obs);
	free_multi_emulator(emu);
	return 0;
}
