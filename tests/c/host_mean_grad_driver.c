/* Drives the mean-gradient entries of the host-side libEmu mirror (csrc/host/libemu.h: emulate_points_mean_grad,
 * emulate_points_multi_mean_grad) and prints them beside central differences (h = 1e-5) of the mean-only entries, for
 * tests/test_host_mean_grad.py.
 *
 *   host_mean_grad_driver uni INPUT_MODEL_FILE QUERY_FILE cov_fn order theta_full...
 *       per query one line "uni mean_only mean g_0 .. g_{d-1} c_0 .. c_{d-1}" (g: gradient, c: central differences)
 *   host_mean_grad_driver multi MODEL_SNAPSHOT_FILE QUERY_FILE
 *       per query and space S in {pca, obs} the lines "S_m" (means), "S_g" (gradients, output-major), "S_c" (central
 *       differences in the same order)
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "libemu.h"

#define H 1e-5

static int read_model(const char *name, gsl_matrix **x, gsl_matrix **y)
{
	FILE *in = fopen(name, "r");
	int nt, d, n;
	if (!in || fscanf(in, "%d %d %d", &nt, &d, &n) != 3) return 0;
	*x = gsl_matrix_alloc(n, d);
	*y = gsl_matrix_alloc(n, nt);
	for (int i = 0; i < n; i++) for (int j = 0; j < d; j++) if (fscanf(in, "%lf", gsl_matrix_ptr(*x, i, j)) != 1) return 0;
	for (int i = 0; i < n; i++) for (int j = 0; j < nt; j++) if (fscanf(in, "%lf", gsl_matrix_ptr(*y, i, j)) != 1) return 0;
	fclose(in);
	return 1;
}

/* all numbers of the file, d per row */
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

static gsl_matrix *shifted(const gsl_matrix *q, int j, double h)
{
	gsl_matrix *s = gsl_matrix_alloc(q->size1, q->size2);
	for (size_t i = 0; i < q->size1; i++)
		for (size_t k = 0; k < q->size2; k++) *gsl_matrix_ptr(s, i, k) = gsl_matrix_get(q, i, k) + ((int)k == j ? h : 0.0);
	return s;
}

static int run_uni(int argc, char **argv)
{
	if (argc < 6) return 2;
	gsl_matrix *x, *ymat;
	if (!read_model(argv[2], &x, &ymat)) return 3;
	const int cov = atoi(argv[4]), order = atoi(argv[5]);
	const int N = (int)x->size1, d = (int)x->size2;
	gsl_vector *y = gsl_vector_alloc(x->size1);
	for (int i = 0; i < N; i++) gsl_vector_set(y, i, gsl_matrix_get(ymat, i, 0));
	modelstruct *model = alloc_modelstruct_2(x, y, cov, order);
	const int nthetas = model->options->nthetas;
	if (argc != 6 + nthetas) return 4;
	for (int i = 0; i < nthetas; i++) gsl_vector_set(model->thetas, i, atof(argv[6 + i]));
	gsl_matrix *q = read_queries(argv[3], d);
	if (!q) return 5;
	const int M = (int)q->size1;
	emulator_struct *e = alloc_emulator_struct(model);
	double *mean = (double *)malloc(sizeof(double) * (size_t)M), *only = (double *)malloc(sizeof(double) * (size_t)M);
	double *grad = (double *)malloc(sizeof(double) * (size_t)M * d), *cd = (double *)malloc(sizeof(double) * (size_t)M * d);
	double *mp = (double *)malloc(sizeof(double) * (size_t)M), *mm = (double *)malloc(sizeof(double) * (size_t)M);
	emulate_points_mean_grad(e, q, mean, grad);          /* first: before any other path has allocated anything */
	emulate_points_mean_grad(e, q, NULL, grad);          /* the mean is optional */
	emulate_points_mean(e, q, only);
	for (int j = 0; j < d; j++) {
		gsl_matrix *qp = shifted(q, j, H), *qm = shifted(q, j, -H);
		emulate_points_mean(e, qp, mp);
		emulate_points_mean(e, qm, mm);
		for (int i = 0; i < M; i++) cd[(size_t)i * d + j] = (mp[i] - mm[i]) / (2.0 * H);
		gsl_matrix_free(qp); gsl_matrix_free(qm);
	}
	for (int i = 0; i < M; i++) {
		printf("uni %.17g %.17g", only[i], mean[i]);
		for (int j = 0; j < d; j++) printf(" %.17g", grad[(size_t)i * d + j]);
		for (int j = 0; j < d; j++) printf(" %.17g", cd[(size_t)i * d + j]);
		printf("\n");
	}
	free_emulator_struct(e);
	return 0;
}

static void print_rows(const char *tag, const double *v, int M, int n)
{
	for (int i = 0; i < M; i++) {
		printf("%s", tag);
		for (int j = 0; j < n; j++) printf(" %.17g", v[(size_t)i * n + j]);
		printf("\n");
	}
}

static int run_multi(int argc, char **argv)
{
	if (argc != 4) return 2;
	FILE *in = fopen(argv[2], "r");
	if (!in) return 3;
	multi_modelstruct *model = load_multi_modelstruct(in);
	fclose(in);
	multi_emulator *emu = alloc_multi_emulator(model);
	const int d = model->nparams;
	gsl_matrix *q = read_queries(argv[3], d);
	if (!q) return 5;
	const int M = (int)q->size1;
	for (int pca = 1; pca >= 0; pca--) {
		const int no = pca ? emu->nr : emu->nt;
		double *mean = (double *)malloc(sizeof(double) * (size_t)M * no), *grad = (double *)malloc(sizeof(double) * (size_t)M * no * d);
		double *cd = (double *)malloc(sizeof(double) * (size_t)M * no * d);
		double *mp = (double *)malloc(sizeof(double) * (size_t)M * no), *mm = (double *)malloc(sizeof(double) * (size_t)M * no);
		emulate_points_multi_mean_grad(emu, q, pca, mean, grad);
		for (int j = 0; j < d; j++) {
			gsl_matrix *qp = shifted(q, j, H), *qm = shifted(q, j, -H);
			emulate_points_multi_mean(emu, qp, pca, mp);
			emulate_points_multi_mean(emu, qm, pca, mm);
			for (int i = 0; i < M; i++)
				for (int t = 0; t < no; t++)
					cd[((size_t)i * no + t) * d + j] = (mp[(size_t)i * no + t] - mm[(size_t)i * no + t]) / (2.0 * H);
			gsl_matrix_free(qp); gsl_matrix_free(qm);
		}
		print_rows(pca ? "pca_m" : "obs_m", mean, M, no);
		print_rows(pca ? "pca_g" : "obs_g", grad, M, no * d);
		print_rows(pca ? "pca_c" : "obs_c", cd, M, no * d);
		free(mean); free(grad); free(cd); free(mp); free(mm);
	}
	free_multi_emulator(emu);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc >= 2 && !strcmp(argv[1], "uni")) return run_uni(argc, argv);
	if (argc >= 2 && !strcmp(argv[1], "multi")) return run_multi(argc, argv);
	return 2;
}
