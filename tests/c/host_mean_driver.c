/* Drives the mean-only entries of the host-side libEmu mirror (csrc/host/libemu.h: emulate_points_mean,
 * emulate_points_multi_mean) beside the mean+variance ones, and prints both for tests/test_host_mean.py.
 *
 *   host_mean_driver uni INPUT_MODEL_FILE QUERY_FILE cov_fn order theta_full...
 *       one line "uni mean variance mean_only" per query (QUERY_FILE: d numbers per query)
 *   host_mean_driver multi MODEL_SNAPSHOT_FILE QUERY_FILE
 *       per query one line "pca" and one line "obs": per output "mean mean_only"
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "libemu.h"

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

static int run_uni(int argc, char **argv)
{
	if (argc < 6) return 2;
	gsl_matrix *x, *ymat;
	if (!read_model(argv[2], &x, &ymat)) return 3;
	const int cov = atoi(argv[4]), order = atoi(argv[5]);
	const int N = (int)x->size1;
	gsl_vector *y = gsl_vector_alloc(x->size1);
	for (int i = 0; i < N; i++) gsl_vector_set(y, i, gsl_matrix_get(ymat, i, 0));
	modelstruct *model = alloc_modelstruct_2(x, y, cov, order);
	const int nthetas = model->options->nthetas;
	if (argc != 6 + nthetas) return 4;
	for (int i = 0; i < nthetas; i++) gsl_vector_set(model->thetas, i, atof(argv[6 + i]));
	gsl_matrix *q = read_queries(argv[3], (int)x->size2);
	if (!q) return 5;
	const int M = (int)q->size1;
	emulator_struct *e = alloc_emulator_struct(model);
	double *mean = (double *)malloc(sizeof(double) * (size_t)M), *var = (double *)malloc(sizeof(double) * (size_t)M);
	double *only = (double *)malloc(sizeof(double) * (size_t)M);
	emulate_points_mean(e, q, only);                     /* first: before the mean+variance path has allocated anything */
	emulate_points(e, q, mean, var);
	for (int i = 0; i < M; i++) printf("uni %.17g %.17g %.17g\n", mean[i], var[i], only[i]);
	free(mean); free(var); free(only);
	free_emulator_struct(e);
	return 0;
}

static int run_multi(int argc, char **argv)
{
	if (argc != 4) return 2;
	FILE *in = fopen(argv[2], "r");
	if (!in) return 3;
	multi_modelstruct *model = load_multi_modelstruct(in);
	fclose(in);
	multi_emulator *emu = alloc_multi_emulator(model);
	gsl_matrix *q = read_queries(argv[3], model->nparams);
	if (!q) return 5;
	const int M = (int)q->size1;
	for (int pca = 1; pca >= 0; pca--) {
		const int no = pca ? emu->nr : emu->nt;
		double *mean = (double *)malloc(sizeof(double) * (size_t)M * no), *var = (double *)malloc(sizeof(double) * (size_t)M * no);
		double *only = (double *)malloc(sizeof(double) * (size_t)M * no);
		emulate_points_multi_mean(emu, q, pca, only);
		emulate_points_multi(emu, q, pca, mean, var);
		for (int i = 0; i < M; i++) {
			printf("%s", pca ? "pca" : "obs");
			for (int j = 0; j < no; j++) printf(" %.17g %.17g", mean[(size_t)i * no + j], only[(size_t)i * no + j]);
			printf("\n");
		}
		free(mean); free(var); free(only);
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
