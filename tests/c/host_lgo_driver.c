/* Drives the K-fold / leave-group-out entries of the host-side libEmu mirror (csrc/host/libemu.h: emulate_lgo,
 * emulate_lgo_multi) the way a caller of alloc_emulator_struct / alloc_multi_emulator would, and prints the results for
 * tests/test_host_lgo.py.  Training point i is in group i mod K.
 *
 *   host_lgo_driver lgo INPUT_MODEL_FILE cov_fn order K theta_full...
 *       "lgo mean variance werr" per training point in design order, then "grp maha logpdf" per group
 *   host_lgo_driver multi MODEL_SNAPSHOT_FILE K pca_space
 *       "pt v_0 v_1 ..." per training point (mean and variance alternating over the outputs), then "stat c g maha logpdf"
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

static int *folds(int N, int K)
{
	int *g = (int *)malloc(sizeof(int) * (size_t)N);
	for (int i = 0; i < N; i++) g[i] = i % K;
	return g;
}

static int single(int argc, char **argv)
{
	if (argc < 6) return 2;
	gsl_matrix *x, *ymat;
	if (!read_model(argv[2], &x, &ymat)) return 3;
	const int cov = atoi(argv[3]), order = atoi(argv[4]), K = atoi(argv[5]);
	const int N = (int)x->size1;
	gsl_vector *y = gsl_vector_alloc(x->size1);
	for (int i = 0; i < N; i++) gsl_vector_set(y, i, gsl_matrix_get(ymat, i, 0));
	modelstruct *model = alloc_modelstruct_2(x, y, cov, order);
	const int nthetas = model->options->nthetas;
	if (argc != 6 + nthetas) return 4;
	for (int i = 0; i < nthetas; i++) gsl_vector_set(model->thetas, i, atof(argv[6 + i]));
	emulator_struct *e = alloc_emulator_struct(model);
	int *group = folds(N, K);
	double *pt = (double *)malloc(sizeof(double) * 3 * (size_t)N), *st = (double *)malloc(sizeof(double) * 2 * (size_t)K);
	emulate_lgo(e, K, group, pt, pt + N, pt + 2 * N, st, st + K);
	for (int i = 0; i < N; i++) printf("lgo %.17g %.17g %.17g\n", pt[i], pt[N + i], pt[2 * N + i]);
	for (int g = 0; g < K; g++) printf("grp %.17g %.17g\n", st[g], st[K + g]);
	free(pt); free(st); free(group);
	free_emulator_struct(e);
	return 0;
}

static int multi(int argc, char **argv)
{
	if (argc != 5) return 2;
	FILE *fp = fopen(argv[2], "r");
	if (!fp) return 3;
	const int K = atoi(argv[3]), pca = atoi(argv[4]);
	multi_modelstruct *model = load_multi_modelstruct(fp);
	fclose(fp);
	multi_emulator *emu = alloc_multi_emulator(model);
	const int N = model->nmodel_points, nr = model->nr, nout = pca ? nr : model->nt;
	int *group = folds(N, K);
	double *mean = (double *)malloc(sizeof(double) * (size_t)N * nout), *var = (double *)malloc(sizeof(double) * (size_t)N * nout);
	double *maha = (double *)malloc(sizeof(double) * (size_t)nr * K), *logpdf = (double *)malloc(sizeof(double) * (size_t)nr * K);
	emulate_lgo_multi(emu, pca, K, group, mean, var, maha, logpdf);
	for (int i = 0; i < N; i++) {
		printf("pt");
		for (int j = 0; j < nout; j++) printf(" %.17g %.17g", mean[(size_t)i * nout + j], var[(size_t)i * nout + j]);
		printf("\n");
	}
	for (int c = 0; c < nr; c++)
		for (int g = 0; g < K; g++) printf("stat %d %d %.17g %.17g\n", c, g, maha[(size_t)c * K + g], logpdf[(size_t)c * K + g]);
	free(mean); free(var); free(maha); free(logpdf); free(group);
	free_multi_emulator(emu);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc < 2) return 2;
	if (!strcmp(argv[1], "lgo")) return single(argc, argv);
	if (!strcmp(argv[1], "multi")) return multi(argc, argv);
	return 2;
}
