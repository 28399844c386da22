/* Drives the leave-one-out entry of the host-side libEmu mirror (csrc/host/libemu.h: emulate_loo) the way a caller of
 * alloc_emulator_struct would, and prints the results for tests/test_host_loo.py.
 *
 *   host_loo_driver loo INPUT_MODEL_FILE cov_fn order theta_full...
 *
 * One line "loo mean variance" per training point, in design order.
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

int main(int argc, char **argv)
{
	if (argc < 5 || strcmp(argv[1], "loo")) return 2;
	gsl_matrix *x, *ymat;
	if (!read_model(argv[2], &x, &ymat)) return 3;
	const int cov = atoi(argv[3]), order = atoi(argv[4]);
	const int N = (int)x->size1;
	gsl_vector *y = gsl_vector_alloc(x->size1);
	for (int i = 0; i < N; i++) gsl_vector_set(y, i, gsl_matrix_get(ymat, i, 0));
	modelstruct *model = alloc_modelstruct_2(x, y, cov, order);
	const int nthetas = model->options->nthetas;
	if (argc != 5 + nthetas) return 4;
	for (int i = 0; i < nthetas; i++) gsl_vector_set(model->thetas, i, atof(argv[5 + i]));
	emulator_struct *e = alloc_emulator_struct(model);
	double *mean = (double *)malloc(sizeof(double) * (size_t)N), *var = (double *)malloc(sizeof(double) * (size_t)N);
	emulate_loo(e, mean, var);
	for (int i = 0; i < N; i++) printf("loo %.17g %.17g\n", mean[i], var[i]);
	free(mean); free(var);
	free_emulator_struct(e);
	return 0;
}
