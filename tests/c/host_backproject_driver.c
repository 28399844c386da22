/* gpemu_host_backproject (multi.c), the one PCA -> observable rule of the host layer, against the rule written out as
 * literal loops (multivar_support.c:118-157: the factor first, the sum over the components in index order from 0.0, the
 * training mean added afterwards).  No device: alloc_multimodelstruct is the PCA of the training outputs, host code.
 *   host_backproject_driver INPUT_MODEL_FILE OUT_BIN
 * stdout: "dims nt nr d", then per case "case NAME squared add_mean nrows width equal" (equal: memcmp of the two results);
 * OUT_BIN: raw doubles -- training_mean (nt), evals (nr), evecs (nt x nr), then per case in (nrows x nr x width) and the
 * routine's out (nrows x nt x width)
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
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

/* the rule as every entry of multi.c spelt it before it had one home */
static void literal_rule(const multi_modelstruct *m, int squared, int add_mean, size_t nrows, size_t width, const double *in, double *out)
{
	const size_t nt = (size_t)m->nt, nr = (size_t)m->nr;
	for (size_t q = 0; q < nrows; q++)
		for (size_t t = 0; t < nt; t++)
			for (size_t j = 0; j < width; j++) {
				double s = 0.0;
				for (size_t c = 0; c < nr; c++) {
					const double u = gsl_matrix_get(m->pca_evecs_r, t, c), lam = gsl_vector_get(m->pca_evals_r, c);
					const double f = squared ? pow(u, 2.0) * lam : u * sqrt(lam);
					s += f * in[(q * nr + c) * width + j];
				}
				out[(q * nt + t) * width + j] = (add_mean && j == 0) ? gsl_vector_get(m->training_mean, t) + s : s;
			}
}

int main(int argc, char **argv)
{
	if (argc < 3) return 2;
	gsl_matrix *x, *y;
	if (!read_model(argv[1], &x, &y)) return 3;
	multi_modelstruct *m = alloc_multimodelstruct(x, y, POWEREXPCOVFN, 1, 0.99);
	const size_t nt = (size_t)m->nt, nr = (size_t)m->nr, d = (size_t)m->nparams;
	FILE *bin = fopen(argv[2], "wb");
	if (!bin) return 4;
	printf("dims %zu %zu %zu\n", nt, nr, d);
	for (size_t t = 0; t < nt; t++) { const double v = gsl_vector_get(m->training_mean, t); fwrite(&v, sizeof v, 1, bin); }
	for (size_t c = 0; c < nr; c++) { const double v = gsl_vector_get(m->pca_evals_r, c); fwrite(&v, sizeof v, 1, bin); }
	for (size_t t = 0; t < nt; t++)
		for (size_t c = 0; c < nr; c++) { const double v = gsl_matrix_get(m->pca_evecs_r, t, c); fwrite(&v, sizeof v, 1, bin); }

	const struct { const char *name; int squared, add_mean; size_t nrows, width; } cases[4] = {
		{"mean", 0, 1, 3, 1}, {"variance", 1, 0, 3, 1}, {"mean_gradient", 0, 0, 3, d}, {"covariance_layout", 1, 0, 1, 9}};
	gsl_rng *r = gsl_rng_alloc(gsl_rng_default);
	gsl_rng_set(r, 20240611UL);
	for (int k = 0; k < 4; k++) {
		const size_t nin = cases[k].nrows * nr * cases[k].width, nout = cases[k].nrows * nt * cases[k].width;
		double *in = (double *)malloc(sizeof(double) * nin);
		double *got = (double *)malloc(sizeof(double) * nout), *want = (double *)malloc(sizeof(double) * nout);
		/* means and gradients of either sign, variances and covariance entries likewise (the rule is linear: no sign matters) */
		for (size_t i = 0; i < nin; i++) in[i] = 4.0 * gsl_rng_uniform(r) - 2.0;
		memset(got, 0xff, sizeof(double) * nout);         /* the routine writes every element: none of this survives */
		gpemu_host_backproject(m, cases[k].squared, cases[k].add_mean, cases[k].nrows, cases[k].width, in, got);
		literal_rule(m, cases[k].squared, cases[k].add_mean, cases[k].nrows, cases[k].width, in, want);
		const int equal = memcmp(got, want, sizeof(double) * nout) == 0;
		printf("case %s %d %d %zu %zu %d\n", cases[k].name, cases[k].squared, cases[k].add_mean, cases[k].nrows, cases[k].width, equal);
		fwrite(in, sizeof(double), nin, bin);
		fwrite(got, sizeof(double), nout, bin);
		free(in); free(got); free(want);
	}
	gsl_rng_free(r);
	fclose(bin);
	return 0;
}
