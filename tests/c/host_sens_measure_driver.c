/* Drives the host layer's sensitivity entries under an input measure (csrc/host/libemu.h: emulate_sensitivity_measure,
 * emulate_sensitivity_measure_multi) and prints the results for tests/test_host_sens_measure.py.  MEASURE_FILE holds one line
 * "kind lo hi" per parameter, kind 0 (uniform on [lo, hi]) or 1 (Gaussian, mean lo, sd hi); GRID_FILE one line of G values per
 * parameter.
 *
 *   host_sens_measure_driver single INPUT_MODEL_FILE cov_fn order MEASURE_FILE GRID_FILE G theta_full...
 *       "sens e0 var", "first ...", "total ...", "main j ..." per parameter, "e0main v", "post s_none s_all s_first.. s_rest..",
 *       "vpair ..." (d >= 2); then, the measure set back to all uniform (NULL), "usens e0 var" from the same bounds
 *   host_sens_measure_driver multi MODEL_SNAPSHOT_FILE MEASURE_FILE GRID_FILE G pca_space
 *       per output t: "out t e0 var", "first t ...", "total t ...", "main t j ..." per parameter, "e0main t v",
 *       "unc t var_e0 imse evar"
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

static int read_measure(const char *name, int d, int *kind, double *lo, double *hi)
{
	FILE *in = fopen(name, "r");
	if (!in) return 0;
	for (int j = 0; j < d; j++) if (fscanf(in, "%d %lf %lf", &kind[j], &lo[j], &hi[j]) != 3) return 0;
	fclose(in);
	return 1;
}

static double *read_grid(const char *name, int d, int G)
{
	FILE *in = fopen(name, "r");
	double *g = (double *)malloc(sizeof(double) * (size_t)d * G);
	if (!in) return NULL;
	for (int i = 0; i < d * G; i++) if (fscanf(in, "%lf", &g[i]) != 1) return NULL;
	fclose(in);
	return g;
}

static void row(const char *tag, const double *v, int n)
{
	printf("%s", tag);
	for (int i = 0; i < n; i++) printf(" %.17g", v[i]);
	printf("\n");
}

static int single(int argc, char **argv)
{
	if (argc < 8) return 2;
	gsl_matrix *x, *ymat;
	if (!read_model(argv[2], &x, &ymat)) return 3;
	const int cov = atoi(argv[3]), order = atoi(argv[4]), G = atoi(argv[7]);
	const int N = (int)x->size1, d = (int)x->size2;
	gsl_vector *y = gsl_vector_alloc(x->size1);
	for (int i = 0; i < N; i++) gsl_vector_set(y, i, gsl_matrix_get(ymat, i, 0));
	modelstruct *model = alloc_modelstruct_2(x, y, cov, order);
	const int nthetas = model->options->nthetas;
	if (argc != 8 + nthetas) return 4;
	for (int i = 0; i < nthetas; i++) gsl_vector_set(model->thetas, i, atof(argv[8 + i]));
	double *lo = (double *)malloc(sizeof(double) * 2 * (size_t)d), *hi = lo + d;
	int *kind = (int *)malloc(sizeof(int) * (size_t)d);
	if (!read_measure(argv[5], d, kind, lo, hi)) return 5;
	double *grid = read_grid(argv[6], d, G);
	if (!grid) return 6;
	emulator_struct *e = alloc_emulator_struct(model);
	emulate_sensitivity_measure(e, kind);
	double e0, var, *first = (double *)malloc(sizeof(double) * 2 * (size_t)d), *total = first + d;
	emulate_sensitivity(e, lo, hi, &e0, &var, first, total);
	printf("sens %.17g %.17g\n", e0, var);
	row("first", first, d);
	row("total", total, d);
	double *mainv = (double *)malloc(sizeof(double) * (size_t)d * G), e0m;
	emulate_main_effects(e, lo, hi, G, grid, &e0m, mainv);
	for (int j = 0; j < d; j++) {
		char tag[32];
		snprintf(tag, sizeof tag, "main %d", j);
		row(tag, mainv + (size_t)j * G, G);
	}
	printf("e0main %.17g\n", e0m);
	double *s = (double *)malloc(sizeof(double) * (2 + 2 * (size_t)d));
	emulate_sensitivity_post(e, lo, hi, s);
	row("post", s, 2 + 2 * d);
	if (d >= 2) {
		const int np = d * (d - 1) / 2;
		double *vp = (double *)malloc(sizeof(double) * 2 * (size_t)np);
		emulate_sensitivity_pairs(e, lo, hi, vp, vp + np);
		row("vpair", vp, np);
		free(vp);
	}
	/* back to all uniform: the bounds are read as a box again (the test gives bounds that are a valid box too) */
	emulate_sensitivity_measure(e, NULL);
	emulate_sensitivity(e, lo, hi, &e0, &var, first, total);
	printf("usens %.17g %.17g\n", e0, var);
	free(lo); free(kind); free(first); free(grid); free(mainv); free(s);
	free_emulator_struct(e);
	return 0;
}

static int multi(int argc, char **argv)
{
	if (argc != 7) return 2;
	FILE *fp = fopen(argv[2], "r");
	if (!fp) return 3;
	const int G = atoi(argv[5]), pca = atoi(argv[6]);
	multi_modelstruct *model = load_multi_modelstruct(fp);
	fclose(fp);
	const int d = model->nparams, nout = pca ? model->nr : model->nt;
	double *lo = (double *)malloc(sizeof(double) * 2 * (size_t)d), *hi = lo + d;
	int *kind = (int *)malloc(sizeof(int) * (size_t)d);
	if (!read_measure(argv[3], d, kind, lo, hi)) return 5;
	double *grid = read_grid(argv[4], d, G);
	if (!grid) return 6;
	multi_emulator *emu = alloc_multi_emulator(model);
	emulate_sensitivity_measure_multi(emu, kind);
	double *e0 = (double *)malloc(sizeof(double) * 3 * (size_t)nout), *var = e0 + nout, *e0m = var + nout;
	double *first = (double *)malloc(sizeof(double) * 2 * (size_t)nout * d), *total = first + (size_t)nout * d;
	emulate_sensitivity_multi(emu, pca, lo, hi, e0, var, first, total);
	double *mainv = (double *)malloc(sizeof(double) * (size_t)d * G * nout), *curve = (double *)malloc(sizeof(double) * (size_t)G);
	emulate_main_effects_multi(emu, pca, lo, hi, G, grid, e0m, mainv);
	double *ve0 = (double *)malloc(sizeof(double) * 3 * (size_t)nout), *imse = ve0 + nout, *evar = imse + nout;
	double *ef = (double *)malloc(sizeof(double) * 2 * (size_t)nout * d), *et = ef + (size_t)nout * d;
	emulate_sensitivity_uncertainty_multi(emu, pca, lo, hi, ve0, imse, evar, ef, et);
	for (int t = 0; t < nout; t++) {
		char tag[48];
		printf("out %d %.17g %.17g\n", t, e0[t], var[t]);
		snprintf(tag, sizeof tag, "first %d", t);
		row(tag, first + (size_t)t * d, d);
		snprintf(tag, sizeof tag, "total %d", t);
		row(tag, total + (size_t)t * d, d);
		for (int j = 0; j < d; j++) {
			for (int k = 0; k < G; k++) curve[k] = mainv[((size_t)j * G + k) * nout + t];
			snprintf(tag, sizeof tag, "main %d %d", t, j);
			row(tag, curve, G);
		}
		printf("e0main %d %.17g\n", t, e0m[t]);
		printf("unc %d %.17g %.17g %.17g\n", t, ve0[t], imse[t], evar[t]);
	}
	free(lo); free(kind); free(e0); free(first); free(grid); free(mainv); free(curve); free(ve0); free(ef);
	free_multi_emulator(emu);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc < 2) return 2;
	if (!strcmp(argv[1], "single")) return single(argc, argv);
	if (!strcmp(argv[1], "multi")) return multi(argc, argv);
	return 2;
}
