/* Drives the sensitivity entries of the host-side libEmu mirror (csrc/host/libemu.h: emulate_sensitivity, emulate_main_effects,
 * emulate_sensitivity_enqueue / _collect, emulate_sensitivity_multi, emulate_main_effects_multi) the way a caller of
 * alloc_emulator_struct / alloc_multi_emulator would, and prints the results for tests/test_host_sens.py.  BOX_FILE holds one
 * line "lo hi" per parameter; the main-effect grid is G equally spaced values from lo to hi per parameter.
 *
 *   host_sens_driver single INPUT_MODEL_FILE cov_fn order BOX_FILE G theta_full...
 *       "sens e0 var", "first ...", "total ...", "main j ..." per parameter, "e0main v"; then the enqueue / collect pair:
 *       "pair e0a e0b cov_all", "pfirst ...", "prest ..."
 *   host_sens_driver multi MODEL_SNAPSHOT_FILE BOX_FILE G pca_space
 *       per output t: "out t e0 var", "first t ...", "total t ...", "main t j ..." per parameter, "e0main t v"
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

static int read_box(const char *name, int d, double *lo, double *hi)
{
	FILE *in = fopen(name, "r");
	if (!in) return 0;
	for (int j = 0; j < d; j++) if (fscanf(in, "%lf %lf", &lo[j], &hi[j]) != 2) return 0;
	fclose(in);
	return 1;
}

static double *make_grid(int d, int G, const double *lo, const double *hi)
{
	double *g = (double *)malloc(sizeof(double) * (size_t)d * G);
	for (int j = 0; j < d; j++)
		for (int k = 0; k < G; k++) g[(size_t)j * G + k] = G > 1 ? lo[j] + k * (hi[j] - lo[j]) / (G - 1) : 0.5 * (lo[j] + hi[j]);
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
	if (argc < 7) return 2;
	gsl_matrix *x, *ymat;
	if (!read_model(argv[2], &x, &ymat)) return 3;
	const int cov = atoi(argv[3]), order = atoi(argv[4]), G = atoi(argv[6]);
	const int N = (int)x->size1, d = (int)x->size2;
	gsl_vector *y = gsl_vector_alloc(x->size1);
	for (int i = 0; i < N; i++) gsl_vector_set(y, i, gsl_matrix_get(ymat, i, 0));
	modelstruct *model = alloc_modelstruct_2(x, y, cov, order);
	const int nthetas = model->options->nthetas;
	if (argc != 7 + nthetas) return 4;
	for (int i = 0; i < nthetas; i++) gsl_vector_set(model->thetas, i, atof(argv[7 + i]));
	double *lo = (double *)malloc(sizeof(double) * 2 * (size_t)d), *hi = lo + d;
	if (!read_box(argv[5], d, lo, hi)) return 5;
	emulator_struct *e = alloc_emulator_struct(model);
	double e0[2], var, *first = (double *)malloc(sizeof(double) * 3 * (size_t)d), *total = first + d, *rest = total + d;
	emulate_sensitivity(e, lo, hi, e0, &var, first, total);
	printf("sens %.17g %.17g\n", e0[0], var);
	row("first", first, d);
	row("total", total, d);
	double *grid = make_grid(d, G, lo, hi), *mainv = (double *)malloc(sizeof(double) * (size_t)d * G), e0m;
	emulate_main_effects(e, lo, hi, G, grid, &e0m, mainv);
	for (int j = 0; j < d; j++) {
		char tag[32];
		snprintf(tag, sizeof tag, "main %d", j);
		row(tag, mainv + (size_t)j * G, G);
	}
	printf("e0main %.17g\n", e0m);
	void *dev = NULL;
	emulate_sensitivity_enqueue(e, NULL, lo, hi, &dev);
	emulate_sensitivity_collect(e, dev, e0, &var, first, rest);
	printf("pair %.17g %.17g %.17g\n", e0[0], e0[1], var);
	row("pfirst", first, d);
	row("prest", rest, d);
	free(lo); free(first); free(grid); free(mainv);
	free_emulator_struct(e);
	return 0;
}

static int multi(int argc, char **argv)
{
	if (argc != 6) return 2;
	FILE *fp = fopen(argv[2], "r");
	if (!fp) return 3;
	const int G = atoi(argv[4]), pca = atoi(argv[5]);
	multi_modelstruct *model = load_multi_modelstruct(fp);
	fclose(fp);
	const int d = model->nparams, nout = pca ? model->nr : model->nt;
	double *lo = (double *)malloc(sizeof(double) * 2 * (size_t)d), *hi = lo + d;
	if (!read_box(argv[3], d, lo, hi)) return 5;
	multi_emulator *emu = alloc_multi_emulator(model);
	double *e0 = (double *)malloc(sizeof(double) * 3 * (size_t)nout), *var = e0 + nout, *e0m = var + nout;
	double *first = (double *)malloc(sizeof(double) * 2 * (size_t)nout * d), *total = first + (size_t)nout * d;
	emulate_sensitivity_multi(emu, pca, lo, hi, e0, var, first, total);
	double *grid = make_grid(d, G, lo, hi), *mainv = (double *)malloc(sizeof(double) * (size_t)d * G * nout);
	double *curve = (double *)malloc(sizeof(double) * (size_t)G);
	emulate_main_effects_multi(emu, pca, lo, hi, G, grid, e0m, mainv);
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
	}
	free(lo); free(e0); free(first); free(grid); free(mainv); free(curve);
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
