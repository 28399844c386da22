/* Drives the gradient entries of the host-side libEmu mirror (csrc/host/libemu.h: emulate_points_grad and its halves,
 * emulate_points_multi_grad), for tests/test_host_var_grad.py.
 *
 *   host_var_grad_driver uni INPUT_MODEL_FILE QUERY_FILE cov_fn order theta_full...
 *       per query one line "uni mean var gm_0 .. gm_{d-1} gv_0 .. gv_{d-1}" from one emulate_points_grad call with every
 *       output, then one line "same N": how many values of the calls with some outputs NULL, of the enqueue / collect pair and
 *       of a second full call differ from it in any bit (0 expected)
 *   host_var_grad_driver multi MODEL_SNAPSHOT_FILE QUERY_FILE
 *       per query and space S in {pca, obs} the lines "S_m", "S_v" (means, variances), "S_gm", "S_gv" (gradients,
 *       output-major); per query and component c the line "comp c mean var gm.. gv.." of emulate_points_grad on that
 *       component's emulator_struct
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

static double *vec(size_t n) { return (double *)malloc(sizeof(double) * n); }
static int differ(const double *a, const double *b, size_t n)
{
	int c = 0;
	for (size_t i = 0; i < n; i++) c += memcmp(a + i, b + i, sizeof(double)) != 0;
	return c;
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
	const size_t md = (size_t)M * d;
	emulator_struct *e = alloc_emulator_struct(model);
	double *mean = vec(M), *var = vec(M), *gm = vec(md), *gv = vec(md);
	double *m2 = vec(M), *v2 = vec(M), *gm2 = vec(md), *gv2 = vec(md);
	emulate_points_grad(e, q, mean, var, gm, gv);        /* first: before any other path has allocated anything */
	int bad = 0;
	emulate_points_grad(e, q, m2, v2, gm2, gv2);
	bad += differ(mean, m2, M) + differ(var, v2, M) + differ(gm, gm2, md) + differ(gv, gv2, md);
	emulate_points_grad(e, q, NULL, NULL, NULL, gv2);    /* any output may be NULL */
	bad += differ(gv, gv2, md);
	emulate_points_grad(e, q, NULL, v2, NULL, NULL);
	bad += differ(var, v2, M);
	emulate_points_grad(e, q, NULL, NULL, gm2, NULL);    /* (no variance asked for: the mean-gradient sweep alone) */
	bad += differ(gm, gm2, md);
	emulate_points_grad_enqueue(e, q);
	emulate_points_grad_collect(e, M, m2, v2, gm2, gv2);
	bad += differ(mean, m2, M) + differ(var, v2, M) + differ(gm, gm2, md) + differ(gv, gv2, md);
	emulate_points(e, q, m2, v2);                        /* the batch path shares its buffers and still answers */
	for (int i = 0; i < M; i++) {
		printf("uni %.17g %.17g", mean[i], var[i]);
		for (int j = 0; j < d; j++) printf(" %.17g", gm[(size_t)i * d + j]);
		for (int j = 0; j < d; j++) printf(" %.17g", gv[(size_t)i * d + j]);
		printf("\nbatch %.17g %.17g\n", m2[i], v2[i]);
	}
	printf("same %d\n", bad);
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
		double *mean = vec((size_t)M * no), *var = vec((size_t)M * no), *gm = vec((size_t)M * no * d), *gv = vec((size_t)M * no * d);
		emulate_points_multi_grad(emu, q, pca, mean, var, gm, gv);
		print_rows(pca ? "pca_m" : "obs_m", mean, M, no);
		print_rows(pca ? "pca_v" : "obs_v", var, M, no);
		print_rows(pca ? "pca_gm" : "obs_gm", gm, M, no * d);
		print_rows(pca ? "pca_gv" : "obs_gv", gv, M, no * d);
		free(mean); free(var); free(gm); free(gv);
	}
	double *mean = vec(M), *var = vec(M), *gm = vec((size_t)M * d), *gv = vec((size_t)M * d);
	for (int c = 0; c < emu->nr; c++) {
		emulate_points_grad(emu->emu_struct_array[c], q, mean, var, gm, gv);
		for (int i = 0; i < M; i++) {
			printf("comp %d %.17g %.17g", c, mean[i], var[i]);
			for (int j = 0; j < d; j++) printf(" %.17g", gm[(size_t)i * d + j]);
			for (int j = 0; j < d; j++) printf(" %.17g", gv[(size_t)i * d + j]);
			printf("\n");
		}
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
