/* Drives the joint-covariance entries of the host-side libEmu mirror (csrc/host/libemu.h: emulate_points_cov and its halves,
 * emulate_points_multi_cov), for tests/test_host_cov.py.
 *
 *   host_cov_driver uni INPUT_MODEL_FILE QUERY_FILE cov_fn order theta_full...
 *       one line "mean m_0 .. m_{M-1}", per query p one line "cov S_p0 .. S_p,M-1" from one emulate_points_cov call, one line
 *       "batch mean var" per query from emulate_points after it, then one line "same N": how many values of a call with a
 *       NULL mean, of the enqueue / collect pair and of a second call differ from the first in any bit (0 expected)
 *   host_cov_driver multi MODEL_SNAPSHOT_FILE QUERY_FILE
 *       per space S in {pca, obs}: the lines "S_m" (means, one per query), "S_c o" (output o's matrix, one line per row);
 *       per component c the lines "comp_m c" and "comp_c c" of emulate_points_cov on that component's emulator_struct;
 *       "multi_m" / "multi_v": means and variances of emulate_points_multi in observable space, one line per query
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

static void print_rows(const char *tag, int idx, const double *v, int rows, int n)
{
	for (int i = 0; i < rows; i++) {
		if (idx >= 0) printf("%s %d", tag, idx); else printf("%s", tag);
		for (int j = 0; j < n; j++) printf(" %.17g", v[(size_t)i * n + j]);
		printf("\n");
	}
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
	const size_t mm = (size_t)M * M;
	emulator_struct *e = alloc_emulator_struct(model);
	double *mean = vec(M), *S = vec(mm), *m2 = vec(M), *S2 = vec(mm), *v2 = vec(M);
	emulate_points_cov(e, q, mean, S);                   /* first: before any other path has allocated anything */
	int bad = 0;
	emulate_points_cov(e, q, m2, S2);
	bad += differ(mean, m2, M) + differ(S, S2, mm);
	memset(S2, 0, sizeof(double) * mm);
	emulate_points_cov(e, q, NULL, S2);                  /* the mean may be NULL */
	bad += differ(S, S2, mm);
	void *dev = NULL;
	memset(S2, 0, sizeof(double) * mm);
	emulate_points_cov_enqueue(e, q, &dev);
	emulate_points_cov_collect(e, dev, M, m2, S2);
	bad += differ(mean, m2, M) + differ(S, S2, mm);
	emulate_points(e, q, m2, v2);                        /* the batch path shares its buffers and still answers */
	print_rows("mean", -1, mean, 1, M);
	print_rows("cov", -1, S, M, M);
	for (int i = 0; i < M; i++) printf("batch %.17g %.17g\n", m2[i], v2[i]);
	printf("same %d\n", bad);
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
	const int d = model->nparams;
	gsl_matrix *q = read_queries(argv[3], d);
	if (!q) return 5;
	const int M = (int)q->size1;
	const size_t mm = (size_t)M * M;
	for (int pca = 1; pca >= 0; pca--) {
		const int no = pca ? emu->nr : emu->nt;
		double *mean = vec((size_t)M * no), *S = vec(mm * no);
		emulate_points_multi_cov(emu, q, pca, mean, S);
		print_rows(pca ? "pca_m" : "obs_m", -1, mean, M, no);
		for (int o = 0; o < no; o++) print_rows(pca ? "pca_c" : "obs_c", o, S + mm * o, M, M);
		free(mean); free(S);
	}
	double *mean = vec(M), *S = vec(mm);
	for (int c = 0; c < emu->nr; c++) {
		emulate_points_cov(emu->emu_struct_array[c], q, mean, S);
		print_rows("comp_m", c, mean, 1, M);
		print_rows("comp_c", c, S, M, M);
	}
	double *mo = vec((size_t)M * emu->nt), *vo = vec((size_t)M * emu->nt);
	emulate_points_multi(emu, q, 0, mo, vo);
	print_rows("multi_m", -1, mo, M, emu->nt);
	print_rows("multi_v", -1, vo, M, emu->nt);
	free_multi_emulator(emu);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc >= 2 && !strcmp(argv[1], "uni")) return run_uni(argc, argv);
	if (argc >= 2 && !strcmp(argv[1], "multi")) return run_multi(argc, argv);
	return 2;
}
