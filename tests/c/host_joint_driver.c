/* Drives the hold-out validation and joint-draw entries of the host-side libEmu mirror (csrc/host/libemu.h:
 * emulate_points_holdout and its halves, emulate_points_draw, emulate_points_multi_holdout, emulate_points_multi_draw,
 * gpemu_host_project_observations), for tests/test_host_joint.py.
 *
 *   host_joint_driver uni INPUT_MODEL_FILE QUERY_FILE AUX_FILE cov_fn order theta_full...
 *       AUX_FILE: M observations, M noise variances, then ndraw x M normals.  Lines "mean", "var", "werr" (M numbers each),
 *       "stat maha logdet logpdf", one "draw" line per draw, from one emulate_points_holdout / emulate_points_draw; then
 *       "same N": how many values of a second call, of the enqueue / collect pair (and a draw after it) and of a call with
 *       NULL outputs differ from the first in any bit (0 expected)
 *   host_joint_driver multi MODEL_SNAPSHOT_FILE QUERY_FILE Y_FILE Z_FILE
 *       Y_FILE: M x nt observations; Z_FILE: nr x ndraw x M normals.  Lines "proj c" (component c's projected observations),
 *       "pca_m" / "pca_v" / "pca_w" (one per query, nr numbers), "stat c maha logdet logpdf", "sum L"; per component the lines
 *       "comp_m c", "comp_v c", "comp_w c", "comp_stat c ..." of emulate_points_holdout on that component's emulator_struct
 *       with its projected observations and "comp_draw c" (one per draw) of emulate_points_draw after it; "draw_pca s" and
 *       "draw_obs s" (one per query) of emulate_points_multi_draw
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

/* all numbers of the file */
static double *read_numbers(const char *name, size_t *count)
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
	*count = n;
	return v;
}

static gsl_matrix *read_queries(const char *name, int d)
{
	size_t n = 0;
	double *v = read_numbers(name, &n);
	if (!v || n == 0 || n % (size_t)d) return NULL;
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
	if (argc < 7) return 2;
	gsl_matrix *x, *ymat;
	if (!read_model(argv[2], &x, &ymat)) return 3;
	const int cov = atoi(argv[5]), order = atoi(argv[6]);
	const int N = (int)x->size1, d = (int)x->size2;
	gsl_vector *y = gsl_vector_alloc(x->size1);
	for (int i = 0; i < N; i++) gsl_vector_set(y, i, gsl_matrix_get(ymat, i, 0));
	modelstruct *model = alloc_modelstruct_2(x, y, cov, order);
	const int nthetas = model->options->nthetas;
	if (argc != 7 + nthetas) return 4;
	for (int i = 0; i < nthetas; i++) gsl_vector_set(model->thetas, i, atof(argv[7 + i]));
	gsl_matrix *q = read_queries(argv[3], d);
	if (!q) return 5;
	const size_t M = q->size1;
	size_t na = 0;
	double *aux = read_numbers(argv[4], &na);
	if (!aux || na < 3 * M || (na - 2 * M) % M) return 6;
	const double *yobs = aux, *noise = aux + M, *z = aux + 2 * M;
	const int nd = (int)((na - 2 * M) / M);
	emulator_struct *e = alloc_emulator_struct(model);
	double *mean = vec(M), *var = vec(M), *werr = vec(M), st[3], *draw = vec(nd * M);
	double *m2 = vec(M), *v2 = vec(M), *w2 = vec(M), s2[3], *d2 = vec(nd * M);
	emulate_points_holdout(e, q, yobs, noise, mean, var, werr, &st[0], &st[1], &st[2]);    /* first: nothing else has allocated */
	emulate_points_draw(e, nd, z, draw);
	int bad = 0;
	emulate_points_holdout(e, q, yobs, noise, m2, v2, w2, &s2[0], &s2[1], &s2[2]);
	emulate_points_draw(e, nd, z, d2);
	bad += differ(mean, m2, M) + differ(var, v2, M) + differ(werr, w2, M) + differ(st, s2, 3) + differ(draw, d2, nd * M);
	void *dev = NULL;
	memset(m2, 0, sizeof(double) * M); memset(v2, 0, sizeof(double) * M); memset(w2, 0, sizeof(double) * M); memset(d2, 0, sizeof(double) * nd * M);
	emulate_points_holdout_enqueue(e, q, yobs, noise, &dev);
	emulate_points_holdout_collect(e, dev, (int)M, 1, m2, v2, w2, &s2[0], &s2[1], &s2[2]);
	emulate_points_draw(e, nd, z, d2);
	bad += differ(mean, m2, M) + differ(var, v2, M) + differ(werr, w2, M) + differ(st, s2, 3) + differ(draw, d2, nd * M);
	emulate_points_holdout(e, q, yobs, noise, NULL, NULL, NULL, NULL, &s2[1], NULL);     /* every other output may be NULL */
	emulate_points_draw(e, nd, z, d2);
	bad += differ(st + 1, s2 + 1, 1) + differ(draw, d2, nd * M);
	print_rows("mean", -1, mean, 1, (int)M);
	print_rows("var", -1, var, 1, (int)M);
	print_rows("werr", -1, werr, 1, (int)M);
	print_rows("stat", -1, st, 1, 3);
	print_rows("draw", -1, draw, nd, (int)M);
	printf("same %d\n", bad);
	free_emulator_struct(e);
	return 0;
}

static int run_multi(int argc, char **argv)
{
	if (argc != 6) return 2;
	FILE *in = fopen(argv[2], "r");
	if (!in) return 3;
	multi_modelstruct *model = load_multi_modelstruct(in);
	fclose(in);
	multi_emulator *emu = alloc_multi_emulator(model);
	const int d = model->nparams, nr = emu->nr, nt = emu->nt;
	gsl_matrix *q = read_queries(argv[3], d);
	if (!q) return 5;
	const size_t M = q->size1;
	size_t ny = 0, nz = 0;
	double *Y = read_numbers(argv[4], &ny), *Z = read_numbers(argv[5], &nz);
	if (!Y || ny != M * (size_t)nt || !Z || nz == 0 || nz % (M * (size_t)nr)) return 6;
	const int nd = (int)(nz / (M * (size_t)nr));
	double *proj = vec(M * nr);
	gpemu_host_project_observations(model, M, Y, proj);
	for (int c = 0; c < nr; c++) print_rows("proj", c, proj + (size_t)c * M, 1, (int)M);
	double *mean = vec(M * nr), *var = vec(M * nr), *werr = vec(M * nr), *stat = vec(3 * (size_t)nr), sum = 0.0;
	emulate_points_multi_holdout(emu, q, Y, NULL, mean, var, werr, stat, stat + nr, stat + 2 * nr, &sum);
	print_rows("pca_m", -1, mean, (int)M, nr);
	print_rows("pca_v", -1, var, (int)M, nr);
	print_rows("pca_w", -1, werr, (int)M, nr);
	for (int c = 0; c < nr; c++) printf("stat %d %.17g %.17g %.17g\n", c, stat[c], stat[nr + c], stat[2 * nr + c]);
	printf("sum %.17g\n", sum);
	for (int pca = 1; pca >= 0; pca--) {
		const int no = pca ? nr : nt;
		double *out = vec((size_t)nd * M * no);
		emulate_points_multi_draw(emu, pca, (int)M, nd, Z, out);
		for (int s = 0; s < nd; s++) print_rows(pca ? "draw_pca" : "draw_obs", s, out + (size_t)s * M * no, (int)M, no);
		free(out);
	}
	double *mc = vec(M), *vc = vec(M), *wc = vec(M), *dc = vec((size_t)nd * M), st[3];
	for (int c = 0; c < nr; c++) {
		emulate_points_holdout(emu->emu_struct_array[c], q, proj + (size_t)c * M, NULL, mc, vc, wc, &st[0], &st[1], &st[2]);
		emulate_points_draw(emu->emu_struct_array[c], nd, Z + (size_t)c * nd * M, dc);
		print_rows("comp_m", c, mc, 1, (int)M);
		print_rows("comp_v", c, vc, 1, (int)M);
		print_rows("comp_w", c, wc, 1, (int)M);
		print_rows("comp_stat", c, st, 1, 3);
		print_rows("comp_draw", c, dc, nd, (int)M);
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
