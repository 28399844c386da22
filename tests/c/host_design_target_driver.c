/* Drives the targeted design entries of the host-side libEmu mirror (csrc/host/libemu.h: emulate_design_target_set,
 * emulate_design_target_gain, emulate_design_target_gain_multi) and prints the results for tests/test_host_design_target.py.
 * TARGETS_FILE holds the targets, nparams numbers and a weight per line; POINTS_FILE the candidates, nparams numbers each.
 *
 *   host_design_target_driver MODEL_SNAPSHOT_FILE TARGETS_FILE POINTS_FILE pca_space
 *       per PCA component c: "comp c gain..", "cnum c num..", "cvar c var.." (npoints values each), "ctv c target_var",
 *                            "cvt c var_t.." (ntargets values)
 *       per candidate q: "gain q" with one value per output, "total q v"; then "tv 0" with one value per output and
 *       "again 0 gain..": component 0 set, asked and released once more behind the multi call
 */
#include <stdio.h>
#include <stdlib.h>
#include "libemu.h"

static void row(const char *tag, size_t i, const double *v, size_t n)
{
	printf("%s %zu", tag, i);
	for (size_t k = 0; k < n; k++) printf(" %.17g", v[k]);
	printf("\n");
}

static double *numbers(const char *path, size_t *n)
{
	size_t cap = 64;
	double *v = (double *)malloc(sizeof(double) * cap), x;
	FILE *f = fopen(path, "r");
	*n = 0;
	if (!f) return NULL;
	while (fscanf(f, "%lf", &x) == 1) {
		if (*n == cap) v = (double *)realloc(v, sizeof(double) * (cap *= 2));
		v[(*n)++] = x;
	}
	fclose(f);
	return v;
}

int main(int argc, char **argv)
{
	if (argc != 5) return 2;
	FILE *fp = fopen(argv[1], "r");
	if (!fp) return 3;
	const int pca = atoi(argv[4]);
	multi_modelstruct *model = load_multi_modelstruct(fp);
	fclose(fp);
	const size_t d = (size_t)model->nparams, nr = (size_t)model->nr, nout = pca ? nr : (size_t)model->nt;
	size_t nt, n;
	double *tw = numbers(argv[2], &nt), *pts = numbers(argv[3], &n);
	if (!tw || !nt || nt % (d + 1)) return 5;
	if (!pts || !n || n % d) return 6;
	const size_t ns = nt / (d + 1), np = n / d;
	double *tg = (double *)malloc(sizeof(double) * ns * (d + 1)), *w = tg + ns * d;
	for (size_t s = 0; s < ns; s++) {
		for (size_t j = 0; j < d; j++) tg[s * d + j] = tw[s * (d + 1) + j];
		w[s] = tw[s * (d + 1) + d];
	}
	multi_emulator *emu = alloc_multi_emulator(model);
	double *g = (double *)malloc(sizeof(double) * (3 * np + ns + 1)), *num = g + np, *var = num + np, *vt = var + np, *tv = vt + ns;
	for (size_t c = 0; c < nr; c++) {
		emulate_design_target_set(emu->emu_struct_array[c], (int)ns, tg, w, tv, vt);
		emulate_design_target_gain(emu->emu_struct_array[c], (int)np, pts, g, num, var);
		row("comp", c, g, np);
		row("cnum", c, num, np);
		row("cvar", c, var, np);
		row("ctv", c, tv, 1);
		row("cvt", c, vt, ns);
	}
	double *go = (double *)malloc(sizeof(double) * (np * nout + np + nout)), *tot = go + np * nout, *tvo = tot + np;
	emulate_design_target_gain_multi(emu, pca, (int)ns, tg, w, (int)np, pts, go, tot, tvo);
	for (size_t q = 0; q < np; q++) {
		row("gain", q, go + q * nout, nout);
		row("total", q, tot + q, 1);
	}
	row("tv", 0, tvo, nout);
	/* the multi entry left nothing resident: a component's targets can be set, used and released again */
	emulate_design_target_set(emu->emu_struct_array[0], (int)ns, tg, w, tv, NULL);
	emulate_design_target_gain(emu->emu_struct_array[0], (int)np, pts, g, NULL, NULL);
	emulate_design_target_release(emu->emu_struct_array[0]);
	row("again", 0, g, np);
	free(tw); free(pts); free(tg); free(g); free(go);
	free_multi_emulator(emu);
	return 0;
}
