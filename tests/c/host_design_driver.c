/* Drives the design entries of the host-side libEmu mirror (csrc/host/libemu.h: emulate_design_gain, emulate_design_gain_multi)
 * and prints the results for tests/test_host_design.py.  BOX_FILE holds one line "lo hi" per parameter, POINTS_FILE the
 * candidates, nparams numbers each.
 *
 *   host_design_driver MODEL_SNAPSHOT_FILE BOX_FILE POINTS_FILE pca_space
 *       per PCA component c: "comp c gain..", "cnum c num..", "cvar c var.." (npoints values each)
 *       per candidate q: "gain q" with one value per output, "total q v"
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

int main(int argc, char **argv)
{
	if (argc != 5) return 2;
	FILE *fp = fopen(argv[1], "r");
	if (!fp) return 3;
	const int pca = atoi(argv[4]);
	multi_modelstruct *model = load_multi_modelstruct(fp);
	fclose(fp);
	const size_t d = (size_t)model->nparams, nr = (size_t)model->nr, nout = pca ? nr : (size_t)model->nt;
	double *lo = (double *)malloc(sizeof(double) * 2 * d), *hi = lo + d;
	FILE *bf = fopen(argv[2], "r");
	if (!bf) return 5;
	for (size_t j = 0; j < d; j++) if (fscanf(bf, "%lf %lf", &lo[j], &hi[j]) != 2) return 5;
	fclose(bf);
	size_t cap = 64, n = 0;
	double *pts = (double *)malloc(sizeof(double) * cap), x;
	FILE *pf = fopen(argv[3], "r");
	if (!pf) return 6;
	while (fscanf(pf, "%lf", &x) == 1) {
		if (n == cap) pts = (double *)realloc(pts, sizeof(double) * (cap *= 2));
		pts[n++] = x;
	}
	fclose(pf);
	if (!n || n % d) return 6;
	const size_t np = n / d;
	multi_emulator *emu = alloc_multi_emulator(model);
	double *g = (double *)malloc(sizeof(double) * 3 * np), *num = g + np, *var = num + np;
	for (size_t c = 0; c < nr; c++) {
		emulate_design_gain(emu->emu_struct_array[c], lo, hi, (int)np, pts, g, num, var);
		row("comp", c, g, np);
		row("cnum", c, num, np);
		row("cvar", c, var, np);
	}
	double *go = (double *)malloc(sizeof(double) * np * nout), *tot = (double *)malloc(sizeof(double) * np);
	emulate_design_gain_multi(emu, pca, lo, hi, (int)np, pts, go, tot);
	for (size_t q = 0; q < np; q++) {
		row("gain", q, go + q * nout, nout);
		row("total", q, tot + q, 1);
	}
	free(lo); free(pts); free(g); free(go); free(tot);
	free_multi_emulator(emu);
	return 0;
}
