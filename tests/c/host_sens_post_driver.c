/* Drives the emulator-uncertainty entries of the host-side libEmu mirror (csrc/host/libemu.h: emulate_sensitivity_post,
 * emulate_sensitivity_uncertainty, emulate_main_effects_var / _band and the two _multi forms) and prints the results for
 * tests/test_host_sens_post.py.  BOX_FILE holds one line "lo hi" per parameter; the grid is G equally spaced values per parameter.
 *
 *   host_sens_post_driver MODEL_SNAPSHOT_FILE BOX_FILE G pca_space
 *       per PCA component c: "comp c S_none S_all S_first.. S_rest..", "cplug c e0 V", "cfirst c ..", "ctotal c ..",
 *           "cunc c var_e0 imse evar", "cefirst c ..", "cetotal c ..", "cvar c j .." per parameter, "cvare0 c v"
 *       per output t: "plug t e0 V", "pfirst t ..", "ptotal t ..", "unc t var_e0 imse evar", "efirst t ..", "etotal t ..",
 *           "main t j ..", "sd t j .." per parameter, "e0main t v"
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "libemu.h"

static void row(const char *tag, const double *v, size_t n)
{
	printf("%s", tag);
	for (size_t i = 0; i < n; i++) printf(" %.17g", v[i]);
	printf("\n");
}

int main(int argc, char **argv)
{
	if (argc != 5) return 2;
	FILE *fp = fopen(argv[1], "r");
	if (!fp) return 3;
	const int G = atoi(argv[3]), pca = atoi(argv[4]);
	multi_modelstruct *model = load_multi_modelstruct(fp);
	fclose(fp);
	const size_t d = (size_t)model->nparams, nr = (size_t)model->nr, nout = pca ? nr : (size_t)model->nt, ng = d * (size_t)G;
	double *lo = (double *)malloc(sizeof(double) * 2 * d), *hi = lo + d;
	FILE *bf = fopen(argv[2], "r");
	if (!bf) return 5;
	for (size_t j = 0; j < d; j++) if (fscanf(bf, "%lf %lf", &lo[j], &hi[j]) != 2) return 5;
	fclose(bf);
	double *grid = (double *)malloc(sizeof(double) * ng);
	for (size_t j = 0; j < d; j++)
		for (int k = 0; k < G; k++) grid[j * G + k] = G > 1 ? lo[j] + k * (hi[j] - lo[j]) / (G - 1) : 0.5 * (lo[j] + hi[j]);
	multi_emulator *emu = alloc_multi_emulator(model);
	char tag[48];
	double *s = (double *)malloc(sizeof(double) * (2 + 2 * d)), *a = (double *)malloc(sizeof(double) * 2 * d), *b = a + d;
	double *mv = (double *)malloc(sizeof(double) * 2 * ng), *vv = mv + ng;
	for (size_t c = 0; c < nr; c++) {
		emulator_struct *e = emu->emu_struct_array[c];
		double e0, var, ve0, imse, evar;
		emulate_sensitivity_post(e, lo, hi, s);
		snprintf(tag, sizeof tag, "comp %zu", c);
		row(tag, s, 2 + 2 * d);
		emulate_sensitivity(e, lo, hi, &e0, &var, a, b);
		printf("cplug %zu %.17g %.17g\n", c, e0, var);
		snprintf(tag, sizeof tag, "cfirst %zu", c);
		row(tag, a, d);
		snprintf(tag, sizeof tag, "ctotal %zu", c);
		row(tag, b, d);
		emulate_sensitivity_uncertainty(e, lo, hi, &ve0, &imse, &evar, a, b);
		printf("cunc %zu %.17g %.17g %.17g\n", c, ve0, imse, evar);
		snprintf(tag, sizeof tag, "cefirst %zu", c);
		row(tag, a, d);
		snprintf(tag, sizeof tag, "cetotal %zu", c);
		row(tag, b, d);
		emulate_main_effects_var(e, lo, hi, G, grid, &e0, mv, vv, &ve0);
		for (size_t j = 0; j < d; j++) {
			snprintf(tag, sizeof tag, "cvar %zu %zu", c, j);
			row(tag, vv + j * G, (size_t)G);
		}
		printf("cvare0 %zu %.17g\n", c, ve0);
	}
	double *e0 = (double *)malloc(sizeof(double) * 6 * nout), *var = e0 + nout, *ve0 = var + nout, *imse = ve0 + nout, *evar = imse + nout,
	       *e0m = evar + nout;
	double *f = (double *)malloc(sizeof(double) * 4 * nout * d), *t = f + nout * d, *ef = t + nout * d, *et = ef + nout * d;
	double *mainv = (double *)malloc(sizeof(double) * 2 * ng * nout), *sdv = mainv + ng * nout, *curve = (double *)malloc(sizeof(double) * (size_t)G);
	emulate_sensitivity_multi(emu, pca, lo, hi, e0, var, f, t);
	emulate_sensitivity_uncertainty_multi(emu, pca, lo, hi, ve0, imse, evar, ef, et);
	emulate_main_effects_band_multi(emu, pca, lo, hi, G, grid, e0m, mainv, sdv);
	for (size_t o = 0; o < nout; o++) {
		printf("plug %zu %.17g %.17g\n", o, e0[o], var[o]);
		snprintf(tag, sizeof tag, "pfirst %zu", o);
		row(tag, f + o * d, d);
		snprintf(tag, sizeof tag, "ptotal %zu", o);
		row(tag, t + o * d, d);
		printf("unc %zu %.17g %.17g %.17g\n", o, ve0[o], imse[o], evar[o]);
		snprintf(tag, sizeof tag, "efirst %zu", o);
		row(tag, ef + o * d, d);
		snprintf(tag, sizeof tag, "etotal %zu", o);
		row(tag, et + o * d, d);
		for (size_t j = 0; j < d; j++) {
			for (int k = 0; k < G; k++) curve[k] = mainv[(j * G + k) * nout + o];
			snprintf(tag, sizeof tag, "main %zu %zu", o, j);
			row(tag, curve, (size_t)G);
			for (int k = 0; k < G; k++) curve[k] = sdv[(j * G + k) * nout + o];
			snprintf(tag, sizeof tag, "sd %zu %zu", o, j);
			row(tag, curve, (size_t)G);
		}
		printf("e0main %zu %.17g\n", o, e0m[o]);
	}
	free(lo); free(grid); free(s); free(a); free(mv); free(e0); free(f); free(mainv); free(curve);
	free_multi_emulator(emu);
	return 0;
}
