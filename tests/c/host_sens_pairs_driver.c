/* Drives the second-order entries of the host-side libEmu mirror (csrc/host/libemu.h: emulate_sensitivity_pairs, its enqueue /
 * collect pair, emulate_sensitivity_pairs_post, emulate_sensitivity_pairs_uncertainty, emulate_interaction_surface and the three
 * _multi forms) and prints the results for tests/test_host_sens_pairs.py.  BOX_FILE holds one line "lo hi" per parameter; the
 * surface is that of parameters J and K on G equally spaced values each.
 *
 *   host_sens_pairs_driver MODEL_SNAPSHOT_FILE BOX_FILE G pca_space J K
 *       per PCA component c: "cpair c ..", "cinter c ..", "cspair c ..", "cevpair c ..", "ceinter c ..", "ce0 c v",
 *           "cjoint c a .." and "cfx c a .." per grid value a of parameter J; per pair of components "xpair c c2 .."
 *       per output t: "vpair t ..", "inter t ..", "evpair t ..", "einter t ..", "e0 t v", "joint t a ..", "fx t a .."
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
	if (argc != 7) return 2;
	FILE *fp = fopen(argv[1], "r");
	if (!fp) return 3;
	const int G = atoi(argv[3]), pca = atoi(argv[4]), J = atoi(argv[5]), K = atoi(argv[6]);
	multi_modelstruct *model = load_multi_modelstruct(fp);
	fclose(fp);
	const size_t d = (size_t)model->nparams, nr = (size_t)model->nr, nout = pca ? nr : (size_t)model->nt, np = d * (d - 1) / 2;
	const size_t gg = (size_t)G * G;
	double *lo = (double *)malloc(sizeof(double) * 2 * d), *hi = lo + d;
	FILE *bf = fopen(argv[2], "r");
	if (!bf) return 5;
	for (size_t j = 0; j < d; j++) if (fscanf(bf, "%lf %lf", &lo[j], &hi[j]) != 2) return 5;
	fclose(bf);
	double *gj = (double *)malloc(sizeof(double) * 2 * (size_t)G), *gk = gj + G;
	for (int g = 0; g < G; g++) {
		gj[g] = G > 1 ? lo[J] + g * (hi[J] - lo[J]) / (G - 1) : 0.5 * (lo[J] + hi[J]);
		gk[g] = G > 1 ? lo[K] + g * (hi[K] - lo[K]) / (G - 1) : 0.5 * (lo[K] + hi[K]);
	}
	multi_emulator *emu = alloc_multi_emulator(model);
	char tag[48];
	double *a = (double *)malloc(sizeof(double) * 2 * np), *b = a + np;
	double *jt = (double *)malloc(sizeof(double) * 2 * gg), *fx = jt + gg, *line = (double *)malloc(sizeof(double) * (size_t)G);
	for (size_t c = 0; c < nr; c++) {
		emulator_struct *e = emu->emu_struct_array[c];
		double e0;
		emulate_sensitivity_pairs(e, lo, hi, a, b);
		snprintf(tag, sizeof tag, "cpair %zu", c);
		row(tag, a, np);
		snprintf(tag, sizeof tag, "cinter %zu", c);
		row(tag, b, np);
		emulate_sensitivity_pairs_post(e, lo, hi, a);
		snprintf(tag, sizeof tag, "cspair %zu", c);
		row(tag, a, np);
		emulate_sensitivity_pairs_uncertainty(e, lo, hi, a, b);
		snprintf(tag, sizeof tag, "cevpair %zu", c);
		row(tag, a, np);
		snprintf(tag, sizeof tag, "ceinter %zu", c);
		row(tag, b, np);
		emulate_interaction_surface(e, lo, hi, J, K, G, gj, gk, &e0, jt, fx);
		printf("ce0 %zu %.17g\n", c, e0);
		for (int g = 0; g < G; g++) {
			snprintf(tag, sizeof tag, "cjoint %zu %d", c, g);
			row(tag, jt + (size_t)g * G, (size_t)G);
			snprintf(tag, sizeof tag, "cfx %zu %d", c, g);
			row(tag, fx + (size_t)g * G, (size_t)G);
		}
		for (size_t c2 = c; c2 < nr; c2++) {
			void *dev = NULL;
			emulate_sensitivity_pairs_enqueue(e, emu->emu_struct_array[c2], lo, hi, &dev);
			emulate_sensitivity_pairs_collect(e, dev, a);
			snprintf(tag, sizeof tag, "xpair %zu %zu", c, c2);
			row(tag, a, np);
		}
	}
	double *vp = (double *)malloc(sizeof(double) * 4 * nout * np), *in = vp + nout * np, *ev = in + nout * np, *ei = ev + nout * np;
	double *e0 = (double *)malloc(sizeof(double) * nout), *jo = (double *)malloc(sizeof(double) * 2 * gg * nout), *fo = jo + gg * nout;
	emulate_sensitivity_pairs_multi(emu, pca, lo, hi, vp, in);
	emulate_sensitivity_pairs_uncertainty_multi(emu, pca, lo, hi, ev, ei);
	emulate_interaction_surface_multi(emu, pca, lo, hi, J, K, G, gj, gk, e0, jo, fo);
	for (size_t o = 0; o < nout; o++) {
		snprintf(tag, sizeof tag, "vpair %zu", o);
		row(tag, vp + o * np, np);
		snprintf(tag, sizeof tag, "inter %zu", o);
		row(tag, in + o * np, np);
		snprintf(tag, sizeof tag, "evpair %zu", o);
		row(tag, ev + o * np, np);
		snprintf(tag, sizeof tag, "einter %zu", o);
		row(tag, ei + o * np, np);
		printf("e0 %zu %.17g\n", o, e0[o]);
		for (int g = 0; g < G; g++) {
			for (int h = 0; h < G; h++) line[h] = jo[((size_t)g * G + h) * nout + o];
			snprintf(tag, sizeof tag, "joint %zu %d", o, g);
			row(tag, line, (size_t)G);
			for (int h = 0; h < G; h++) line[h] = fo[((size_t)g * G + h) * nout + o];
			snprintf(tag, sizeof tag, "fx %zu %d", o, g);
			row(tag, line, (size_t)G);
		}
	}
	free(lo); free(gj); free(a); free(jt); free(line); free(vp); free(e0); free(jo);
	free_multi_emulator(emu);
	return 0;
}
