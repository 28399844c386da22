/* Drives the greedy-batch entries of the host-side libEmu mirror (csrc/host/libemu.h: emulate_design_batch,
 * emulate_design_batch_multi) and prints the results for tests/test_host_design_batch.py.  BOX_FILE holds one line "lo hi" per
 * parameter, POINTS_FILE the candidates, nparams numbers each.
 *
 *   host_design_batch_driver MODEL_SNAPSHOT_FILE BOX_FILE POINTS_FILE pca_space nbatch
 *       per PCA component c and pick j: "comp c j index gain" (emulate_design_batch on the component alone)
 *       per pick j: "pick j index gain" (emulate_design_batch_multi)
 */
#include <stdio.h>
#include <stdlib.h>
#include "libemu.h"

int main(int argc, char **argv)
{
	if (argc != 6) return 2;
	FILE *fp = fopen(argv[1], "r");
	if (!fp) return 3;
	const int pca = atoi(argv[4]), nbatch = atoi(argv[5]);
	if (nbatch < 1) return 4;
	multi_modelstruct *model = load_multi_modelstruct(fp);
	fclose(fp);
	const size_t d = (size_t)model->nparams, nr = (size_t)model->nr;
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
	int *pick = (int *)malloc(sizeof(int) * (size_t)nbatch);
	double *g = (double *)malloc(sizeof(double) * (size_t)nbatch);
	for (size_t c = 0; c < nr; c++) {
		emulate_design_batch(emu->emu_struct_array[c], lo, hi, (int)np, pts, nbatch, pick, g);
		for (int j = 0; j < nbatch; j++) printf("comp %zu %d %d %.17g\n", c, j, pick[j], g[j]);
	}
	emulate_design_batch_multi(emu, pca, lo, hi, (int)np, pts, nbatch, pick, g);
	for (int j = 0; j < nbatch; j++) printf("pick %d %d %.17g\n", j, pick[j], g[j]);
	free(lo); free(pts); free(pick); free(g);
	free_multi_emulator(emu);
	return 0;
}
