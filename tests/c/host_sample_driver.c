/* Drives the posterior sampler of the host-side libEmu mirror (csrc/host/libemu.h: emulate_sample_posterior_multi,
 * gpemu_host_sample_starts, gpemu_host_calib_sample), for tests/test_host_sample.py.
 *
 *   host_sample_driver MODEL_SNAPSHOT_FILE OBS_FILE PRIOR_FILE X0_FILE W nsteps burn thin seed a
 *       OBS_FILE: nt values z, then nt standard deviations.  PRIOR_FILE: per parameter "kind lo hi" (kind 0 uniform, 1 Gaussian
 *       with mean lo and sd hi).  X0_FILE: W x d starts, or "-": the default starts.
 *       Lines: "nrec n"; "accept f"; per walker "start .." (the starts the run used; for "-" what gpemu_host_sample_starts
 *       gives); per recorded sample "trace x_0 .. x_{d-1} lp"; "summary .." six rows of d; "end .." per walker; "same n": how
 *       many of {trace, log posteriors, end state} differ in any bit between the entry, a second call of it, and the
 *       library's run called through gpemu_host_calib_sample with the same starts (0 expected).
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "libemu.h"

static double *vec(size_t n) { return (double *)malloc(sizeof(double) * (n ? n : 1)); }
static int read_vec(FILE *in, double *v, size_t n)
{
	for (size_t i = 0; i < n; i++) if (fscanf(in, "%lf", v + i) != 1) return 0;
	return 1;
}
static void print_rows(const char *tag, const double *v, size_t rows, int n)
{
	for (size_t i = 0; i < rows; i++) {
		printf("%s", tag);
		for (int j = 0; j < n; j++) printf(" %.17g", v[i * (size_t)n + j]);
		printf("\n");
	}
}

int main(int argc, char **argv)
{
	if (argc != 11) return 2;
	FILE *in = fopen(argv[1], "r");
	if (!in) return 3;
	multi_modelstruct *model = load_multi_modelstruct(in);
	fclose(in);
	const int nt = model->nt, d = model->nparams;
	double *z = vec(nt), *sd = vec(nt), *lo = vec(d), *hi = vec(d);
	int *kind = (int *)calloc((size_t)d, sizeof(int));
	in = fopen(argv[2], "r");
	if (!in || !read_vec(in, z, nt) || !read_vec(in, sd, nt)) return 4;
	fclose(in);
	in = fopen(argv[3], "r");
	if (!in) return 5;
	for (int j = 0; j < d; j++) if (fscanf(in, "%d %lf %lf", &kind[j], &lo[j], &hi[j]) != 3) return 5;
	fclose(in);
	gpemu_host_sample_args args = {atoi(argv[5]), atoi(argv[6]), atoi(argv[7]), atoi(argv[8]), strtoull(argv[9], NULL, 0), 0ull, atof(argv[10])};
	const int W = args.nwalkers;
	const size_t wd = (size_t)W * d, nrec = (size_t)gpemu_host_sample_nrec(&args);
	double *x0 = vec(wd);
	const int given = strcmp(argv[4], "-") != 0;
	if (given) {
		in = fopen(argv[4], "r");
		if (!in || !read_vec(in, x0, wd)) return 6;
		fclose(in);
	} else gpemu_host_sample_starts(args.seed, W, d, kind, lo, hi, x0);

	multi_emulator *emu = alloc_multi_emulator(model);
	gpemu_observations *obs = alloc_observations(model, z, sd, NULL, NULL);
	double *tx = vec(nrec * wd), *tl = vec(nrec * W), *xe = vec(wd), *sm = vec(6 * (size_t)d), accept = -1.0;
	emulate_sample_posterior_multi(emu, obs, lo, hi, kind, &args, given ? x0 : NULL, tx, tl, xe, &accept, sm);
	printf("nrec %zu\naccept %.17g\n", nrec, accept);
	print_rows("start", x0, (size_t)W, d);
	for (size_t r = 0; r < nrec * W; r++) {
		printf("trace");
		for (int j = 0; j < d; j++) printf(" %.17g", tx[r * d + j]);
		printf(" %.17g\n", tl[r]);
	}
	print_rows("summary", sm, 6, d);
	print_rows("end", xe, (size_t)W, d);

	int bad = 0;
	double *tx2 = vec(nrec * wd), *tl2 = vec(nrec * W), *xe2 = vec(wd), *lpe = vec(W), acc2 = -1.0;
	int *nacc = (int *)malloc(sizeof(int) * (size_t)W), nrec2 = -1;
	emulate_sample_posterior_multi(emu, obs, lo, hi, kind, &args, given ? x0 : NULL, tx2, tl2, xe2, &acc2, NULL);
	bad += memcmp(tx, tx2, sizeof(double) * nrec * wd) != 0 || memcmp(tl, tl2, sizeof(double) * nrec * W) != 0;
	bad += memcmp(xe, xe2, sizeof(double) * wd) != 0 || acc2 != accept;
	memset(tx2, 0, sizeof(double) * nrec * wd); memset(tl2, 0, sizeof(double) * nrec * W); memset(xe2, 0, sizeof(double) * wd);
	gpemu_host_calib_sample(obs, emu->emu_struct_array, emu->nr, d, kind, lo, hi, &args, x0, tx2, tl2, xe2, lpe, nacc, &nrec2);
	bad += (size_t)nrec2 != nrec || memcmp(tx, tx2, sizeof(double) * nrec * wd) != 0 || memcmp(tl, tl2, sizeof(double) * nrec * W) != 0;
	bad += memcmp(xe, xe2, sizeof(double) * wd) != 0;
	double s = 0.0;
	for (int k = 0; k < W; k++) s += nacc[k];
	bad += s / ((double)W * args.nsteps) != accept;
	printf("same %d\n", bad);
	free_observations(obs);
	free_multi_emulator(emu);
	return 0;
}
