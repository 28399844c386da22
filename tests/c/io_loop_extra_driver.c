/* Drives gpemu_host_interactive_loop_extra (csrc/host/interactive_io.c) with stand-ins for the device stage, without a GPU:
 *   io_loop_extra_driver D NOUT NPRINT BINARY NEXTRA
 * mean_i = (i + 1) * sum_k x_k, variance_i = x_0 * x_0 + i (the stand-in of io_loop_driver.c); extra_e = (e + 1) * x_0 - sum_k x_k.
 * NEXTRA = 0 passes no extra function.  stderr: "stats points batches max_batch". */
#include <stdio.h>
#include <stdlib.h>
#include <unistd.h>
#include "libemu.h"

struct fake { int d, nout, nextra; };

static void fake_points(void *user, int np, const double *pts, double *mean, double *var)
{
	const struct fake *f = (const struct fake *)user;
	for (int q = 0; q < np; q++) {
		double s = 0.0;
		for (int k = 0; k < f->d; k++) s += pts[(size_t)q * f->d + k];
		for (int i = 0; i < f->nout; i++) {
			mean[(size_t)q * f->nout + i] = (double)(i + 1) * s;
			var[(size_t)q * f->nout + i] = pts[(size_t)q * f->d] * pts[(size_t)q * f->d] + (double)i;
		}
	}
}

static void fake_extra(void *user, int np, const double *pts, double *extra)
{
	const struct fake *f = (const struct fake *)user;
	for (int q = 0; q < np; q++) {
		double s = 0.0;
		for (int k = 0; k < f->d; k++) s += pts[(size_t)q * f->d + k];
		for (int e = 0; e < f->nextra; e++) extra[(size_t)q * f->nextra + e] = (double)(e + 1) * pts[(size_t)q * f->d] - s;
	}
}

int main(int argc, char **argv)
{
	if (argc != 6) return 2;
	struct fake f = {atoi(argv[1]), atoi(argv[2]), atoi(argv[5])};
	struct gpemu_io_stats st = {0};
	const int rc = gpemu_host_interactive_loop_extra(STDIN_FILENO, STDOUT_FILENO, f.d, f.nout, atoi(argv[3]), atoi(argv[4]), fake_points,
	                                                 f.nextra, f.nextra ? fake_extra : NULL, &f, &st);
	fprintf(stderr, "stats %ld %ld %d\n", st.points, st.batches, st.max_batch);
	if (rc == -1) return 3;
	return rc == 0 ? 0 : 1;
}
