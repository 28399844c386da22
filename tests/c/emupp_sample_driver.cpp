// Drives emulator::SamplePosterior (csrc/host/EmuPlusPlus.h), for tests/test_host_sample.py.
//
//   emupp_sample_driver MODEL_SNAPSHOT_FILE OBS_FILE PRIOR_FILE X0_FILE W nsteps burn thin seed a
//       the arguments and the lines "nrec", "accept", "trace", "summary" of tests/c/host_sample_driver.c
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>
#include "EmuPlusPlus.h"

int main(int argc, char **argv)
{
	if (argc != 11) return 2;
	emulator emu(argv[1]);
	const int nt = emu.number_outputs, d = emu.number_params;
	std::vector<double> z(nt), sd(nt), lo(d), hi(d);
	std::vector<int> kind(d);
	std::ifstream obs(argv[2]);
	for (int t = 0; t < nt; t++) obs >> z[t];
	for (int t = 0; t < nt; t++) obs >> sd[t];
	std::ifstream pr(argv[3]);
	for (int j = 0; j < d; j++) pr >> kind[j] >> lo[j] >> hi[j];
	if (!obs || !pr) return 4;
	const int W = atoi(argv[5]);
	std::vector<std::vector<double> > starts;
	if (strcmp(argv[4], "-")) {
		std::ifstream xf(argv[4]);
		starts.assign(W, std::vector<double>(d));
		for (int k = 0; k < W; k++) for (int j = 0; j < d; j++) xf >> starts[k][j];
		if (!xf) return 6;
	}
	emu.SetObservations(z, sd, std::vector<double>(), std::vector<double>());
	std::vector<std::vector<double> > samples, summary;
	std::vector<double> lp;
	const double accept = emu.SamplePosterior(lo, hi, kind, W, atoi(argv[6]), atoi(argv[7]), atoi(argv[8]), strtoull(argv[9], NULL, 0),
	                                          atof(argv[10]), starts, samples, lp, summary);
	printf("nrec %zu\naccept %.17g\n", samples.size() / (size_t)W, accept);
	for (size_t r = 0; r < samples.size(); r++) {
		printf("trace");
		for (int j = 0; j < d; j++) printf(" %.17g", samples[r][j]);
		printf(" %.17g\n", lp[r]);
	}
	for (size_t s = 0; s < summary.size(); s++) {
		printf("summary");
		for (int j = 0; j < d; j++) printf(" %.17g", summary[s][j]);
		printf("\n");
	}
	return 0;
}
