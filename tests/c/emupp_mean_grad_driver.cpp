// drives emulator::QueryEmulatorMeanGradients beside QueryEmulatorMeans: emupp_mean_grad_driver SNAPSHOT QUERY_FILE [pca]
// per query a line "m" (means of QueryEmulatorMeanGradients, then of QueryEmulatorMeans), a line "g" (gradients, output-major)
// and a line "c" (central differences of QueryEmulatorMeans at h = 1e-5 in the same order)
#include "EmuPlusPlus.h"
#include <cstdio>
#include <fstream>
int main(int argc, char **argv)
{
	if (argc < 3) return 2;
	emulator emu(argv[1], argc > 3);
	std::ifstream in(argv[2]);
	std::vector<std::vector<double> > pts;
	std::vector<double> p(emu.number_params);
	for (;;) {
		int k = 0;
		for (; k < emu.number_params && (in >> p[k]); k++) {}
		if (k < emu.number_params) break;
		pts.push_back(p);
	}
	const double h = 1e-5;
	const int d = emu.number_params;
	std::vector<std::vector<double> > mg, gg, only;
	emu.QueryEmulatorMeanGradients(pts, mg, gg);
	emu.QueryEmulatorMeans(pts, only);
	if (mg.size() != pts.size() || gg.size() != pts.size()) return 3;
	const size_t no = only[0].size();
	std::vector<std::vector<double> > cd(pts.size(), std::vector<double>(no * d));
	for (int j = 0; j < d; j++) {
		std::vector<std::vector<double> > pp(pts), pm(pts), mp, mm;
		for (size_t q = 0; q < pts.size(); q++) { pp[q][j] += h; pm[q][j] -= h; }
		emu.QueryEmulatorMeans(pp, mp);
		emu.QueryEmulatorMeans(pm, mm);
		for (size_t q = 0; q < pts.size(); q++)
			for (size_t i = 0; i < no; i++) cd[q][i * d + j] = (mp[q][i] - mm[q][i]) / (2.0 * h);
	}
	for (size_t q = 0; q < pts.size(); q++) {
		if (mg[q].size() != no || gg[q].size() != no * d) return 3;
		printf("m");
		for (size_t i = 0; i < no; i++) printf(" %.17g", mg[q][i]);
		for (size_t i = 0; i < no; i++) printf(" %.17g", only[q][i]);
		printf("\ng");
		for (size_t i = 0; i < no * d; i++) printf(" %.17g", gg[q][i]);
		printf("\nc");
		for (size_t i = 0; i < no * d; i++) printf(" %.17g", cd[q][i]);
		printf("\n");
	}
	return 0;
}
