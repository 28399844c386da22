// drives emulator::QueryEmulatorMeans beside QueryEmulator: emupp_mean_driver SNAPSHOT QUERY_FILE [pca]
// one line "q" per query: per output "mean mean_only"
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
	std::vector<std::vector<double> > only, mm, ee;
	emu.QueryEmulatorMeans(pts, only);
	emu.QueryEmulator(pts, mm, ee);
	if (only.size() != pts.size()) return 3;
	for (size_t q = 0; q < pts.size(); q++) {
		if (only[q].size() != mm[q].size()) return 3;
		printf("q");
		for (size_t i = 0; i < mm[q].size(); i++) printf(" %.17g %.17g", mm[q][i], only[q][i]);
		printf("\n");
	}
	return 0;
}
