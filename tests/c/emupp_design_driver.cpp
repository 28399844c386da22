// drives emulator::QueryEmulatorDesignGain: emupp_design_driver SNAPSHOT BOX_FILE POINTS_FILE [pca]
// BOX_FILE: one line "lo hi" per parameter; POINTS_FILE: the candidates, number_params numbers each.
// per candidate q the lines "gain q" with one value per output and "total q v"
#include "EmuPlusPlus.h"
#include <cstdio>
#include <fstream>
int main(int argc, char **argv)
{
	if (argc < 4) return 2;
	emulator emu(argv[1], argc > 4);
	const int d = emu.number_params;
	std::ifstream in(argv[2]);
	std::vector<double> lo(d), hi(d);
	for (int j = 0; j < d; j++)
		if (!(in >> lo[j] >> hi[j])) return 3;
	std::ifstream pf(argv[3]);
	std::vector<std::vector<double> > pts;
	std::vector<double> p(d);
	for (;;) {
		int j = 0;
		while (j < d && (pf >> p[j])) j++;
		if (j < d) break;
		pts.push_back(p);
	}
	std::vector<std::vector<double> > gains;
	std::vector<double> total;
	emu.QueryEmulatorDesignGain(lo, hi, pts, gains, total);
	if (gains.size() != pts.size() || total.size() != pts.size()) return 4;
	for (size_t q = 0; q < pts.size(); q++) {
		printf("gain %zu", q);
		for (size_t t = 0; t < gains[q].size(); t++) printf(" %.17g", gains[q][t]);
		printf("\ntotal %zu %.17g\n", q, total[q]);
	}
	return 0;
}
