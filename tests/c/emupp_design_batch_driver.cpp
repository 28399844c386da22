// drives emulator::QueryEmulatorDesignBatch: emupp_design_batch_driver SNAPSHOT BOX_FILE POINTS_FILE NBATCH [pca]
// BOX_FILE: one line "lo hi" per parameter; POINTS_FILE: the candidates, number_params numbers each.
// per pick j the line "pick j index gain"
#include "EmuPlusPlus.h"
#include <cstdio>
#include <cstdlib>
#include <fstream>
int main(int argc, char **argv)
{
	if (argc < 5) return 2;
	emulator emu(argv[1], argc > 5);
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
	std::vector<int> picks;
	std::vector<double> gains;
	emu.QueryEmulatorDesignBatch(lo, hi, pts, atoi(argv[4]), picks, gains);
	if (picks.size() != gains.size()) return 4;
	for (size_t j = 0; j < picks.size(); j++) printf("pick %zu %d %.17g\n", j, picks[j], gains[j]);
	return 0;
}
