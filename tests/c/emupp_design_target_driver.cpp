// drives emulator::QueryEmulatorTargetedDesignGain: emupp_design_target_driver SNAPSHOT TARGETS_FILE POINTS_FILE [pca]
// TARGETS_FILE: the targets, number_params numbers and a weight per line; POINTS_FILE: the candidates, number_params numbers each.
// per candidate q the lines "gain q" with one value per output and "total q v", then "tv 0" with one value per output
#include "EmuPlusPlus.h"
#include <cstdio>
#include <fstream>
int main(int argc, char **argv)
{
	if (argc < 4) return 2;
	emulator emu(argv[1], argc > 4);
	const int d = emu.number_params;
	std::ifstream tf(argv[2]);
	std::vector<std::vector<double> > targets, pts;
	std::vector<double> weights, p(d);
	for (;;) {
		int j = 0;
		double w;
		while (j < d && (tf >> p[j])) j++;
		if (j < d || !(tf >> w)) break;
		targets.push_back(p);
		weights.push_back(w);
	}
	std::ifstream pf(argv[3]);
	for (;;) {
		int j = 0;
		while (j < d && (pf >> p[j])) j++;
		if (j < d) break;
		pts.push_back(p);
	}
	std::vector<std::vector<double> > gains;
	std::vector<double> total, tv;
	emu.QueryEmulatorTargetedDesignGain(targets, weights, pts, gains, total, tv);
	if (gains.size() != pts.size() || total.size() != pts.size()) return 4;
	for (size_t q = 0; q < pts.size(); q++) {
		printf("gain %zu", q);
		for (size_t t = 0; t < gains[q].size(); t++) printf(" %.17g", gains[q][t]);
		printf("\ntotal %zu %.17g\n", q, total[q]);
	}
	printf("tv 0");
	for (size_t t = 0; t < tv.size(); t++) printf(" %.17g", tv[t]);
	printf("\n");
	return 0;
}
