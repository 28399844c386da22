// drives emulator::SetSensitivityMeasure before emulator::QueryEmulatorSensitivity: emupp_sens_measure_driver SNAPSHOT MEASURE_FILE [pca]
// MEASURE_FILE: one line "kind lo hi" per parameter, kind 0 (uniform on [lo, hi]) or 1 (Gaussian, mean lo, sd hi).
// per output t the lines "out t e0 var", "first t ..." and "total t ..." (the INDICES V_j / V and VT_j / V)
#include "EmuPlusPlus.h"
#include <cstdio>
#include <fstream>
static void row(const char *tag, int t, const std::vector<double> &v)
{
	printf("%s %d", tag, t);
	for (size_t i = 0; i < v.size(); i++) printf(" %.17g", v[i]);
	printf("\n");
}
int main(int argc, char **argv)
{
	if (argc < 3) return 2;
	emulator emu(argv[1], argc > 3);
	const int d = emu.number_params;
	std::ifstream in(argv[2]);
	std::vector<int> kind(d);
	std::vector<double> lo(d), hi(d);
	for (int j = 0; j < d; j++)
		if (!(in >> kind[j] >> lo[j] >> hi[j])) return 3;
	emu.SetSensitivityMeasure(kind);
	std::vector<double> e0, var;
	std::vector<std::vector<double> > first, total;
	emu.QueryEmulatorSensitivity(lo, hi, e0, var, first, total);
	for (int t = 0; t < emu.number_outputs; t++) {
		printf("out %d %.17g %.17g\n", t, e0[t], var[t]);
		row("first", t, first[t]);
		row("total", t, total[t]);
	}
	return 0;
}
