// drives emulator::QueryEmulatorSensitivity and emulator::QueryEmulatorMainEffects: emupp_sens_driver SNAPSHOT BOX_FILE G [pca]
// BOX_FILE: one line "lo hi" per parameter; the grid is G equally spaced values from lo to hi per parameter.
// per output t the lines "out t e0 var", "first t ..." and "total t ..." (the INDICES V_j / V and VT_j / V), "main t j ..." per
// parameter and "e0main t v"
#include "EmuPlusPlus.h"
#include <cstdio>
#include <fstream>
static void row(const char *tag, int t, int j, const std::vector<double> &v)
{
	printf("%s %d", tag, t);
	if (j >= 0) printf(" %d", j);
	for (size_t i = 0; i < v.size(); i++) printf(" %.17g", v[i]);
	printf("\n");
}
int main(int argc, char **argv)
{
	if (argc < 4) return 2;
	emulator emu(argv[1], argc > 4);
	const int d = emu.number_params, G = atoi(argv[3]);
	std::ifstream in(argv[2]);
	std::vector<double> lo(d), hi(d);
	for (int j = 0; j < d; j++)
		if (!(in >> lo[j] >> hi[j])) return 3;
	std::vector<double> e0, var, e0m;
	std::vector<std::vector<double> > first, total, grid(d, std::vector<double>(G));
	std::vector<std::vector<std::vector<double> > > curves;
	for (int j = 0; j < d; j++)
		for (int k = 0; k < G; k++) grid[j][k] = G > 1 ? lo[j] + k * (hi[j] - lo[j]) / (G - 1) : 0.5 * (lo[j] + hi[j]);
	emu.QueryEmulatorSensitivity(lo, hi, e0, var, first, total);
	emu.QueryEmulatorMainEffects(lo, hi, grid, e0m, curves);
	if ((int)e0.size() != emu.number_outputs || (int)curves.size() != emu.number_outputs) return 4;
	for (int t = 0; t < emu.number_outputs; t++) {
		printf("out %d %.17g %.17g\n", t, e0[t], var[t]);
		row("first", t, -1, first[t]);
		row("total", t, -1, total[t]);
		for (int j = 0; j < d; j++) row("main", t, j, curves[t][j]);
		printf("e0main %d %.17g\n", t, e0m[t]);
	}
	return 0;
}
