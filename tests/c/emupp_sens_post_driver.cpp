// drives emulator::QueryEmulatorSensitivityUncertainty and emulator::QueryEmulatorMainEffectBands:
//   emupp_sens_post_driver SNAPSHOT BOX_FILE G [pca]
// BOX_FILE: one line "lo hi" per parameter; the grid is G equally spaced values from lo to hi per parameter.
// per output t the lines "unc t var_e0 imse evar", "efirst t ...", "etotal t ..." (variance units), "main t j ..." and "sd t j ..."
// per parameter and "e0main t v": the tags of host_sens_post_driver.c
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
	std::vector<double> ve0, imse, evar, e0m;
	std::vector<std::vector<double> > efirst, etotal, grid(d, std::vector<double>(G));
	std::vector<std::vector<std::vector<double> > > curves, bands;
	for (int j = 0; j < d; j++)
		for (int k = 0; k < G; k++) grid[j][k] = G > 1 ? lo[j] + k * (hi[j] - lo[j]) / (G - 1) : 0.5 * (lo[j] + hi[j]);
	emu.QueryEmulatorSensitivityUncertainty(lo, hi, ve0, imse, evar, efirst, etotal);
	emu.QueryEmulatorMainEffectBands(lo, hi, grid, e0m, curves, bands);
	if ((int)ve0.size() != emu.number_outputs || (int)bands.size() != emu.number_outputs) return 4;
	for (int t = 0; t < emu.number_outputs; t++) {
		printf("unc %d %.17g %.17g %.17g\n", t, ve0[t], imse[t], evar[t]);
		row("efirst", t, -1, efirst[t]);
		row("etotal", t, -1, etotal[t]);
		for (int j = 0; j < d; j++) {
			row("main", t, j, curves[t][j]);
			row("sd", t, j, bands[t][j]);
		}
		printf("e0main %d %.17g\n", t, e0m[t]);
	}
	return 0;
}
