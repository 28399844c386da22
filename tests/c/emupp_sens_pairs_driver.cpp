// drives emulator::QueryEmulatorInteractions, QueryEmulatorInteractionUncertainty and QueryEmulatorInteractionSurface:
//   emupp_sens_pairs_driver SNAPSHOT BOX_FILE G J K [pca]
// BOX_FILE: one line "lo hi" per parameter; the surface is that of parameters J and K on G equally spaced values each.
// per output t the lines "vpair t ..", "second t .." (the indices), "evpair t ..", "einter t ..", "e0 t v", "joint t a .." and
// "fx t a .." per grid value a of parameter J: the tags of host_sens_pairs_driver.c
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
	if (argc < 6) return 2;
	emulator emu(argv[1], argc > 6);
	const int d = emu.number_params, G = atoi(argv[3]), J = atoi(argv[4]), K = atoi(argv[5]);
	std::ifstream in(argv[2]);
	std::vector<double> lo(d), hi(d), gj(G), gk(G), e0;
	for (int j = 0; j < d; j++)
		if (!(in >> lo[j] >> hi[j])) return 3;
	for (int g = 0; g < G; g++) {
		gj[g] = G > 1 ? lo[J] + g * (hi[J] - lo[J]) / (G - 1) : 0.5 * (lo[J] + hi[J]);
		gk[g] = G > 1 ? lo[K] + g * (hi[K] - lo[K]) / (G - 1) : 0.5 * (lo[K] + hi[K]);
	}
	std::vector<std::vector<double> > vpair, second, evpair, einter;
	std::vector<std::vector<std::vector<double> > > joint, fx;
	emu.QueryEmulatorInteractions(lo, hi, vpair, second);
	emu.QueryEmulatorInteractionUncertainty(lo, hi, evpair, einter);
	emu.QueryEmulatorInteractionSurface(lo, hi, J, K, gj, gk, e0, joint, fx);
	if ((int)vpair.size() != emu.number_outputs || (int)joint.size() != emu.number_outputs) return 4;
	for (int t = 0; t < emu.number_outputs; t++) {
		row("vpair", t, -1, vpair[t]);
		row("second", t, -1, second[t]);
		row("evpair", t, -1, evpair[t]);
		row("einter", t, -1, einter[t]);
		printf("e0 %d %.17g\n", t, e0[t]);
		for (int g = 0; g < G; g++) {
			row("joint", t, g, joint[t][g]);
			row("fx", t, g, fx[t][g]);
		}
	}
	return 0;
}
