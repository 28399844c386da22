// drives emulator::QueryEmulatorGradients beside QueryEmulator: emupp_var_grad_driver SNAPSHOT QUERY_FILE [pca]
// per query the lines "m" (means), "v" (variances), "gm", "gv" (gradients, output-major) and "e" (QueryEmulator's errors)
#include "EmuPlusPlus.h"
#include <cstdio>
#include <fstream>
static void row(const char *tag, const std::vector<double> &v)
{
	printf("%s", tag);
	for (size_t i = 0; i < v.size(); i++) printf(" %.17g", v[i]);
	printf("\n");
}
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
	std::vector<std::vector<double> > m, v, gm, gv;
	emu.QueryEmulatorGradients(pts, m, v, gm, gv);
	if (m.size() != pts.size() || v.size() != pts.size() || gm.size() != pts.size() || gv.size() != pts.size()) return 3;
	for (size_t q = 0; q < pts.size(); q++) {
		std::vector<double> mean, err;
		emu.QueryEmulator(pts[q], mean, err);
		row("m", m[q]);
		row("v", v[q]);
		row("gm", gm[q]);
		row("gv", gv[q]);
		row("e", err);
	}
	return 0;
}
