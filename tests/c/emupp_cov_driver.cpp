// drives emulator::QueryEmulatorCovariance beside QueryEmulator: emupp_cov_driver SNAPSHOT QUERY_FILE [pca]
// per query the lines "m" (means) and "e" (QueryEmulator's errors); per output o the lines "c o" (its matrix, one line per row)
#include "EmuPlusPlus.h"
#include <cstdio>
#include <fstream>
static void row(const char *tag, const double *v, size_t n)
{
	printf("%s", tag);
	for (size_t i = 0; i < n; i++) printf(" %.17g", v[i]);
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
	const size_t np = pts.size();
	std::vector<std::vector<double> > m, c, mm, ee;
	emu.QueryEmulatorCovariance(pts, m, c);
	if (m.size() != np || (int)c.size() != emu.number_outputs) return 3;
	emu.QueryEmulator(pts, mm, ee);
	for (size_t q = 0; q < np; q++) {
		row("m", m[q].data(), m[q].size());
		row("e", ee[q].data(), ee[q].size());
	}
	for (int o = 0; o < emu.number_outputs; o++) {
		if (c[o].size() != np * np) return 4;
		char tag[32];
		snprintf(tag, sizeof tag, "c %d", o);
		for (size_t q = 0; q < np; q++) row(tag, c[o].data() + q * np, np);
	}
	return 0;
}
