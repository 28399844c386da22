// drives emulator::QueryEmulatorLogLikelihoodGradient:
//   emupp_calib_grad_driver SNAPSHOT QUERY_FILE OBS_FILE      (OBS_FILE as host_calib_driver's)
// per query the lines "ll logpdf" and "grad g_0 .. g_{d-1}"
#include "EmuPlusPlus.h"
#include <cstdio>
#include <fstream>
int main(int argc, char **argv)
{
	if (argc != 4) return 2;
	emulator emu(argv[1]);
	std::ifstream in(argv[2]);
	std::vector<std::vector<double> > pts;
	std::vector<double> p(emu.number_params);
	for (;;) {
		int k = 0;
		for (; k < emu.number_params && (in >> p[k]); k++) {}
		if (k < emu.number_params) break;
		pts.push_back(p);
	}
	std::ifstream ob(argv[3]);
	int full = 0, hasrel = 0;
	if (!(ob >> full >> hasrel)) return 3;
	const size_t nt = (size_t)emu.number_outputs;
	std::vector<double> z(nt), sd, cov, rel;
	for (size_t t = 0; t < nt; t++) ob >> z[t];
	std::vector<double> &s = full ? cov : sd;
	s.resize(full ? nt * nt : nt);
	for (size_t i = 0; i < s.size(); i++) ob >> s[i];
	if (hasrel) { rel.resize(nt); for (size_t t = 0; t < nt; t++) ob >> rel[t]; }
	if (!ob) return 4;
	emu.SetObservations(z, sd, cov, rel);
	std::vector<double> ll;
	std::vector<std::vector<double> > g;
	emu.QueryEmulatorLogLikelihoodGradient(pts, ll, g);
	if (ll.size() != pts.size() || g.size() != pts.size()) return 5;
	for (size_t q = 0; q < pts.size(); q++) {
		printf("ll %.17g\ngrad", ll[q]);
		for (size_t j = 0; j < g[q].size(); j++) printf(" %.17g", g[q][j]);
		printf("\n");
	}
	return 0;
}
