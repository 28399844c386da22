// drives emulator::SetObservations, QueryEmulatorImplausibility and QueryEmulatorNonImplausible:
//   emupp_calib_driver SNAPSHOT QUERY_FILE OBS_FILE cut_chi2 level cut_I      (OBS_FILE and the cuts as host_calib_driver's)
// per query the line "stat chi2 logpdf I1 I2 I3 worst"; "nkeep n" and per kept point "keep idx chi2 logpdf I1 I2 I3"
#include "EmuPlusPlus.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
int main(int argc, char **argv)
{
	if (argc != 7) return 2;
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
	emu.SetObservations(z, sd, cov, rel);                 // a second set replaces the first
	std::vector<std::vector<double> > st, kst;
	std::vector<int> worst, kept;
	emu.QueryEmulatorImplausibility(pts, st, worst);
	if (st.size() != pts.size() || worst.size() != pts.size()) return 5;
	for (size_t q = 0; q < st.size(); q++)
		printf("stat %.17g %.17g %.17g %.17g %.17g %d\n", st[q][0], st[q][1], st[q][2], st[q][3], st[q][4], worst[q]);
	const double c2 = !strcmp(argv[4], "inf") ? INFINITY : atof(argv[4]), cI = !strcmp(argv[6], "inf") ? INFINITY : atof(argv[6]);
	emu.QueryEmulatorNonImplausible(pts, c2, atoi(argv[5]), cI, kept, kst);
	if (kept.size() != kst.size()) return 6;
	printf("nkeep %d\n", (int)kept.size());
	for (size_t k = 0; k < kept.size(); k++)
		printf("keep %d %.17g %.17g %.17g %.17g %.17g\n", kept[k], kst[k][0], kst[k][1], kst[k][2], kst[k][3], kst[k][4]);
	return 0;
}
