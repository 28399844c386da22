// drives emulator::ValidateHoldout and emulator::DrawEmulator: emupp_joint_driver SNAPSHOT QUERY_FILE Y_FILE Z_FILE [pca]
// Y_FILE: np x nt observations; Z_FILE: nr x ndraw x np normals.  Per query the lines "m", "v", "w" (nr numbers); per component
// "stat c maha logdet logpdf"; "sum L"; per draw s the lines "draw s" (one per query, number_outputs numbers)
#include "EmuPlusPlus.h"
#include <cstdio>
#include <fstream>
static void row(const char *tag, const double *v, size_t n)
{
	printf("%s", tag);
	for (size_t i = 0; i < n; i++) printf(" %.17g", v[i]);
	printf("\n");
}
static std::vector<std::vector<double> > read_rows(const char *name, size_t width)
{
	std::ifstream in(name);
	std::vector<std::vector<double> > rows;
	std::vector<double> p(width);
	for (;;) {
		size_t k = 0;
		for (; k < width && (in >> p[k]); k++) {}
		if (k < width) break;
		rows.push_back(p);
	}
	return rows;
}
int main(int argc, char **argv)
{
	if (argc < 5) return 2;
	emulator emu(argv[1], argc > 5);
	std::vector<double> evals, pmean;
	std::vector<std::vector<double> > evecs;
	emu.getEmulatorPCA(&evals, &evecs, &pmean);
	const size_t nr = evals.size(), nt = pmean.size();
	std::vector<std::vector<double> > pts = read_rows(argv[2], emu.number_params), obs = read_rows(argv[3], nt);
	const size_t np = pts.size();
	if (obs.size() != np) return 3;
	std::vector<std::vector<double> > zrows = read_rows(argv[4], np);
	if (zrows.empty() || zrows.size() % nr) return 4;
	const size_t nd = zrows.size() / nr;
	std::vector<std::vector<std::vector<double> > > normals(nr), draws;
	for (size_t c = 0; c < nr; c++) normals[c].assign(zrows.begin() + c * nd, zrows.begin() + (c + 1) * nd);
	std::vector<std::vector<double> > m, v, w;
	std::vector<double> maha, logdet, logpdf;
	const double sum = emu.ValidateHoldout(pts, obs, m, v, w, maha, logdet, logpdf);
	if (m.size() != np || maha.size() != nr) return 5;
	for (size_t q = 0; q < np; q++) {
		row("m", m[q].data(), nr);
		row("v", v[q].data(), nr);
		row("w", w[q].data(), nr);
	}
	for (size_t c = 0; c < nr; c++) printf("stat %d %.17g %.17g %.17g\n", (int)c, maha[c], logdet[c], logpdf[c]);
	printf("sum %.17g\n", sum);
	emu.DrawEmulator(pts, normals, draws);
	if (draws.size() != nd) return 6;
	for (size_t s = 0; s < nd; s++) {
		char tag[32];
		snprintf(tag, sizeof tag, "draw %d", (int)s);
		for (size_t q = 0; q < np; q++) row(tag, draws[s][q].data(), draws[s][q].size());
	}
	return 0;
}
