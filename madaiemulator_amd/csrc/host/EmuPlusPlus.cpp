// EmuPlusPlus.cpp -- see EmuPlusPlus.h (reference: src/EmuPlusPlus.cpp:57-235)
#include "EmuPlusPlus.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>

void emulator::init(const std::string &path, bool pca)
{
	outputPCAValues = pca;
	StateFilePath = path;
	FILE *fptr = fopen(path.c_str(), "r");
	if (!fptr) {
		std::cerr << "error opening statefile: " << path << std::endl;
		gpemu_host_exit(EXIT_FAILURE);
	}
	the_model = load_multi_modelstruct(fptr);
	fclose(fptr);
	the_emulator = alloc_multi_emulator(the_model);
	the_observations = NULL;
	number_outputs = pca ? the_model->nr : the_model->nt;
	number_params = the_model->nparams;
}

emulator::emulator(std::string path) { init(path, false); }
emulator::emulator(std::string path, bool PcaOnly) { init(path, PcaOnly); }
emulator::~emulator()
{
	free_observations(the_observations);
	free_multi_emulator(the_emulator);
}

// the one complaint of the Query* methods about a point's length, under the name of the method that was called
static void wrong_dimensions(const char *method)
{
	std::cerr << "Error::" << method << " called with incorrect number of dimensions in xpoint" << std::endl;
}

// xpoints, every row checked to have number_params entries, as packed row-major doubles (the data of the gsl_matrix view)
static std::vector<double> flatten(const char *method, const std::vector<std::vector<double> > &xpoints, int number_params)
{
	std::vector<double> flat(xpoints.size() * number_params);
	for (size_t q = 0; q < xpoints.size(); q++) {
		if ((int)xpoints[q].size() != number_params) {
			wrong_dimensions(method);
			gpemu_host_exit(EXIT_FAILURE);
		}
		for (int k = 0; k < number_params; k++) flat[q * number_params + k] = xpoints[q][k];
	}
	return flat;
}

void emulator::QueryEmulator(const std::vector<std::vector<double> > &xpoints, std::vector<std::vector<double> > &Means,
                             std::vector<std::vector<double> > &Errors)
{
	const size_t np = xpoints.size();
	std::vector<double> m(np * number_outputs), v(np * number_outputs);
	std::vector<double> flat = flatten("QueryEmulator", xpoints, number_params);
	gsl_matrix view = gpemu_matrix_view(flat.data(), np, number_params);
	emulate_points_multi(the_emulator, &view, outputPCAValues ? 1 : 0, m.data(), v.data());
	Means.assign(np, std::vector<double>(number_outputs));
	Errors.assign(np, std::vector<double>(number_outputs));
	for (size_t q = 0; q < np; q++)
		for (int i = 0; i < number_outputs; i++) {
			Means[q][i] = m[q * number_outputs + i];
			Errors[q][i] = sqrt(v[q * number_outputs + i]);      // the reference returns the square root of the variance
		}
}

void emulator::QueryEmulatorMeans(const std::vector<std::vector<double> > &xpoints, std::vector<std::vector<double> > &Means)
{
	const size_t np = xpoints.size();
	std::vector<double> m(np * number_outputs);
	std::vector<double> flat = flatten("QueryEmulatorMeans", xpoints, number_params);
	gsl_matrix view = gpemu_matrix_view(flat.data(), np, number_params);
	emulate_points_multi_mean(the_emulator, &view, outputPCAValues ? 1 : 0, m.data());
	Means.assign(np, std::vector<double>(number_outputs));
	for (size_t q = 0; q < np; q++)
		for (int i = 0; i < number_outputs; i++) Means[q][i] = m[q * number_outputs + i];
}

void emulator::QueryEmulatorMeanGradients(const std::vector<std::vector<double> > &xpoints, std::vector<std::vector<double> > &Means,
                                          std::vector<std::vector<double> > &Gradients)
{
	const size_t np = xpoints.size(), ng = (size_t)number_outputs * number_params;
	std::vector<double> m(np * number_outputs), g(np * ng);
	std::vector<double> flat = flatten("QueryEmulatorMeanGradients", xpoints, number_params);
	gsl_matrix view = gpemu_matrix_view(flat.data(), np, number_params);
	emulate_points_multi_mean_grad(the_emulator, &view, outputPCAValues ? 1 : 0, m.data(), g.data());
	Means.assign(np, std::vector<double>(number_outputs));
	Gradients.assign(np, std::vector<double>(ng));
	for (size_t q = 0; q < np; q++) {
		for (int i = 0; i < number_outputs; i++) Means[q][i] = m[q * number_outputs + i];
		for (size_t i = 0; i < ng; i++) Gradients[q][i] = g[q * ng + i];
	}
}

void emulator::QueryEmulatorGradients(const std::vector<std::vector<double> > &xpoints, std::vector<std::vector<double> > &Means,
                                      std::vector<std::vector<double> > &Variances, std::vector<std::vector<double> > &MeanGradients,
                                      std::vector<std::vector<double> > &VarianceGradients)
{
	const size_t np = xpoints.size(), ng = (size_t)number_outputs * number_params;
	std::vector<double> m(np * number_outputs), v(np * number_outputs), gm(np * ng), gv(np * ng);
	std::vector<double> flat = flatten("QueryEmulatorGradients", xpoints, number_params);
	gsl_matrix view = gpemu_matrix_view(flat.data(), np, number_params);
	emulate_points_multi_grad(the_emulator, &view, outputPCAValues ? 1 : 0, m.data(), v.data(), gm.data(), gv.data());
	Means.assign(np, std::vector<double>(number_outputs));
	Variances.assign(np, std::vector<double>(number_outputs));
	MeanGradients.assign(np, std::vector<double>(ng));
	VarianceGradients.assign(np, std::vector<double>(ng));
	for (size_t q = 0; q < np; q++) {
		for (int i = 0; i < number_outputs; i++) { Means[q][i] = m[q * number_outputs + i]; Variances[q][i] = v[q * number_outputs + i]; }
		for (size_t i = 0; i < ng; i++) { MeanGradients[q][i] = gm[q * ng + i]; VarianceGradients[q][i] = gv[q * ng + i]; }
	}
}

void emulator::QueryEmulatorCovariance(const std::vector<std::vector<double> > &xpoints, std::vector<std::vector<double> > &Means,
                                       std::vector<std::vector<double> > &Covariances)
{
	const size_t np = xpoints.size();
	std::vector<double> m(np * number_outputs), c((size_t)number_outputs * np * np);
	std::vector<double> flat = flatten("QueryEmulatorCovariance", xpoints, number_params);
	gsl_matrix view = gpemu_matrix_view(flat.data(), np, number_params);
	emulate_points_multi_cov(the_emulator, &view, outputPCAValues ? 1 : 0, m.data(), c.data());
	Means.assign(np, std::vector<double>(number_outputs));
	for (size_t q = 0; q < np; q++)
		for (int i = 0; i < number_outputs; i++) Means[q][i] = m[q * number_outputs + i];
	Covariances.assign(number_outputs, std::vector<double>());
	for (int i = 0; i < number_outputs; i++) Covariances[i].assign(c.begin() + (size_t)i * np * np, c.begin() + (size_t)(i + 1) * np * np);
}

void emulator::SetObservations(const std::vector<double> &Values, const std::vector<double> &StandardDeviations,
                               const std::vector<double> &Covariance, const std::vector<double> &RelativeErrors)
{
	const size_t nt = (size_t)the_model->nt;
	const bool cov = !Covariance.empty();
	if (Values.size() != nt || (cov ? Covariance.size() != nt * nt : StandardDeviations.size() != nt)
	    || (!RelativeErrors.empty() && RelativeErrors.size() != nt)) {
		std::cerr << "Error::SetObservations called with vectors that do not match the number of outputs" << std::endl;
		gpemu_host_exit(EXIT_FAILURE);
	}
	free_observations(the_observations);
	the_observations = alloc_observations(the_model, Values.data(), cov ? NULL : StandardDeviations.data(), cov ? Covariance.data() : NULL,
	                                      RelativeErrors.empty() ? NULL : RelativeErrors.data());
}

// the observation set the two calibration methods need
static void need_observations(const char *method, const gpemu_observations *obs)
{
	if (obs) return;
	std::cerr << "Error::" << method << " called before SetObservations" << std::endl;
	gpemu_host_exit(EXIT_FAILURE);
}

void emulator::QueryEmulatorImplausibility(const std::vector<std::vector<double> > &xpoints, std::vector<std::vector<double> > &Statistics,
                                           std::vector<int> &WorstOutput)
{
	need_observations("QueryEmulatorImplausibility", the_observations);
	const size_t np = xpoints.size();
	std::vector<double> st(np * 5 + 1);
	std::vector<double> flat = flatten("QueryEmulatorImplausibility", xpoints, number_params);
	gsl_matrix view = gpemu_matrix_view(flat.data(), np, number_params);
	WorstOutput.assign(np, 0);
	if (np) emulate_points_multi_implausibility(the_emulator, the_observations, &view, st.data(), WorstOutput.data());
	Statistics.assign(np, std::vector<double>(5));
	for (size_t q = 0; q < np; q++)
		for (int s = 0; s < 5; s++) Statistics[q][s] = st[q * 5 + s];
}

void emulator::QueryEmulatorNonImplausible(const std::vector<std::vector<double> > &xpoints, double CutChi2, int Level, double CutI,
                                           std::vector<int> &Kept, std::vector<std::vector<double> > &Statistics)
{
	need_observations("QueryEmulatorNonImplausible", the_observations);
	const size_t np = xpoints.size();
	std::vector<double> st(np * 5 + 1);
	std::vector<double> flat = flatten("QueryEmulatorNonImplausible", xpoints, number_params);
	gsl_matrix view = gpemu_matrix_view(flat.data(), np, number_params);
	Kept.assign(np + 1, 0);
	int nkeep = 0;
	if (np) emulate_points_multi_nonimplausible(the_emulator, the_observations, &view, CutChi2, Level, CutI, Kept.data(), st.data(), &nkeep);
	Kept.resize((size_t)nkeep);
	Statistics.assign((size_t)nkeep, std::vector<double>(5));
	for (int q = 0; q < nkeep; q++)
		for (int s = 0; s < 5; s++) Statistics[q][s] = st[(size_t)q * 5 + s];
}

void emulator::QueryEmulatorLogLikelihoodGradient(const std::vector<std::vector<double> > &xpoints, std::vector<double> &LogLikelihoods,
                                                  std::vector<std::vector<double> > &Gradients)
{
	need_observations("QueryEmulatorLogLikelihoodGradient", the_observations);
	const size_t np = xpoints.size(), d = (size_t)number_params;
	std::vector<double> st(np * 5 + 1), g(np * d + 1);
	std::vector<double> flat = flatten("QueryEmulatorLogLikelihoodGradient", xpoints, number_params);
	gsl_matrix view = gpemu_matrix_view(flat.data(), np, number_params);
	if (np) emulate_points_multi_logpdf_grad(the_emulator, the_observations, &view, st.data(), g.data(), NULL);
	LogLikelihoods.assign(np, 0.0);
	Gradients.assign(np, std::vector<double>(d));
	for (size_t q = 0; q < np; q++) {
		LogLikelihoods[q] = st[q * 5 + 1];
		for (size_t j = 0; j < d; j++) Gradients[q][j] = g[q * d + j];
	}
}

double emulator::SamplePosterior(const std::vector<double> &lo, const std::vector<double> &hi, const std::vector<int> &kind, int Walkers,
                                 int Steps, int Burn, int Thin, unsigned long long Seed, double Stretch,
                                 const std::vector<std::vector<double> > &Starts, std::vector<std::vector<double> > &Samples,
                                 std::vector<double> &LogPosteriors, std::vector<std::vector<double> > &Summary)
{
	need_observations("SamplePosterior", the_observations);
	const size_t d = (size_t)number_params;
	if (lo.size() != d || hi.size() != d || (!kind.empty() && kind.size() != d) || (!Starts.empty() && (int)Starts.size() != Walkers)) {
		std::cerr << "Error::SamplePosterior called with a prior that has not one entry per parameter, or with starts that are not one per walker" << std::endl;
		gpemu_host_exit(EXIT_FAILURE);
	}
	gpemu_host_sample_args args = {Walkers, Steps, Burn, Thin, Seed, 0ull, Stretch};
	const size_t nrec = (size_t)gpemu_host_sample_nrec(&args), W = Walkers > 0 ? (size_t)Walkers : 0;
	std::vector<double> flat = flatten("SamplePosterior", Starts, number_params);
	std::vector<double> tx(nrec * W * d + 1), tl(nrec * W + 1), sm(6 * d);
	double accept = 0.0;
	emulate_sample_posterior_multi(the_emulator, the_observations, lo.data(), hi.data(), kind.empty() ? NULL : kind.data(), &args,
	                               Starts.empty() ? NULL : flat.data(), tx.data(), tl.data(), NULL, &accept, sm.data());
	Samples.assign(nrec * W, std::vector<double>(d));
	for (size_t r = 0; r < nrec * W; r++) Samples[r].assign(tx.begin() + r * d, tx.begin() + (r + 1) * d);
	LogPosteriors.assign(tl.begin(), tl.begin() + nrec * W);
	Summary.assign(6, std::vector<double>(d));
	for (size_t s = 0; s < 6; s++) Summary[s].assign(sm.begin() + s * d, sm.begin() + (s + 1) * d);
	return accept;
}

// the box of the two sensitivity methods, checked to have number_params entries on either side
static void check_box(const char *method, const std::vector<double> &lo, const std::vector<double> &hi, int number_params)
{
	if ((int)lo.size() != number_params || (int)hi.size() != number_params) {
		std::cerr << "Error::" << method << " called with a box that has not one bound pair per parameter" << std::endl;
		gpemu_host_exit(EXIT_FAILURE);
	}
}

void emulator::SetSensitivityMeasure(const std::vector<int> &kind)
{
	if (!kind.empty() && (int)kind.size() != number_params) {
		std::cerr << "Error::SetSensitivityMeasure called with a vector that has not one kind per parameter" << std::endl;
		gpemu_host_exit(EXIT_FAILURE);
	}
	emulate_sensitivity_measure_multi(the_emulator, kind.empty() ? NULL : kind.data());
}

void emulator::QueryEmulatorSensitivity(const std::vector<double> &lo, const std::vector<double> &hi, std::vector<double> &Means,
                                        std::vector<double> &Variances, std::vector<std::vector<double> > &FirstOrder,
                                        std::vector<std::vector<double> > &Total)
{
	check_box("QueryEmulatorSensitivity", lo, hi, number_params);
	const size_t no = (size_t)number_outputs, d = (size_t)number_params;
	std::vector<double> f(no * d), t(no * d);
	Means.assign(no, 0.0);
	Variances.assign(no, 0.0);
	emulate_sensitivity_multi(the_emulator, outputPCAValues ? 1 : 0, lo.data(), hi.data(), Means.data(), Variances.data(), f.data(), t.data());
	FirstOrder.assign(no, std::vector<double>(d));
	Total.assign(no, std::vector<double>(d));
	for (size_t i = 0; i < no; i++)
		for (size_t j = 0; j < d; j++) {
			const double V = Variances[i];
			FirstOrder[i][j] = V != 0.0 ? f[i * d + j] / V : NAN;
			Total[i][j] = V != 0.0 ? t[i * d + j] / V : NAN;
		}
}

void emulator::QueryEmulatorMainEffects(const std::vector<double> &lo, const std::vector<double> &hi, const std::vector<std::vector<double> > &grid,
                                        std::vector<double> &Means, std::vector<std::vector<std::vector<double> > > &Curves)
{
	check_box("QueryEmulatorMainEffects", lo, hi, number_params);
	const size_t no = (size_t)number_outputs, d = (size_t)number_params, G = grid.empty() ? 0 : grid[0].size();
	if (grid.size() != d || G < 1) {
		std::cerr << "Error::QueryEmulatorMainEffects called with a grid that has not one non-empty row per parameter" << std::endl;
		gpemu_host_exit(EXIT_FAILURE);
	}
	std::vector<double> g = flatten("QueryEmulatorMainEffects", grid, (int)G), m(d * G * no);
	Means.assign(no, 0.0);
	emulate_main_effects_multi(the_emulator, outputPCAValues ? 1 : 0, lo.data(), hi.data(), (int)G, g.data(), Means.data(), m.data());
	Curves.assign(no, std::vector<std::vector<double> >(d, std::vector<double>(G)));
	for (size_t i = 0; i < no; i++)
		for (size_t j = 0; j < d; j++)
			for (size_t k = 0; k < G; k++) Curves[i][j][k] = m[(j * G + k) * no + i];
}

void emulator::QueryEmulatorSensitivityUncertainty(const std::vector<double> &lo, const std::vector<double> &hi, std::vector<double> &MeanVariances,
                                                   std::vector<double> &IntegratedVariances, std::vector<double> &ExpectedVariances,
                                                   std::vector<std::vector<double> > &ExpectedFirstOrder,
                                                   std::vector<std::vector<double> > &ExpectedTotal)
{
	check_box("QueryEmulatorSensitivityUncertainty", lo, hi, number_params);
	const size_t no = (size_t)number_outputs, d = (size_t)number_params;
	std::vector<double> f(no * d), t(no * d);
	MeanVariances.assign(no, 0.0);
	IntegratedVariances.assign(no, 0.0);
	ExpectedVariances.assign(no, 0.0);
	emulate_sensitivity_uncertainty_multi(the_emulator, outputPCAValues ? 1 : 0, lo.data(), hi.data(), MeanVariances.data(),
	                                      IntegratedVariances.data(), ExpectedVariances.data(), f.data(), t.data());
	ExpectedFirstOrder.assign(no, std::vector<double>(d));
	ExpectedTotal.assign(no, std::vector<double>(d));
	for (size_t i = 0; i < no; i++)
		for (size_t j = 0; j < d; j++) {
			ExpectedFirstOrder[i][j] = f[i * d + j];
			ExpectedTotal[i][j] = t[i * d + j];
		}
}

void emulator::QueryEmulatorDesignGain(const std::vector<double> &lo, const std::vector<double> &hi, const std::vector<std::vector<double> > &xpoints,
                                       std::vector<std::vector<double> > &Gains, std::vector<double> &TotalGains)
{
	check_box("QueryEmulatorDesignGain", lo, hi, number_params);
	const size_t no = (size_t)number_outputs, np = xpoints.size();
	Gains.assign(np, std::vector<double>(no));
	TotalGains.assign(np, 0.0);
	if (np == 0) return;
	std::vector<double> flat = flatten("QueryEmulatorDesignGain", xpoints, number_params), g(np * no);
	emulate_design_gain_multi(the_emulator, outputPCAValues ? 1 : 0, lo.data(), hi.data(), (int)np, flat.data(), g.data(), TotalGains.data());
	for (size_t q = 0; q < np; q++)
		for (size_t t = 0; t < no; t++) Gains[q][t] = g[q * no + t];
}

void emulator::QueryEmulatorTargetedDesignGain(const std::vector<std::vector<double> > &targets, const std::vector<double> &weights,
                                               const std::vector<std::vector<double> > &xpoints, std::vector<std::vector<double> > &Gains,
                                               std::vector<double> &TotalGains, std::vector<double> &TargetVariances)
{
	const size_t no = (size_t)number_outputs, np = xpoints.size(), ns = targets.size();
	if (ns < 1 || ns > 65536 || (!weights.empty() && weights.size() != ns)) {
		std::cerr << "Error::QueryEmulatorTargetedDesignGain needs 1 .. 65536 targets and one weight per target, or none" << std::endl;
		gpemu_host_exit(EXIT_FAILURE);
	}
	Gains.assign(np, std::vector<double>(no));
	TotalGains.assign(np, 0.0);
	TargetVariances.assign(no, 0.0);
	std::vector<double> tflat = flatten("QueryEmulatorTargetedDesignGain", targets, number_params);
	std::vector<double> flat = flatten("QueryEmulatorTargetedDesignGain", xpoints, number_params), g(np * no + 1);
	if (np == 0) {                               // the targets alone: their variance
		std::vector<double> one(tflat.begin(), tflat.begin() + number_params), g1(no), t1(1);
		emulate_design_target_gain_multi(the_emulator, outputPCAValues ? 1 : 0, (int)ns, tflat.data(), weights.empty() ? NULL : weights.data(), 1,
		                                 one.data(), g1.data(), t1.data(), TargetVariances.data());
		return;
	}
	emulate_design_target_gain_multi(the_emulator, outputPCAValues ? 1 : 0, (int)ns, tflat.data(), weights.empty() ? NULL : weights.data(), (int)np,
	                                 flat.data(), g.data(), TotalGains.data(), TargetVariances.data());
	for (size_t q = 0; q < np; q++)
		for (size_t t = 0; t < no; t++) Gains[q][t] = g[q * no + t];
}

void emulator::QueryEmulatorDesignBatch(const std::vector<double> &lo, const std::vector<double> &hi, const std::vector<std::vector<double> > &xpoints,
                                        int BatchSize, std::vector<int> &Picks, std::vector<double> &PickGains)
{
	check_box("QueryEmulatorDesignBatch", lo, hi, number_params);
	const size_t np = xpoints.size();
	if (BatchSize < 1 || (size_t)BatchSize > np || BatchSize > 256 || np > 16384) {
		std::cerr << "Error::QueryEmulatorDesignBatch needs 1 <= BatchSize <= min(number of points, 256) and at most 16384 points" << std::endl;
		gpemu_host_exit(EXIT_FAILURE);
	}
	Picks.assign((size_t)BatchSize, -1);
	PickGains.assign((size_t)BatchSize, 0.0);
	std::vector<double> flat = flatten("QueryEmulatorDesignBatch", xpoints, number_params);
	emulate_design_batch_multi(the_emulator, outputPCAValues ? 1 : 0, lo.data(), hi.data(), (int)np, flat.data(), BatchSize, Picks.data(),
	                           PickGains.data());
}

void emulator::QueryEmulatorMainEffectBands(const std::vector<double> &lo, const std::vector<double> &hi, const std::vector<std::vector<double> > &grid,
                                            std::vector<double> &Means, std::vector<std::vector<std::vector<double> > > &Curves,
                                            std::vector<std::vector<std::vector<double> > > &Bands)
{
	check_box("QueryEmulatorMainEffectBands", lo, hi, number_params);
	const size_t no = (size_t)number_outputs, d = (size_t)number_params, G = grid.empty() ? 0 : grid[0].size();
	if (grid.size() != d || G < 1) {
		std::cerr << "Error::QueryEmulatorMainEffectBands called with a grid that has not one non-empty row per parameter" << std::endl;
		gpemu_host_exit(EXIT_FAILURE);
	}
	std::vector<double> g = flatten("QueryEmulatorMainEffectBands", grid, (int)G), m(d * G * no), s(d * G * no);
	Means.assign(no, 0.0);
	emulate_main_effects_band_multi(the_emulator, outputPCAValues ? 1 : 0, lo.data(), hi.data(), (int)G, g.data(), Means.data(), m.data(), s.data());
	Curves.assign(no, std::vector<std::vector<double> >(d, std::vector<double>(G)));
	Bands.assign(no, std::vector<std::vector<double> >(d, std::vector<double>(G)));
	for (size_t i = 0; i < no; i++)
		for (size_t j = 0; j < d; j++)
			for (size_t k = 0; k < G; k++) {
				Curves[i][j][k] = m[(j * G + k) * no + i];
				Bands[i][j][k] = s[(j * G + k) * no + i];
			}
}

void emulator::QueryEmulatorInteractions(const std::vector<double> &lo, const std::vector<double> &hi,
                                         std::vector<std::vector<double> > &PairVariances, std::vector<std::vector<double> > &SecondOrder)
{
	check_box("QueryEmulatorInteractions", lo, hi, number_params);
	const size_t no = (size_t)number_outputs, d = (size_t)number_params, np = d * (d - 1) / 2;
	std::vector<double> v(no * np), in(no * np), e0(no), var(no), f(no * d), t(no * d);
	emulate_sensitivity_pairs_multi(the_emulator, outputPCAValues ? 1 : 0, lo.data(), hi.data(), v.data(), in.data());
	emulate_sensitivity_multi(the_emulator, outputPCAValues ? 1 : 0, lo.data(), hi.data(), e0.data(), var.data(), f.data(), t.data());
	PairVariances.assign(no, std::vector<double>(np));
	SecondOrder.assign(no, std::vector<double>(np));
	for (size_t i = 0; i < no; i++)
		for (size_t p = 0; p < np; p++) {
			PairVariances[i][p] = v[i * np + p];
			SecondOrder[i][p] = var[i] != 0.0 ? in[i * np + p] / var[i] : NAN;
		}
}

void emulator::QueryEmulatorInteractionUncertainty(const std::vector<double> &lo, const std::vector<double> &hi,
                                                   std::vector<std::vector<double> > &ExpectedPairVariances,
                                                   std::vector<std::vector<double> > &ExpectedInteractions)
{
	check_box("QueryEmulatorInteractionUncertainty", lo, hi, number_params);
	const size_t no = (size_t)number_outputs, d = (size_t)number_params, np = d * (d - 1) / 2;
	std::vector<double> v(no * np), in(no * np);
	emulate_sensitivity_pairs_uncertainty_multi(the_emulator, outputPCAValues ? 1 : 0, lo.data(), hi.data(), v.data(), in.data());
	ExpectedPairVariances.assign(no, std::vector<double>(np));
	ExpectedInteractions.assign(no, std::vector<double>(np));
	for (size_t i = 0; i < no; i++)
		for (size_t p = 0; p < np; p++) {
			ExpectedPairVariances[i][p] = v[i * np + p];
			ExpectedInteractions[i][p] = in[i * np + p];
		}
}

void emulator::QueryEmulatorInteractionSurface(const std::vector<double> &lo, const std::vector<double> &hi, int j, int k,
                                               const std::vector<double> &gj, const std::vector<double> &gk, std::vector<double> &Means,
                                               std::vector<std::vector<std::vector<double> > > &Joint,
                                               std::vector<std::vector<std::vector<double> > > &Interaction)
{
	check_box("QueryEmulatorInteractionSurface", lo, hi, number_params);
	const size_t no = (size_t)number_outputs, G = gj.size();
	if (G < 1 || gk.size() != G) {
		std::cerr << "Error::QueryEmulatorInteractionSurface called with grids that are empty or differ in length" << std::endl;
		gpemu_host_exit(EXIT_FAILURE);
	}
	std::vector<double> jt(G * G * no), it(G * G * no);
	Means.assign(no, 0.0);
	emulate_interaction_surface_multi(the_emulator, outputPCAValues ? 1 : 0, lo.data(), hi.data(), j, k, (int)G, gj.data(), gk.data(), Means.data(),
	                                  jt.data(), it.data());
	Joint.assign(no, std::vector<std::vector<double> >(G, std::vector<double>(G)));
	Interaction.assign(no, std::vector<std::vector<double> >(G, std::vector<double>(G)));
	for (size_t i = 0; i < no; i++)
		for (size_t a = 0; a < G; a++)
			for (size_t b = 0; b < G; b++) {
				Joint[i][a][b] = jt[(a * G + b) * no + i];
				Interaction[i][a][b] = it[(a * G + b) * no + i];
			}
}

double emulator::ValidateHoldout(const std::vector<std::vector<double> > &xpoints, const std::vector<std::vector<double> > &Observations,
                                 std::vector<std::vector<double> > &Means, std::vector<std::vector<double> > &Variances,
                                 std::vector<std::vector<double> > &WhitenedErrors, std::vector<double> &Mahalanobis,
                                 std::vector<double> &LogDeterminant, std::vector<double> &LogDensity)
{
	const size_t np = xpoints.size(), nr = (size_t)the_model->nr;
	if (Observations.size() != np) {
		std::cerr << "Error::ValidateHoldout called with " << Observations.size() << " observations for " << np << " points" << std::endl;
		gpemu_host_exit(EXIT_FAILURE);
	}
	std::vector<double> flat = flatten("ValidateHoldout", xpoints, number_params);
	std::vector<double> y = flatten("ValidateHoldout (Observations)", Observations, the_model->nt);
	std::vector<double> m(np * nr), v(np * nr), w(np * nr);
	Mahalanobis.assign(nr, 0.0);
	LogDeterminant.assign(nr, 0.0);
	LogDensity.assign(nr, 0.0);
	double sum = 0.0;
	gsl_matrix view = gpemu_matrix_view(flat.data(), np, number_params);
	emulate_points_multi_holdout(the_emulator, &view, y.data(), NULL, m.data(), v.data(), w.data(), Mahalanobis.data(), LogDeterminant.data(),
	                             LogDensity.data(), &sum);
	Means.assign(np, std::vector<double>(nr));
	Variances.assign(np, std::vector<double>(nr));
	WhitenedErrors.assign(np, std::vector<double>(nr));
	for (size_t q = 0; q < np; q++)
		for (size_t c = 0; c < nr; c++) {
			Means[q][c] = m[q * nr + c];
			Variances[q][c] = v[q * nr + c];
			WhitenedErrors[q][c] = w[q * nr + c];
		}
	return sum;
}

void emulator::DrawEmulator(const std::vector<std::vector<double> > &xpoints, const std::vector<std::vector<std::vector<double> > > &Normals,
                            std::vector<std::vector<std::vector<double> > > &Draws)
{
	const size_t np = xpoints.size(), nr = (size_t)the_model->nr, no = (size_t)number_outputs;
	const size_t nd = Normals.empty() ? 0 : Normals[0].size();
	if (Normals.size() != nr || nd < 1) {
		std::cerr << "Error::DrawEmulator called without normals for each of the " << nr << " PCA components" << std::endl;
		gpemu_host_exit(EXIT_FAILURE);
	}
	std::vector<double> flat = flatten("DrawEmulator", xpoints, number_params);
	std::vector<double> z(nr * nd * np), out(nd * np * no);
	for (size_t c = 0; c < nr; c++) {
		if (Normals[c].size() != nd) { wrong_dimensions("DrawEmulator (Normals)"); gpemu_host_exit(EXIT_FAILURE); }
		std::vector<double> zc = flatten("DrawEmulator (Normals)", Normals[c], (int)np);
		for (size_t i = 0; i < nd * np; i++) z[c * nd * np + i] = zc[i];
	}
	gsl_matrix view = gpemu_matrix_view(flat.data(), np, number_params);
	emulate_points_multi_holdout(the_emulator, &view, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL);
	emulate_points_multi_draw(the_emulator, outputPCAValues ? 1 : 0, (int)np, (int)nd, z.data(), out.data());
	Draws.assign(nd, std::vector<std::vector<double> >(np, std::vector<double>(no)));
	for (size_t s = 0; s < nd; s++)
		for (size_t q = 0; q < np; q++)
			for (size_t i = 0; i < no; i++) Draws[s][q][i] = out[(s * np + q) * no + i];
}

void emulator::QueryEmulator(const std::vector<double> &xpoint, std::vector<double> &Means, std::vector<double> &Errors)
{
	if ((int)xpoint.size() != number_params) {
		wrong_dimensions("QueryEmulator");
		std::cerr << "xpoint.length: " << xpoint.size() << " emulator->number_params: " << number_params << std::endl;
		gpemu_host_exit(EXIT_FAILURE);
	}
	if (!Means.empty()) { std::cerr << "Error::QueryEmulator called with nonempty Means vector" << std::endl; gpemu_host_exit(EXIT_FAILURE); }
	if (!Errors.empty()) { std::cerr << "Error::QueryEmulator called with nonempty Errors vector" << std::endl; gpemu_host_exit(EXIT_FAILURE); }
	std::vector<std::vector<double> > xs(1, xpoint), mm, ee;
	QueryEmulator(xs, mm, ee);
	Means = mm[0];
	Errors = ee[0];
}

void emulator::getEmulatorPCA(std::vector<double> *pca_evals, std::vector<std::vector<double> > *pca_evecs,
                              std::vector<double> *pca_mean)
{
	const int nt = the_model->nt, nr = the_model->nr;
	pca_evals->assign(nr, 0.0);
	pca_mean->assign(nt, 0.0);
	pca_evecs->assign(nt, std::vector<double>(nr, 0.0));
	for (int i = 0; i < nr; i++) (*pca_evals)[i] = gsl_vector_get(the_model->pca_evals_r, i);
	for (int i = 0; i < nt; i++) {
		(*pca_mean)[i] = gsl_vector_get(the_model->training_mean, i);
		for (int j = 0; j < nr; j++) (*pca_evecs)[i][j] = gsl_matrix_get(the_model->pca_evecs_r, i, j);
	}
}
