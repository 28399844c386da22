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
	number_outputs = pca ? the_model->nr : the_model->nt;
	number_params = the_model->nparams;
}

emulator::emulator(std::string path) { init(path, false); }
emulator::emulator(std::string path, bool PcaOnly) { init(path, PcaOnly); }
emulator::~emulator() { free_multi_emulator(the_emulator); }

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
