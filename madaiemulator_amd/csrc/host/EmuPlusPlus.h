// EmuPlusPlus.h -- C++ query class over a trained emulator, same public interface as the reference's
// src/EmuPlusPlus.h:31-65 (class emulator: constructors from a MODEL_SNAPSHOT_FILE, QueryEmulator returning
// means and sqrt(variance), getEmulatorPCA), plus a batched QueryEmulator: MCMC drivers that hold many
// proposals should pass them in one call -- the posterior sweep is one GEMM over the query block.
#ifndef GPEMU_EMUPLUSPLUS_H
#define GPEMU_EMUPLUSPLUS_H

#include <string>
#include <vector>
extern "C" {
#include "libemu.h"
}

class emulator {
public:
	explicit emulator(std::string StateFilePath);                 // outputs in the observable (Y) space
	emulator(std::string StateFilePath, bool PcaOnly);            // PcaOnly: outputs left in the PCA space
	~emulator();
	// Means / Errors must be empty on entry; Errors = sqrt(variance)  (EmuPlusPlus.cpp:137-178)
	void QueryEmulator(const std::vector<double> &xpoint, std::vector<double> &Means, std::vector<double> &Errors);
	// batch: one row per query point; Means[q], Errors[q] have number_outputs entries
	void QueryEmulator(const std::vector<std::vector<double> > &xpoints, std::vector<std::vector<double> > &Means,
	                   std::vector<std::vector<double> > &Errors);
	// the means alone, one row per query point: the device's mean-only sweep (no variance, no product with L^-1); agrees
	// with QueryEmulator's Means to rounding
	void QueryEmulatorMeans(const std::vector<std::vector<double> > &xpoints, std::vector<std::vector<double> > &Means);
	// the means and their gradients with respect to the query point: Gradients[q] has number_outputs x number_params entries,
	// row-major (output i, parameter j at i * number_params + j)
	void QueryEmulatorMeanGradients(const std::vector<std::vector<double> > &xpoints, std::vector<std::vector<double> > &Means,
	                                std::vector<std::vector<double> > &Gradients);
	// means, variances and the gradients of both with respect to the query point.  Variances, NOT their square roots
	// (QueryEmulator returns Errors = sqrt(variance)): the derivative of an error bar is undefined where the variance rounds
	// to <= 0, so the caller forms grad(sqrt(var)) = VarianceGradients / (2 sqrt(Variances)) where it is positive.
	// MeanGradients[q] and VarianceGradients[q] have number_outputs x number_params entries, row-major
	void QueryEmulatorGradients(const std::vector<std::vector<double> > &xpoints, std::vector<std::vector<double> > &Means,
	                            std::vector<std::vector<double> > &Variances, std::vector<std::vector<double> > &MeanGradients,
	                            std::vector<std::vector<double> > &VarianceGradients);
	// the means and, per output, the joint posterior covariance between the query points: Covariances[t] is the flattened
	// xpoints.size() x xpoints.size() matrix of output t, row-major (points p, q at p * xpoints.size() + q).  The COVARIANCE,
	// not a square root: QueryEmulator returns Errors = sqrt(variance), so Covariances[t][q * (np + 1)] = Errors[q][t]^2 to
	// rounding.  Covariances between different outputs are not modelled (libemu.h: emulate_points_multi_cov).
	void QueryEmulatorCovariance(const std::vector<std::vector<double> > &xpoints, std::vector<std::vector<double> > &Means,
	                             std::vector<std::vector<double> > &Covariances);
	// validation on a held-out campaign (libemu.h: emulate_points_multi_holdout): Observations[q] holds the nt observed outputs
	// at xpoints[q], in observable space whatever PcaOnly says; they are projected onto the nr PCA components, and every
	// component c answers in PCA space -- the diagnostics do not exist in observable space, where the covariance is singular
	// whenever nr < nt.  Means[q][c], Variances[q][c], WhitenedErrors[q][c] (decorrelated errors, independent N(0, 1) under the
	// model); Mahalanobis[c], LogDeterminant[c], LogDensity[c] per component.  Returns the sum of LogDensity: the joint log
	// predictive density of the projected observations.  The factors stay resident for DrawEmulator.
	double ValidateHoldout(const std::vector<std::vector<double> > &xpoints, const std::vector<std::vector<double> > &Observations,
	                       std::vector<std::vector<double> > &Means, std::vector<std::vector<double> > &Variances,
	                       std::vector<std::vector<double> > &WhitenedErrors, std::vector<double> &Mahalanobis,
	                       std::vector<double> &LogDeterminant, std::vector<double> &LogDensity);
	// joint draws at xpoints from the emulator's posterior, Normals[c][s] the xpoints.size() standard normals of PCA component c
	// for draw s (the caller's generator): Draws[s][q] has number_outputs entries, in observable space unless PcaOnly.  Factors
	// the joint covariance at xpoints first (no noise); coinciding points end in the layer's fatal exit.
	void DrawEmulator(const std::vector<std::vector<double> > &xpoints, const std::vector<std::vector<std::vector<double> > > &Normals,
	                  std::vector<std::vector<std::vector<double> > > &Draws);
	// the input measure of every sensitivity method below, per parameter: 0 uniform on [lo_j, hi_j] (the default), 1 Gaussian with
	// MEAN lo_j and STANDARD DEVIATION hi_j (libemu.h: emulate_sensitivity_measure_multi); an empty vector: all uniform.  It holds
	// for every later call until it is set again.  A vector of another length or another kind ends in the layer's fatal exit.
	void SetSensitivityMeasure(const std::vector<int> &kind);
	// sensitivity analysis of the posterior mean over the box [lo, hi] (number_params entries each; independent uniform inputs),
	// in closed form, power-exponential covariance only (libemu.h: emulate_sensitivity_multi).  Per output t: Means[t] = E0,
	// Variances[t] = V, FirstOrder[t][j] = V_j / V and Total[t][j] = VT_j / V, the first-order and total-effect Sobol indices of
	// parameter j (NaN where V = 0).  In observable space the cross-covariances between the PCA components are included.
	void QueryEmulatorSensitivity(const std::vector<double> &lo, const std::vector<double> &hi, std::vector<double> &Means,
	                              std::vector<double> &Variances, std::vector<std::vector<double> > &FirstOrder,
	                              std::vector<std::vector<double> > &Total);
	// main-effect curves: grid[j] holds the values of parameter j (number_params rows of equal length G);
	// Curves[t][j][g] = E[output t | x_j = grid[j][g]], Means[t] = E0
	void QueryEmulatorMainEffects(const std::vector<double> &lo, const std::vector<double> &hi, const std::vector<std::vector<double> > &grid,
	                              std::vector<double> &Means, std::vector<std::vector<std::vector<double> > > &Curves);
	// the emulator's own uncertainty about that analysis (libemu.h: emulate_sensitivity_uncertainty_multi), in variance units, not
	// divided by V.  Per output t: MeanVariances[t] = Var*[E0], IntegratedVariances[t] = the box average of the posterior variance,
	// ExpectedVariances[t] = E*[V], ExpectedFirstOrder[t][j] = E*[V_j], ExpectedTotal[t][j] = E*[VT_j].  In observable space the
	// uncertainty terms take the squared rule over the PCA components (independent a posteriori), the plug-in part its cross terms.
	void QueryEmulatorSensitivityUncertainty(const std::vector<double> &lo, const std::vector<double> &hi, std::vector<double> &MeanVariances,
	                                         std::vector<double> &IntegratedVariances, std::vector<double> &ExpectedVariances,
	                                         std::vector<std::vector<double> > &ExpectedFirstOrder,
	                                         std::vector<std::vector<double> > &ExpectedTotal);
	// where to put the next model run (libemu.h: emulate_design_gain_multi): Gains[q][t] = how much IntegratedVariances[t] drops
	// when the design gets one more run at xpoints[q], the hyper-parameters as they are; TotalGains[q] its sum over the outputs
	void QueryEmulatorDesignGain(const std::vector<double> &lo, const std::vector<double> &hi, const std::vector<std::vector<double> > &xpoints,
	                             std::vector<std::vector<double> > &Gains, std::vector<double> &TotalGains);
	// the same for a region given as weighted points (libemu.h: emulate_design_target_gain_multi): targets[s] the points (chain
	// samples, the non-implausible set, quadrature nodes), weights one per target or empty for 1 / size each.  TargetVariances[t] =
	// the weighted posterior variance of output t over the targets, Gains[q][t] how much it drops by one more run at xpoints[q],
	// TotalGains[q] the sum over the outputs.  Every covariance function.
	void QueryEmulatorTargetedDesignGain(const std::vector<std::vector<double> > &targets, const std::vector<double> &weights,
	                                     const std::vector<std::vector<double> > &xpoints, std::vector<std::vector<double> > &Gains,
	                                     std::vector<double> &TotalGains, std::vector<double> &TargetVariances);
	// a batch of BatchSize runs chosen greedily among xpoints (libemu.h: emulate_design_batch_multi): Picks[j] the index of pick j,
	// PickGains[j] how much the sum of IntegratedVariances drops by it, given the picks before it
	void QueryEmulatorDesignBatch(const std::vector<double> &lo, const std::vector<double> &hi, const std::vector<std::vector<double> > &xpoints,
	                              int BatchSize, std::vector<int> &Picks, std::vector<double> &PickGains);
	// QueryEmulatorMainEffects with Bands[t][j][g] = the posterior standard deviation of E[output t | x_j = grid[j][g]]
	void QueryEmulatorMainEffectBands(const std::vector<double> &lo, const std::vector<double> &hi, const std::vector<std::vector<double> > &grid,
	                                  std::vector<double> &Means, std::vector<std::vector<std::vector<double> > > &Curves,
	                                  std::vector<std::vector<std::vector<double> > > &Bands);
	// second order (libemu.h: emulate_sensitivity_pairs_multi): pairs j < k of parameters at p = j (2 number_params - j - 1) / 2 +
	// (k - j - 1).  Per output t: PairVariances[t][p] = V_jk = Var(E[output | x_j, x_k]) and SecondOrder[t][p] =
	// (V_jk - V_j - V_k) / V, the second-order Sobol index (NaN where V = 0).  number_params >= 2.
	void QueryEmulatorInteractions(const std::vector<double> &lo, const std::vector<double> &hi, std::vector<std::vector<double> > &PairVariances,
	                               std::vector<std::vector<double> > &SecondOrder);
	// the emulator's own uncertainty about them (emulate_sensitivity_pairs_uncertainty_multi), in variance units:
	// ExpectedPairVariances[t][p] = E*[V_jk], ExpectedInteractions[t][p] = E*[V_jk - V_j - V_k]
	void QueryEmulatorInteractionUncertainty(const std::vector<double> &lo, const std::vector<double> &hi,
	                                         std::vector<std::vector<double> > &ExpectedPairVariances,
	                                         std::vector<std::vector<double> > &ExpectedInteractions);
	// the two-way surface of parameters j != k on the grid gj x gk (equal lengths G): Joint[t][a][b] = E[output t | x_j = gj[a],
	// x_k = gk[b]], Interaction[t][a][b] = Joint - main effect of j - main effect of k + E0, Means[t] = E0
	void QueryEmulatorInteractionSurface(const std::vector<double> &lo, const std::vector<double> &hi, int j, int k, const std::vector<double> &gj,
	                                     const std::vector<double> &gk, std::vector<double> &Means,
	                                     std::vector<std::vector<std::vector<double> > > &Joint,
	                                     std::vector<std::vector<std::vector<double> > > &Interaction);
	// calibration against observations (libemu.h: alloc_observations, emulate_points_multi_implausibility, _nonimplausible).
	// SetObservations: Values (nt observed outputs, observable space whatever PcaOnly says) with StandardDeviations (nt) or, if
	// not empty, Covariance (nt x nt row-major, replaces the squared standard deviations), and RelativeErrors (nt, or empty: none);
	// replaces an earlier set.  A malformed set ends in the layer's fatal exit.  Statistics[q] = {chi2, joint log density,
	// largest, second and third largest per-output implausibility}, WorstOutput[q] the output of the largest.
	// QueryEmulatorNonImplausible keeps point q iff chi2 <= CutChi2 and the Level-th largest implausibility (1, 2 or 3) <= CutI
	// (INFINITY disables a cut): Kept holds the indices in ascending order, Statistics their rows; only those leave the device.
	void SetObservations(const std::vector<double> &Values, const std::vector<double> &StandardDeviations,
	                     const std::vector<double> &Covariance, const std::vector<double> &RelativeErrors);
	void QueryEmulatorImplausibility(const std::vector<std::vector<double> > &xpoints, std::vector<std::vector<double> > &Statistics,
	                                 std::vector<int> &WorstOutput);
	void QueryEmulatorNonImplausible(const std::vector<std::vector<double> > &xpoints, double CutChi2, int Level, double CutI,
	                                 std::vector<int> &Kept, std::vector<std::vector<double> > &Statistics);
	// the joint log density of the observations at every point and its gradient with respect to the point's parameters
	// (libemu.h: emulate_points_multi_logpdf_grad): LogLikelihoods[q] is Statistics[q][1] of QueryEmulatorImplausibility bit
	// for bit, Gradients[q][j] its derivative in the units of xpoints.  Requires SetObservations.
	void QueryEmulatorLogLikelihoodGradient(const std::vector<std::vector<double> > &xpoints, std::vector<double> &LogLikelihoods,
	                                        std::vector<std::vector<double> > &Gradients);
	// posterior samples of the parameters by the ensemble sampler on the device (libemu.h: emulate_sample_posterior_multi), after
	// SetObservations.  lo, hi, kind: the prior per parameter (kind empty: all uniform on [lo, hi]; kind[j] = 1: Gaussian with mean
	// lo[j] and standard deviation hi[j]).  Starts: Walkers rows of number_params, or empty: drawn from the prior.  Samples[r] is
	// the r-th recorded sample (recorded step r / Walkers, walker r % Walkers), LogPosteriors[r] its log posterior; Summary has
	// six rows of number_params: mean, standard deviation, the 2.5 / 50 / 97.5 % quantiles, the integrated autocorrelation time
	// of the ensemble mean.  Returns the accepted fraction of the proposals.
	double SamplePosterior(const std::vector<double> &lo, const std::vector<double> &hi, const std::vector<int> &kind, int Walkers,
	                       int Steps, int Burn, int Thin, unsigned long long Seed, double Stretch,
	                       const std::vector<std::vector<double> > &Starts, std::vector<std::vector<double> > &Samples,
	                       std::vector<double> &LogPosteriors, std::vector<std::vector<double> > &Summary);
	void getEmulatorPCA(std::vector<double> *pca_evals, std::vector<std::vector<double> > *pca_evecs,
	                    std::vector<double> *pca_mean);
	int getRegressionOrder(void) { return the_model->regression_order; }
	int getCovFnIndex(void) { return the_model->cov_fn_index; }
	int number_params;
	int number_outputs;

private:
	void init(const std::string &path, bool pca);
	bool outputPCAValues;
	std::string StateFilePath;
	multi_modelstruct *the_model;
	multi_emulator *the_emulator;
	gpemu_observations *the_observations;
};
#endif
